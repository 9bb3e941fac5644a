"""NumPy model of the IQ4_XS format (ggml type 23) and of the IQ4_XS x Q8_1 product contract (include/qg/qg.h, "IQ4_XS
weights"), written from the format description and independent of the library.

block_iq4_xs, 136 bytes, 256 elements: f16 d, u16 scales_h, scales_l[4], qs[128]. Sub-block j owns qs[16j .. 16j + 15]:
element 32j + i has the code qs[16j + i] & 15, element 32j + 16 + i the code qs[16j + i] >> 4; its 6-bit scale is
ls_j = ((scales_l[j / 2] >> 4 (j % 2)) & 15) | (((scales_h >> 2j) & 3) << 4). Sub-block j of super-block sb meets Q8_1
block 8 sb + j:  sumi = sum_i KV[code_i] * a_i (int32),  C = sum_sb d * sum_j d_a * float((ls_j - 32) * sumi).
"""
from __future__ import annotations

import numpy as np

from kquant_ref import _f16_bytes, dev_at, q8_1_fields, random_q8_1, tol  # noqa: F401  (re-exported for the tests)

IQ4_XS = 23
BYTES = 136
KV = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.int32)
MMQ_W = 8  # partial sums the MFMA prefill chains per output beyond its K/32 terms (IQ4XS_MMQ_W, csrc/qg_iq4xs.hpp)


def fields(b: np.ndarray):
    """b: uint8 [..., 136] -> d (float32 [...]), ls (int32 [..., 8], 0..63), code (int32 [..., 8, 32], element order)."""
    b = np.ascontiguousarray(b, np.uint8)
    assert b.shape[-1] == BYTES
    d = b[..., 0:2].copy().view(np.float16)[..., 0].astype(np.float32)
    sh = b[..., 2].astype(np.int32) | (b[..., 3].astype(np.int32) << 8)
    j = np.arange(8)
    ls = ((b[..., 4:8].astype(np.int32)[..., j // 2] >> (4 * (j % 2))) & 15) | (((sh[..., None] >> (2 * j)) & 3) << 4)
    qs = b[..., 8:].astype(np.int32).reshape(b.shape[:-1] + (8, 16))
    return d, ls, np.concatenate([qs & 15, qs >> 4], axis=-1)


def build(d, ls, code) -> np.ndarray:
    """The inverse of fields(): d [...], ls [..., 8] in 0..63, code [..., 8, 32] in 0..15 -> uint8 [..., 136]."""
    d, ls, code = np.asarray(d), np.asarray(ls, np.int32), np.asarray(code, np.uint8)
    b = np.zeros(d.shape + (BYTES,), np.uint8)
    b[..., 0:2] = _f16_bytes(d)
    sh = ((ls >> 4) << (2 * np.arange(8))).sum(-1)
    b[..., 2], b[..., 3] = sh & 255, sh >> 8
    b[..., 4:8] = (ls[..., 0::2] & 15) | ((ls[..., 1::2] & 15) << 4)
    b[..., 8:] = (code[..., :16] | (code[..., 16:] << 4)).reshape(d.shape + (128,))
    return b


def dequantize(b: np.ndarray) -> np.ndarray:
    """float32 [..., 256 * super-blocks] = (d * float(ls - 32)) * float(KV[code]), each product rounded to fp32."""
    d, ls, code = fields(b)
    dl = (d[..., None] * (ls - 32).astype(np.float32)).astype(np.float32)
    y = (dl[..., None] * KV[code].astype(np.float32)).astype(np.float32)
    return y.reshape(b.shape[:-2] + (-1,))


def gemm(aq: np.ndarray, bq: np.ndarray):
    """aq [M, K/32, 36] Q8_1, bq [N, K/256, 136] IQ4_XS -> (C float64 [M, N], sumi int32 [M, N, K/32], mag float64
    [M, N] = sum |d d_a (ls - 32) sumi|). Every term is exact in float64 (11 + 11 + 24 significant bits)."""
    d, ls, code = fields(bq)
    n, nsb = d.shape
    da, _, qa = q8_1_fields(aq)
    kv = KV[code].reshape(n, nsb * 8, 32)
    assert da.shape[1] == kv.shape[1]
    # per block a [M, 32] x [32, N] product; float64 holds these integers exactly
    s = np.matmul(qa.transpose(1, 0, 2).astype(np.float64), kv.transpose(1, 2, 0).astype(np.float64))
    sumi = np.ascontiguousarray(s.transpose(1, 2, 0)).astype(np.int32)  # [M, N, nb]
    scale = (np.repeat(d.astype(np.float64), 8, axis=1) * (ls.reshape(n, -1) - 32))[None] * da[:, None, :]
    t = scale * sumi
    return t.sum(-1), sumi, np.abs(t).sum(-1)


def random_iq4xs(rng, n: int, k: int) -> np.ndarray:
    """[n, k/256, 136]: every header and qs byte uniform in 0..255 (all 64 scales, all 16 codes), d in +-0.01 (f16)."""
    b = rng.integers(0, 256, (n, k // 256, BYTES), dtype=np.uint8)
    b[..., 0:2] = _f16_bytes(rng.uniform(-0.01, 0.01, (n, k // 256)))
    return b


EXTREME_D = (2.0 ** -24, -1023 * 2.0 ** -24, 2.0 ** -14, 65504.0, -65504.0, 0.0, -0.25)
EXTREME_LS = (0, 32, 63)
MAX_ROW = len(EXTREME_D) + len(EXTREME_LS)  # all codes 0 (-127), ls = 0: against activations of -128 the largest product


def extremes(rng, m: int, k: int = 512):
    """Q8_1 [m, k/32, 36] and IQ4_XS [11, k/256, 136], one class per weight row: rows 0..6 d = EXTREME_D with random
    scales and codes; 7..9 every ls = 0, 32, 63; 10 every code 0 and ls = 0. Token 0: d_a = 1 and every byte -128, so
    |(ls - 32) * sumi| of row 10 is 16646144, the contract's maximum; the last token d_a = 65504. No Inf, no NaN."""
    bq = random_iq4xs(rng, MAX_ROW + 1, k)
    for r, d in enumerate(EXTREME_D):
        bq[r, :, 0:2] = _f16_bytes(np.float64(d))
    for r, v in enumerate(EXTREME_LS):
        bq[len(EXTREME_D) + r, :, 2:8] = build(0.0, np.full(8, v), np.zeros((8, 32)))[2:8]
    bq[MAX_ROW, :, 2:] = 0
    aq = random_q8_1(rng, m, k)
    aq[0, :, 0:2] = _f16_bytes(np.float64(1.0))
    aq[0, :, 4:] = 0x80
    aq[m - 1, :, 0:2] = _f16_bytes(np.float64(65504.0))
    return aq, bq
