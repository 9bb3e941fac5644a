"""NumPy model of the Q3_K format (ggml type 11) and of the Q3_K x Q8_1 product contract (include/qg/qg.h, "Q3_K
weights"), written from the format description and independent of the library.

block_q3_K, 110 bytes, 256 elements: hmask[32], qs[64], scales[12], f16 d (the layout: include/qg/blocks.h). Q8_1 block
b = 4h + j of super-block sb is activation block 8 sb + b and meets the scale groups 2b, 2b + 1:
isum = s_2b * sum_{l<16} q a + s_2b+1 * sum_{l>=16} q a (int32, s = sc - 32),  C = sum_sb d * sum_b d_a * float(isum).
"""
from __future__ import annotations

import numpy as np

from kquant_ref import _f16_bytes, dev_at, q8_1_fields, random_q8_1, tol  # noqa: F401  (re-exported for the tests)

Q3_K = 11
BYTES = 110
MMQ_W = 7  # partial sums the MFMA prefill chains per output beyond its K/32 terms (Q3K_MMQ_W, csrc/qg_q3k.hpp)
_G = np.arange(16)


def fields(b: np.ndarray):
    """b: uint8 [..., 110] -> d (float32 [...]), sc (int32 [..., 16], 0..63), q (int32 [..., 8, 32], -4..3, block and
    element order)."""
    b = np.ascontiguousarray(b, np.uint8)
    assert b.shape[-1] == BYTES
    hm, qs, s = b[..., 0:32].astype(np.int32), b[..., 32:96].astype(np.int32), b[..., 96:108].astype(np.int32)
    d = b[..., 108:110].copy().view(np.float16)[..., 0].astype(np.float32)
    low4 = np.where(_G < 8, s[..., _G % 8] & 15, s[..., _G % 8] >> 4)
    sc = low4 | (((s[..., 8 + _G % 4] >> (2 * (_G // 4))) & 3) << 4)
    blk = np.arange(8)[:, None]  # b = 4h + j
    lo2 = (qs.reshape(b.shape[:-1] + (2, 32))[..., np.arange(8) // 4, :] >> (2 * (blk % 4))) & 3
    hb = (hm[..., None, :] >> blk) & 1
    return d, sc, lo2 - 4 * (1 - hb)


def build(d, sc, q) -> np.ndarray:
    """The inverse of fields(): d [...], sc [..., 16] in 0..63, q [..., 8, 32] in -4..3 -> uint8 [..., 110]."""
    d, sc, q = np.asarray(d), np.asarray(sc, np.int32), np.asarray(q, np.int32)
    b = np.zeros(d.shape + (BYTES,), np.uint8)
    u = q + 4
    blk = np.arange(8)[:, None]
    b[..., 0:32] = (((u >> 2) & 1) << blk).sum(-2)
    lo = (u & 3) << (2 * (blk % 4))
    b[..., 32:96] = np.concatenate([lo[..., 0:4, :].sum(-2), lo[..., 4:8, :].sum(-2)], axis=-1)
    b[..., 96:104] = (sc[..., 0:8] & 15) | ((sc[..., 8:16] & 15) << 4)
    hi = sc >> 4
    b[..., 104:108] = hi[..., 0:4] | (hi[..., 4:8] << 2) | (hi[..., 8:12] << 4) | (hi[..., 12:16] << 6)
    b[..., 108:110] = _f16_bytes(d)
    return b


def dequantize(b: np.ndarray) -> np.ndarray:
    """float32 [..., 256 * super-blocks] = (d * float(sc - 32)) * float(q), each product rounded to fp32."""
    d, sc, q = fields(b)
    dl = (d[..., None] * (sc - 32).astype(np.float32)).astype(np.float32)  # [..., 16]
    y = (np.repeat(dl, 16, axis=-1) * q.reshape(q.shape[:-2] + (256,)).astype(np.float32)).astype(np.float32)
    return y.reshape(b.shape[:-2] + (-1,))


def gemm(aq: np.ndarray, bq: np.ndarray):
    """aq [M, K/32, 36] Q8_1, bq [N, K/256, 110] Q3_K -> (C float64 [M, N], isum int32 [M, N, K/32], mag float64
    [M, N] = sum |d d_a isum|). Every term is exact in float64 (11 + 11 + 20 significant bits)."""
    d, sc, q = fields(bq)
    n, nsb = d.shape
    da, _, qa = q8_1_fields(aq)
    w = (q * np.repeat(sc - 32, 16, axis=-1).reshape(n, nsb, 8, 32)).reshape(n, nsb * 8, 32)  # q s, |.| <= 128
    assert da.shape[1] == w.shape[1]
    # per block a [M, 32] x [32, N] product; float64 holds these integers exactly
    s = np.matmul(qa.transpose(1, 0, 2).astype(np.float64), w.transpose(1, 2, 0).astype(np.float64))
    isum = np.ascontiguousarray(s.transpose(1, 2, 0)).astype(np.int32)  # [M, N, nb]
    t = np.repeat(d.astype(np.float64), 8, axis=1)[None] * da[:, None, :] * isum
    return t.sum(-1), isum, np.abs(t).sum(-1)


def random_q3k(rng, n: int, k: int) -> np.ndarray:
    """[n, k/256, 110]: every hmask, qs and scales byte uniform in 0..255 (all 64 scales, all 8 codes), d in +-0.01."""
    b = rng.integers(0, 256, (n, k // 256, BYTES), dtype=np.uint8)
    b[..., 108:110] = _f16_bytes(rng.uniform(-0.01, 0.01, (n, k // 256)))
    return b


EXTREME_D = (2.0 ** -24, -1023 * 2.0 ** -24, 2.0 ** -14, 65504.0, -65504.0, 0.0, -0.25)
EXTREME_SC = (0, 32, 63)
D0_ROW, SC32_ROW = 5, len(EXTREME_D) + 1  # the rows that come out exactly 0
MAX_ROW = len(EXTREME_D) + len(EXTREME_SC)  # qs = hmask = 0 (q = -4), sc = 0 (s = -32): q s = +128, the operand byte -128
ROWS = MAX_ROW + 3  # then sc = 63 with q = -4 (q s = -124) and sc = 0 with q = 3 (q s = -96)


def extremes(rng, m: int, k: int = 512):
    """Q8_1 [m, k/32, 36] and Q3_K [ROWS, k/256, 110], one class per weight row: rows 0..6 d = EXTREME_D, 7..9 every
    sc = 0, 32, 63, then (q, sc) = (-4, 0), (-4, 63), (3, 0) with d = 1. Token 0: d_a = 1 and every byte -128, so isum
    of row 10 is -2^19, the contract's maximum; the last token d_a = 65504. No Inf, no NaN."""
    bq = random_q3k(rng, ROWS, k)
    for r, d in enumerate(EXTREME_D):
        bq[r, :, 108:110] = _f16_bytes(np.float64(d))
    for r, v in enumerate(EXTREME_SC):
        bq[len(EXTREME_D) + r, :, 96:108] = build(0.0, np.full(16, v), np.zeros((8, 32)))[96:108]
    for r, (v, q) in enumerate(((0, -4), (63, -4), (0, 3))):
        bq[MAX_ROW + r] = build(1.0, np.full(16, v), np.full((8, 32), q))
    aq = random_q8_1(rng, m, k)
    aq[0, :, 0:2] = _f16_bytes(np.float64(1.0))
    aq[0, :, 4:] = 0x80
    aq[m - 1, :, 0:2] = _f16_bytes(np.float64(65504.0))
    return aq, bq
