"""NumPy model of the MXFP4 format (ggml type 39) and of the MXFP4 x Q8_1 product contract (include/qg/qg.h, "MXFP4
weights"), written from the format description and independent of the library.

block_mxfp4, 17 bytes, 32 elements: an E8M0 scale byte e, then qs[16]; element j (0..15) has the code qs[j] & 15,
element j + 16 the code qs[j] >> 4. A code indexes KV, the doubled E2M1 values; scale(e) = 2^(e - 128), built from its
fp32 bits. Block b of a weight row meets Q8_1 block b of the activation row:
  sumi = sum_j KV[code_j] * a_j (int32),  C = sum_b (d_a * scale(e)) * float(sumi).
"""
from __future__ import annotations

import numpy as np

from kquant_ref import _f16_bytes, dev_at, q8_1_fields, random_q8_1, tol  # noqa: F401  (re-exported for the tests)

MXFP4 = 39
BYTES = 17
KV = np.array([0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12], np.int32)
MMQ_W = 8  # partial sums the MFMA prefill chains per output (MXFP4_MMQ_W, csrc/qg_mxfp4.hpp): its 8 K-slice partials


def scale_bits(e) -> np.ndarray:
    """uint32 bits of scale(e): e < 2 ? 0x00200000 << e : (e - 1) << 23."""
    e = np.asarray(e).astype(np.uint32)
    return np.where(e < 2, np.uint32(0x00200000) << e, (np.maximum(e, 1) - 1) << np.uint32(23)).astype(np.uint32)


def scale(e) -> np.ndarray:
    """float32 2^(e - 128), from the bits (subnormal for e < 2)."""
    return scale_bits(e).view(np.float32)


def codes(b: np.ndarray) -> np.ndarray:
    """b: uint8 [..., 17] -> the 4-bit codes, int32 [..., 32], in element order."""
    b = np.ascontiguousarray(b, np.uint8)
    assert b.shape[-1] == BYTES
    qs = b[..., 1:17].astype(np.int32)
    return np.concatenate([qs & 15, qs >> 4], axis=-1)


def build(e, code) -> np.ndarray:
    """The inverse: e [...], code [..., 32] in 0..15 -> uint8 [..., 17]."""
    e, code = np.asarray(e), np.asarray(code, np.uint8)
    b = np.zeros(e.shape + (BYTES,), np.uint8)
    b[..., 0] = e
    b[..., 1:17] = code[..., :16] | (code[..., 16:] << 4)
    return b


def dequantize(b: np.ndarray) -> np.ndarray:
    """float32 [..., 32 * blocks] = float(KV[code]) * scale(e): exact for every (code, e), +0.0 for code 8."""
    b = np.ascontiguousarray(b, np.uint8)
    y = KV[codes(b)].astype(np.float32) * scale(b[..., 0])[..., None]
    return y.reshape(b.shape[:-2] + (-1,))


def _terms(aq: np.ndarray, bq: np.ndarray):
    da, _, qa = q8_1_fields(aq)
    kv = KV[codes(bq)]  # [N, nb, 32]
    assert da.shape[1] == kv.shape[1]
    # per block b a [M, 32] x [32, N] product; float64 holds these integers (< 2^53) exactly
    s = np.matmul(qa.transpose(1, 0, 2).astype(np.float64), kv.transpose(1, 2, 0).astype(np.float64))
    sumi = np.ascontiguousarray(s.transpose(1, 2, 0)).astype(np.int32)  # [M, N, nb]
    ds = da[:, None, :] * scale(bq[..., 0]).astype(np.float64)[None]    # [M, N, nb]: d_a * scale(e), exact in float64
    return ds, sumi


def gemm(aq: np.ndarray, bq: np.ndarray):
    """aq [M, K/32, 36] Q8_1, bq [N, K/32, 17] MXFP4 -> (C float64 [M, N], sumi int32 [M, N, K/32], mag float64 [M, N] =
    sum_b |d_a scale(e) sumi|). Every term is exact in float64 (11 + 24 significant bits, exponents above 2^-180)."""
    ds, sumi = _terms(aq, bq)
    t = ds * sumi
    return t.sum(-1), sumi, np.abs(t).sum(-1)


def subnormal_slack(aq: np.ndarray, bq: np.ndarray) -> np.ndarray:
    """float64 [M, N]: 2^-149 per term of the output that lies below 2^-126, or whose d_a * scale(e) does (the contract's
    allowance for fp32 subnormals). Zero for every output whose terms and scales are all normal or zero."""
    ds, sumi = _terms(aq, bq)
    t = np.abs(ds * sumi)
    small = ((t > 0) & (t < 2.0 ** -126)) | ((np.abs(ds) > 0) & (np.abs(ds) < 2.0 ** -126) & (sumi != 0))
    return small.sum(-1) * 2.0 ** -149


def contract_bound(aq: np.ndarray, bq: np.ndarray, w: int) -> np.ndarray:
    """The bound as qg.h states it, without the 1e-30 floor tol() adds (which hides everything below 2^-100):
    2 (K/32 + w + 2) 2^-24 mag plus 2^-149 per subnormal term."""
    nb = aq.shape[1]
    return 2.0 * (nb + w + 2) * 2.0 ** -24 * gemm(aq, bq)[2] + subnormal_slack(aq, bq)


def lossy_scale_slack(aq: np.ndarray, bq: np.ndarray) -> np.ndarray:
    """float64 [M, N]: the allowance where d_a * scale(e) is itself not an fp32 number (it lies below 2^-126 and is no
    multiple of 2^-149): rounding it costs at most 2^-150, the term then 2^-150 |sumi|, and the product's own rounding
    2^-150 more. Zero wherever d_a * scale(e) is exact in fp32."""
    ds, sumi = _terms(aq, bq)
    lossy = ds.astype(np.float32).astype(np.float64) != ds
    return (lossy * (np.abs(sumi) + 1.0)).sum(-1) * 2.0 ** -150


def random_mxfp4(rng, n: int, k: int) -> np.ndarray:
    """[n, k/32, 17]: every qs byte uniform over 0..255, e uniform in 110..135 (scales 2^-18 .. 2^7)."""
    b = rng.integers(0, 256, (n, k // 32, BYTES), dtype=np.uint8)
    b[..., 0] = rng.integers(110, 136, (n, k // 32), dtype=np.uint8)
    return b


EXTREME_E = (0, 1, 2, 3, 126, 127, 128, 129)
EXTREME_ROWS = 13   # weight rows extremes() gives a class of their own; the rest are random_mxfp4 rows
F16_MIN_NORMAL = 2.0 ** -14
F16_MAX = 65504.0
# f16 subnormals whose product with every scale(e), e >= 0, is an fp32 number (powers of two, at least 2^-21)
F16_SUBNORMALS_EXACT = (2.0 ** -15, 2.0 ** -20, 2.0 ** -17, 2.0 ** -21)
# f16 subnormals whose product with scale(0..2) is not (2^-152, 3 2^-152, 1023 2^-152 and their doubles)
F16_SUBNORMALS_LOSSY = (2.0 ** -24, 3 * 2.0 ** -24, 1023 * 2.0 ** -24)


def extremes(rng, n: int = 16, k: int = 512, lossy: bool = False):
    """Q8_1 [4, k/32, 36] and MXFP4 [n, k/32, 17] at the ends of the scale formats, one class per weight row and per
    token (an output's tolerance follows its own magnitude, so no row's extreme hides another's).

    Weight rows 0..7: e = 0, 1, 2, 3, 126, 127, 128, 129 in every block, random codes. 8: every code 0; 9: every code 8
    (the other zero); 10: every code 7 (+12); 11: every code 15 (-12); 12: e = 160 .. 200 along the blocks. The rest
    random. Tokens: 0 d_a f16 subnormals, 1 the smallest normal 2^-14, 2 d_a = 1.0 with block 0 all -128 (|sumi| =
    32 * 12 * 128 against rows 10 and 11), 3 d_a = 65504. lossy: token 0 takes subnormals whose product with scale(0..2)
    is no fp32 number (lossy_scale_slack), otherwise ones for which it is. The largest term is 65504 * 2^72 * 49152 <
    2^104: no Inf, no NaN."""
    assert n >= EXTREME_ROWS and k % 32 == 0
    nb = k // 32
    bq = random_mxfp4(rng, n, k)
    for r, e in enumerate(EXTREME_E):
        bq[r, :, 0] = e
    bq[8, :, 1:] = 0x00
    bq[9, :, 1:] = 0x88
    bq[10, :, 1:] = 0x77
    bq[11, :, 1:] = 0xFF
    bq[12, :, 0] = 160 + (np.arange(nb) * 40 // max(nb - 1, 1))
    aq = random_q8_1(rng, 4, k)
    j = np.arange(nb)
    sub = np.array(F16_SUBNORMALS_LOSSY if lossy else F16_SUBNORMALS_EXACT)
    aq[0, :, 0:2] = _f16_bytes(sub[j % len(sub)])
    aq[1, :, 0:2] = _f16_bytes(np.full(nb, F16_MIN_NORMAL))
    aq[2, :, 0:2] = _f16_bytes(np.ones(nb))
    aq[2, 0, 4:36] = 0x80
    aq[3, :, 0:2] = _f16_bytes(np.full(nb, F16_MAX))
    return aq, bq


W_OFFSETS = (0, 1, 2, 3)  # every position of a block in a dword
A_OFFSETS = (0, 4)        # activations: 16-B aligned, and 4 B past it
SWEEP_M = (1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 31, 33, 64)
# the first seed from 390 whose 16 cases hold every weight offset, both activation offsets and 5 cases on each side
FUZZ_SEED = 391


def fuzz_cases(n_cases: int = 16, seed: int = FUZZ_SEED):
    """(i, m, n, k, weight byte offset, activation byte offset): the seeded MXFP4 sweep of tests/test_gpu_mxfp4.py. M on
    both sides of the GEMV / MFMA threshold, N in 1..200, K = 32 * (1..96), every weight offset."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_cases):
        m = int(rng.choice(SWEEP_M))
        n = int(rng.integers(1, 201))
        k = 32 * int(rng.integers(1, 97))
        out.append((i, m, n, k, int(rng.choice(W_OFFSETS)), int(rng.choice(A_OFFSETS))))
    return out


def quantize(x: np.ndarray) -> np.ndarray:
    """A simple test-side MXFP4 quantizer (for NMSE only; not ggml's): float [N, K] -> uint8 [N, K/32, 17]. Per block
    e = 128 + ceil(log2(amax / 12)) (the smallest scale under which amax fits the table; 0 for an all-zero block), each
    element the nearest table value of x / scale(e), ties to the smaller index."""
    x = np.asarray(x, np.float64)
    n, k = x.shape
    xs = x.reshape(n, k // 32, 32)
    amax = np.abs(xs).max(-1)
    with np.errstate(divide="ignore"):
        e = np.where(amax > 0, 128 + np.ceil(np.log2(np.maximum(amax, 1e-300) / 12.0)), 0)
    e = np.clip(e, 0, 255).astype(np.uint8)
    v = xs / scale(e).astype(np.float64)[..., None]
    code = np.abs(v[..., None] - KV[None, None, None, :]).argmin(-1)
    return build(e, code)
