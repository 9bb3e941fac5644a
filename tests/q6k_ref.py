"""NumPy model of ggml's Q6_K format and of the Q6_K x Q8_1 product contract (include/qg/qg.h, "Q6_K weights"),
written from the format description and independent of the library.

block_q6_K, 210 bytes, 256 elements: ql[128] (low 4 bits of the codes), qh[64] (high 2 bits), scales[16] (int8, one
per 16 elements), f16 d. For element e: h = e / 128, p = e % 128, c = p / 32, l = p % 32;
    lo = (ql[64h + 32(c & 1) + l] >> (4 (c >> 1))) & 15,  hi = (qh[32h + l] >> (2c)) & 3,  q = (lo | hi << 4) - 32,
    value = d * scales[8h + 2c + l / 16] * q.
Q8_1 block b of super-block sb is activation block 8 sb + b and meets the scale groups 2b and 2b + 1:
    isum = scales[2b] * s0 + scales[2b + 1] * s1 (int32),  C = sum_sb d * sum_b d_a * float(isum).
"""
from __future__ import annotations

import numpy as np

# shared with the Q4_K reference; re-exported: the tests take them from either module
from kquant_ref import F16_MAX, F16_MIN_NORMAL, F16_SUBNORMALS, _f16_bytes, dev_at, tol  # noqa: F401

QK_K = 256
BYTES = 210
Q6_K = 14


def _index_maps():
    e = np.arange(QK_K)
    h, p = e // 128, e % 128
    c, l = p // 32, p % 32
    return 64 * h + 32 * (c & 1) + l, 4 * (c >> 1), 32 * h + l, 2 * c, 8 * h + 2 * c + l // 16


_QL_IDX, _QL_SH, _QH_IDX, _QH_SH, _GROUP = _index_maps()


def fields(b: np.ndarray):
    """b: uint8 [..., 210] -> d (float32 [...]), sc (int32 [..., 16]), q (int32 [..., 256], the signed codes -32..31)."""
    b = np.ascontiguousarray(b, np.uint8)
    assert b.shape[-1] == BYTES
    ql, qh = b[..., 0:128].astype(np.int32), b[..., 128:192].astype(np.int32)
    sc = b[..., 192:208].view(np.int8).astype(np.int32)
    d = b[..., 208:210].copy().view(np.float16)[..., 0].astype(np.float32)
    lo = (ql[..., _QL_IDX] >> _QL_SH) & 15
    hi = (qh[..., _QH_IDX] >> _QH_SH) & 3
    return d, sc, (lo | (hi << 4)) - 32


def build(d, sc, q) -> np.ndarray:
    """The inverse of fields(): d [...], sc [..., 16] in -128..127, q [..., 256] in -32..31 -> uint8 [..., 210]."""
    d = np.asarray(d)
    u = (np.asarray(q, np.int32) + 32).astype(np.uint8)
    assert (u < 64).all()
    b = np.zeros(d.shape + (BYTES,), np.uint8)
    for e in range(QK_K):
        b[..., _QL_IDX[e]] |= ((u[..., e] & 15) << np.uint8(_QL_SH[e])).astype(np.uint8)
        b[..., 128 + _QH_IDX[e]] |= ((u[..., e] >> 4) << np.uint8(_QH_SH[e])).astype(np.uint8)
    b[..., 192:208] = np.asarray(sc, np.int8).view(np.uint8)
    b[..., 208:210] = _f16_bytes(d)
    return b


def dequant(b: np.ndarray) -> np.ndarray:
    """float32 [..., 256 * super-blocks] = (d * float(scale)) * float(q), each product rounded to fp32, in that order."""
    d, sc, q = fields(b)
    ds = (d[..., None] * sc.astype(np.float32)).astype(np.float32)
    y = (ds[..., _GROUP] * q.astype(np.float32)).astype(np.float32)
    return y.reshape(b.shape[:-2] + (-1,))


def q8_1_fields(aq: np.ndarray):
    """aq: uint8 [M, K/32, 36] -> d_a (float64 [M, K/32]), qs (int32 [M, K/32, 32]). s_a is not part of the contract."""
    aq = np.ascontiguousarray(aq, np.uint8)
    da = aq[..., 0:2].copy().view(np.float16)[..., 0].astype(np.float64)
    return da, aq[..., 4:36].view(np.int8).astype(np.int32)


def gemm(aq: np.ndarray, bq: np.ndarray):
    """aq [M, K/32, 36] Q8_1, bq [N, K/256, 210] Q6_K -> (C float64 [M, N], isum int32 [M, N, K/32], mag float64
    [M, N] = sum |d d_a isum|)."""
    d, sc, q = fields(bq)
    n, nsb = d.shape
    da, qa = q8_1_fields(aq)
    mm, nb = da.shape
    assert nb == 8 * nsb
    # per 16-element group g a [M, 16] x [16, N] product; float64 holds these integers exactly
    qg_ = q.reshape(n, 2 * nb, 16).transpose(1, 2, 0).astype(np.float64)
    ag = qa.reshape(mm, 2 * nb, 16).transpose(1, 0, 2).astype(np.float64)
    s = np.matmul(ag, qg_)  # [2 nb, M, N]
    scg = sc.reshape(n, 2 * nb).T.astype(np.float64)  # [2 nb, N]
    part = s * scg[:, None, :]
    isum = (part[0::2] + part[1::2]).transpose(1, 2, 0)  # [M, N, nb]
    assert np.abs(isum).max(initial=0) <= 2 ** 24
    isum = np.ascontiguousarray(isum).astype(np.int32)
    dn = np.repeat(d.astype(np.float64), 8, axis=1)  # [N, nb]
    t = dn[None] * da[:, None, :] * isum
    return t.sum(-1), isum, np.abs(t).sum(-1)


def random_q6k(rng, n: int, k: int) -> np.ndarray:
    """[n, k/256, 210]: every ql / qh / scales byte uniform in 0..255, d in +-0.01 (f16, both signs)."""
    b = rng.integers(0, 256, (n, k // QK_K, BYTES), dtype=np.uint8)
    b[..., 208:210] = _f16_bytes(rng.uniform(-0.01, 0.01, (n, k // QK_K)))
    return b


def random_q8_1(rng, m: int, k: int) -> np.ndarray:
    """[m, k/32, 36]: qs uniform in -128..127, d_a in (0, 0.05], s_a arbitrary finite (unused by Q6_K)."""
    a = rng.integers(0, 256, (m, k // 32, 36), dtype=np.uint8)
    a[..., 0:2] = _f16_bytes(rng.uniform(1e-3, 0.05, (m, k // 32)))
    a[..., 2:4] = _f16_bytes(rng.uniform(-4.0, 4.0, (m, k // 32)))
    return a


# f16 scale values at the ends of the format
EXTREME_ROWS = 12


def extremes(rng, m: int, n: int = 16, k: int = 512):
    """Q8_1 [m, k/32, 36] and Q6_K [n, k/256, 210] at the ends of their formats, one class per weight row (an output's
    tolerance follows its own magnitude). No Inf, no NaN: the largest term is 65504 * 65504 * 2^24 = 7.2e16.

    Weight rows: 0, 1 d f16 subnormals of both signs; 2 the smallest normal; 3, 4 d = +65504 / -65504; 5 every scale
    -128; 6 every scale 127; 7 every scale 0; 8 every code 0 (q = -32); 9 every code 63 (q = 31); 10 d = 65504,
    scales -128, codes 0 (the largest |isum| against qs = -128 ... : 2 * 128 * 16 * 32 * 128 = 2^24); 11 scales
    alternating 127 / -128 with codes 63 (the two halves of a block cancel almost exactly). Further rows are random.
    Activation token 0: every d_a an f16 subnormal; token 1: d_a = 65504 and qs = -128; token 2 (if any): d_a the
    smallest normal, qs = 127. Further tokens are random."""
    assert m >= 2 and n >= EXTREME_ROWS and k % QK_K == 0
    nsb = k // QK_K
    bq = random_q6k(rng, n, k)
    d, sc, q = fields(bq)
    sub = np.array(F16_SUBNORMALS)
    alt = np.where(np.arange(nsb) % 2 == 0, 1.0, -1.0)
    d[0] = sub[np.arange(nsb) % 5] * alt
    d[1] = -sub[(np.arange(nsb) + 2) % 5] * alt
    d[2] = F16_MIN_NORMAL * alt
    d[3], d[4] = F16_MAX, -F16_MAX
    sc[5], sc[6], sc[7] = -128, 127, 0
    q[8], q[9] = -32, 31
    d[10], sc[10], q[10] = F16_MAX, -128, -32
    sc[11] = np.where(np.arange(16) % 2 == 0, 127, -128)
    q[11] = 31
    bq = build(d, sc, q)

    aq = random_q8_1(rng, m, k)
    nb = k // 32
    j = np.arange(nb)
    aq[0, :, 0:2] = _f16_bytes(sub[j % 5])
    aq[1, :, 0:2] = _f16_bytes(np.full(nb, F16_MAX))
    aq[1, :, 4:36] = 0x80  # qs = -128
    if m > 2:
        aq[2, :, 0:2] = _f16_bytes(np.full(nb, F16_MIN_NORMAL))
        aq[2, :, 4:36] = 127
    return aq, bq


W_OFFSETS = (2, 18)       # 2 mod 4 (every super-block's parity flipped), 2 mod 16
A_OFFSETS = (4, 8, 12)    # 4, 8, 12 mod 16
SWEEP_M = (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 64)  # the product sweep's list (tests/test_gpu_q6k.py)


def fuzz_cases(n_cases: int = 16, seed: int = 614):
    """(i, m, n, k, weight byte offset, activation byte offset): the seeded Q6_K sweep of tests/test_gpu_q6k.py. M from
    the product sweep's list, N in 1..200, K = 256 * (1..12), the offsets from the pointer contract's classes."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_cases):
        m = int(rng.choice(SWEEP_M))
        n = int(rng.integers(1, 201))
        k = 256 * int(rng.integers(1, 13))
        out.append((i, m, n, k, int(rng.choice(W_OFFSETS)), int(rng.choice(A_OFFSETS))))
    return out


PATH_SWEEP_M = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 17, 24, 31, 32, 33, 48, 64, 65, 96)
# the first seed from 600 whose 24 cases hold every M of 1..8 and MFMA cases at K > 2048 for each of TT = 1, 2, 4
# (tests/test_q6k_cpu.py::test_path_fuzz_cases_are_seeded_and_reach_the_loops pins what the sweep needs of it)
PATH_SWEEP_SEED = 677


def path_fuzz_cases(n_cases: int = 24, seed: int = PATH_SWEEP_SEED):
    """(i, m, n, k, weight byte offset, activation byte offset): the seeded sweep of tests/test_gpu_q6k_paths.py. Every
    M tile and token-tile form, N in 1..300, K = 256 * (1..20): past 2048 the MFMA kernel's eight K slices take a
    second pass (the prefetch and reload loop)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_cases):
        m = int(rng.choice(PATH_SWEEP_M))
        n = int(rng.integers(1, 301))
        k = 256 * int(rng.integers(1, 21))
        out.append((i, m, n, k, int(rng.choice(W_OFFSETS)), int(rng.choice(A_OFFSETS))))
    return out


def quantize(x: np.ndarray) -> np.ndarray:
    """A simple test-side min/max Q6_K quantizer (for NMSE only; not ggml's): float [N, K] -> uint8 [N, K/256, 210].
    Per 16-element group scale = max|x| / 31; d = f16(max scale / 127); sc = rint(scale / d);
    q = clip(rint(x / (d sc)), -32, 31); zero wherever a divisor is 0."""
    x = np.asarray(x, np.float64)
    n, k = x.shape
    xs = x.reshape(n, k // QK_K, 16, 16)
    scale = np.abs(xs).max(-1) / 31.0
    d = (scale.max(-1) / 127.0).astype(np.float16)
    d64 = d.astype(np.float64)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = np.clip(np.where(d64 != 0, np.rint(scale / d64), 0.0), -128, 127)
        div = (d64 * sc)[..., None]
        q = np.clip(np.where(div != 0, np.rint(xs / div), 0.0), -32, 31)
    return build(d, sc.astype(np.int8), q.reshape(n, k // QK_K, 256).astype(np.int32))
