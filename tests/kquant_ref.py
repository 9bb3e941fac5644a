"""NumPy model of ggml's Q4_K format and of the Q4_K x Q8_1 product contract (include/qg/qg.h, "Q4_K
weights"), written from the format description and independent of the library.

block_q4_K, 144 bytes, 256 elements: f16 d, f16 dmin, scales[12] (eight 6-bit scales sc and eight 6-bit mins
m), qs[128]; chunk i = 0..3 of qs holds sub-block 2i in the low and sub-block 2i + 1 in the high nibbles.
Element e of sub-block j is d * sc[j] * q_e - dmin * m[j]; sub-block j of super-block sb meets Q8_1 block
8 sb + j.
"""
from __future__ import annotations

import numpy as np

QK_K = 256
BYTES = 144


def pack_scales(sc: np.ndarray, m: np.ndarray) -> np.ndarray:
    """sc, m: [..., 8] integers in 0..63 -> scales [..., 12] uint8."""
    sc, m = np.asarray(sc, np.uint8), np.asarray(m, np.uint8)
    q = np.zeros(sc.shape[:-1] + (12,), np.uint8)
    for j in range(4):
        q[..., j] = (sc[..., j] & 63) | ((sc[..., j + 4] >> 4) << 6)
        q[..., j + 4] = (m[..., j] & 63) | ((m[..., j + 4] >> 4) << 6)
        q[..., j + 8] = (sc[..., j + 4] & 15) | ((m[..., j + 4] & 15) << 4)
    return q


def unpack_scales(q: np.ndarray):
    """scales [..., 12] uint8 -> (sc, m), each [..., 8] int32."""
    q = np.asarray(q, np.uint8).astype(np.int32)
    sc = np.zeros(q.shape[:-1] + (8,), np.int32)
    m = np.zeros_like(sc)
    for j in range(4):
        sc[..., j] = q[..., j] & 63
        m[..., j] = q[..., j + 4] & 63
    for j in range(4, 8):
        sc[..., j] = (q[..., j + 4] & 15) | ((q[..., j - 4] >> 6) << 4)
        m[..., j] = (q[..., j + 4] >> 4) | ((q[..., j] >> 6) << 4)
    return sc, m


def fields(b: np.ndarray):
    """b: uint8 [..., 144] -> d, dmin (float32 [...]), sc, m (int32 [..., 8]), q (int32 [..., 8, 32])."""
    b = np.ascontiguousarray(b, np.uint8)
    assert b.shape[-1] == BYTES
    d = b[..., 0:2].copy().view(np.float16)[..., 0].astype(np.float32)
    dmin = b[..., 2:4].copy().view(np.float16)[..., 0].astype(np.float32)
    sc, m = unpack_scales(b[..., 4:16])
    qs = b[..., 16:144].astype(np.int32).reshape(b.shape[:-1] + (4, 32))
    q = np.stack([qs & 15, qs >> 4], axis=-2).reshape(b.shape[:-1] + (8, 32))  # [.., chunk, (lo, hi), 32]
    return d, dmin, sc, m, q


def dequant(b: np.ndarray) -> np.ndarray:
    """float32 [..., 256 * super-blocks] = (d * sc) * q - dmin * m, each operation rounded to fp32 in that order."""
    d, dmin, sc, m, q = fields(b)
    ds = (d[..., None] * sc.astype(np.float32)).astype(np.float32)
    dm = (dmin[..., None] * m.astype(np.float32)).astype(np.float32)
    y = ((ds[..., None] * q.astype(np.float32)).astype(np.float32) - dm[..., None]).astype(np.float32)
    return y.reshape(b.shape[:-2] + (-1,))


def q8_1_fields(aq: np.ndarray):
    """aq: uint8 [M, K/32, 36] -> d_a, s_a (float64 [M, K/32]), qs (int32 [M, K/32, 32])."""
    aq = np.ascontiguousarray(aq, np.uint8)
    da = aq[..., 0:2].copy().view(np.float16)[..., 0].astype(np.float64)
    sa = aq[..., 2:4].copy().view(np.float16)[..., 0].astype(np.float64)
    return da, sa, aq[..., 4:36].view(np.int8).astype(np.int32)


def gemm(aq: np.ndarray, bq: np.ndarray):
    """aq [M, K/32, 36] Q8_1, bq [N, K/256, 144] Q4_K -> (C float64 [M, N], sumi int32 [M, N, K/32], mag float64
    [M, N] = sum(|d sc d_a sumi| + |dmin m s_a|))."""
    d, dmin, sc, m, q = fields(bq)
    n, nsb = d.shape
    da, sa, qa = q8_1_fields(aq)
    mm, nb = da.shape
    assert nb == 8 * nsb
    qw = q.reshape(n, nb, 32)
    # per block b a [M, 32] x [32, N] product; float64 holds these integers (< 2^53) exactly
    s = np.matmul(qa.transpose(1, 0, 2).astype(np.float64), qw.transpose(1, 2, 0).astype(np.float64))
    sumi = np.ascontiguousarray(s.transpose(1, 2, 0)).astype(np.int32)
    dsc = (d.astype(np.float64)[..., None] * sc).reshape(n, nb)
    dm = (dmin.astype(np.float64)[..., None] * m).reshape(n, nb)
    t1 = dsc[None] * da[:, None, :] * sumi
    t2 = dm[None] * sa[:, None, :]
    return (t1 - t2).sum(-1), sumi, (np.abs(t1) + np.abs(t2)).sum(-1)


def tol(mag: np.ndarray, k: int, w: int) -> np.ndarray:
    """|c - C64| bound of the contract: 2 (K/32 + w + 2) 2^-24 mag, twice the fp32 bound for K/32 + w terms. w = the
    extra partial sums the kernel's reduction chains per output: 0 for q4k_gemv, q6k_gemv and the host twin (lane-serial /
    one chain of K/32 terms), 16 for q4k_mmq, 8 for q6k_mmq (an output is the sum of at most 8 K-slice partials)."""
    return 2.0 * (k // 32 + w + 2) * 2.0 ** -24 * mag + 1e-30


def _f16_bytes(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x)
    return np.ascontiguousarray(x.astype(np.float16)).view(np.uint8).reshape(x.shape + (2,))


def random_q4k(rng, n: int, k: int) -> np.ndarray:
    """[n, k/256, 144]: every scales and qs byte uniform in 0..255, d in +-0.01, dmin in +-0.05 (f16, both signs)."""
    b = rng.integers(0, 256, (n, k // QK_K, BYTES), dtype=np.uint8)
    b[..., 0:2] = _f16_bytes(rng.uniform(-0.01, 0.01, (n, k // QK_K)))
    b[..., 2:4] = _f16_bytes(rng.uniform(-0.05, 0.05, (n, k // QK_K)))
    return b


def random_q8_1(rng, m: int, k: int) -> np.ndarray:
    from test_gpu_product import random_blocks
    return random_blocks(rng, m, 1, k, 2)[0]


def build(d, dmin, sc, m, q) -> np.ndarray:
    """The inverse of fields(): d, dmin [...], sc, m [..., 8], q [..., 8, 32] in 0..15 -> uint8 [..., 144]."""
    d = np.asarray(d)
    b = np.zeros(d.shape + (BYTES,), np.uint8)
    b[..., 0:2] = _f16_bytes(d)
    b[..., 2:4] = _f16_bytes(np.asarray(dmin))
    b[..., 4:16] = pack_scales(sc, m)
    q = np.asarray(q, np.uint8).reshape(d.shape + (4, 2, 32))
    b[..., 16:144] = (q[..., 0, :] | (q[..., 1, :] << 4)).reshape(d.shape + (128,))
    return b


# f16 scale values at the ends of the format: subnormals (2^-24 .. 1023 * 2^-24, 2^-15 among them), the smallest
# normal (2^-14) and the largest finite value (65504)
F16_SUBNORMALS = (2.0 ** -24, 3 * 2.0 ** -24, 2.0 ** -20, 2.0 ** -15, 1023 * 2.0 ** -24)
F16_MIN_NORMAL = 2.0 ** -14
F16_MAX = 65504.0
EXTREME_ROWS = 16  # weight rows extremes() gives a class of their own; the rest are random_q4k rows


def extremes(rng, m: int, n: int = 32, k: int = 512):
    """Q8_1 [m, k/32, 36] and Q4_K [n, k/256, 144] at the ends of their scale formats, one class per weight row
    (an output's tolerance follows its own magnitude, so no row's extreme hides another's). No Inf, no NaN; the
    largest term, 65504 * 63 * 65504 * (15 * 127 * 32) = 1.6e16, is far inside fp32.

    Weight rows: 0..3 d and dmin f16 subnormals of both signs; 4 the smallest normal; 5 d = dmin = 65504 with every
    sc = m = 63 and every nibble 15; 6..8 the other sign pairs of +-65504; 9 sc = 0, m = 63; 10 sc = 63, m = 0;
    11..14 sub-blocks 4..7 (whose sc and m keep their high two bits in another byte) at 16 / 32 / 48 / 63 in four
    rotations, sub-blocks 0..3 at zero (11) or at the complement (12..14); 15 sc = m = 48 in sub-blocks 4..7 and 16 in
    0..3.
    Activation token 0: every d_a and s_a an f16 subnormal. Token 1: super-block 0 meets subnormal d_a with
    s_a = -65504 .. -36832, the others d_a = 65504, qs = +127, s_a = -65504. Further tokens are random."""
    assert m >= 2 and n >= EXTREME_ROWS and k % QK_K == 0
    nsb = k // QK_K
    bq = random_q4k(rng, n, k)
    d, dmin, sc, mn, q = fields(bq)
    sub = np.array(F16_SUBNORMALS)
    alt = np.where(np.arange(nsb) % 2 == 0, 1.0, -1.0)  # the sign alternates along the super-blocks
    for r in range(4):
        d[r] = sub[(r + np.arange(nsb)) % 5] * alt * (1 if r % 2 == 0 else -1)
        dmin[r] = sub[(2 * r + 1 + np.arange(nsb)) % 5] * alt * (1 if r < 2 else -1)
    d[4], dmin[4] = F16_MIN_NORMAL * alt, -F16_MIN_NORMAL * alt
    for r, (sd, sm) in zip(range(5, 9), ((1, 1), (-1, -1), (1, -1), (-1, 1))):
        d[r], dmin[r] = sd * F16_MAX, sm * F16_MAX
    sc[5], mn[5], q[5] = 63, 63, 15
    sc[9], mn[9] = 0, 63
    sc[10], mn[10] = 63, 0
    hi = np.array([16, 32, 48, 63])
    for i, r in enumerate(range(11, 15)):
        sc[r, :, 4:], mn[r, :, 4:] = np.roll(hi, i), np.roll(hi[::-1], i)
        sc[r, :, :4], mn[r, :, :4] = (0, 0) if i == 0 else (63 - sc[r, :, 4:], 63 - mn[r, :, 4:])
    sc[15, :, 4:], mn[15, :, 4:], sc[15, :, :4], mn[15, :, :4] = 48, 48, 16, 16
    bq = build(d, dmin, sc, mn, q)

    aq = random_q8_1(rng, m, k)
    nb = k // 32
    j = np.arange(nb)
    aq[0, :, 0:2] = _f16_bytes(sub[j % 5])
    aq[0, :, 2:4] = _f16_bytes(sub[(j + 2) % 5] * np.where(j % 3 == 0, -1.0, 1.0))
    aq[1, :, 0:2] = _f16_bytes(np.where(j < 8, sub[j % 5], F16_MAX))
    aq[1, :, 2:4] = _f16_bytes(np.where(j < 8, -F16_MAX + 4096.0 * j, -F16_MAX))
    aq[1, 8:, 4:36] = 127
    return aq, bq


W_OFFSETS = (16, 32, 48, 144)  # 16 mod 32, 32 mod 64, 48 mod 64, one whole super-block
A_OFFSETS = (4, 8, 12, 36)     # 4 mod 16, 8 mod 16, 12 mod 16, one whole Q8_1 block


def fuzz_cases(n_cases: int = 24, seed: int = 412):
    """(i, m, n, k, weight byte offset, activation byte offset): the seeded Q4_K sweep of tests/test_gpu_q4k_paths.py.
    M from the product sweep's list (tests/test_gpu_fuzz.py), N in 1..300, K = 256 * (1..20), the offsets from
    the pointer contract's classes (weights 16 B, activations 4 B)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n_cases):
        m = int(rng.choice([1, 2, 3, 4, 5, 7, 8, 9, 12, 16, 17, 24, 31, 32, 33, 48, 64, 65, 96]))
        n = int(rng.integers(1, 301))
        k = 256 * int(rng.integers(1, 21))
        out.append((i, m, n, k, int(rng.choice(W_OFFSETS)), int(rng.choice(A_OFFSETS))))
    return out


def dev_at(x: np.ndarray, offset: int, fill: int = 0):
    """x on the GPU as a contiguous slice of one flat uint8 buffer, starting `offset` bytes past a 256-B boundary; every
    other byte of the buffer (at least 256 after x, `offset` or more before it) is `fill`."""
    import torch
    x = np.ascontiguousarray(x)
    flat = torch.full((x.nbytes + 512 + offset,), fill, dtype=torch.uint8, device="cuda")
    start = (-flat.data_ptr()) % 256 + offset
    t = flat[start:start + x.nbytes]
    t.copy_(torch.from_numpy(x.view(np.uint8).reshape(-1)))
    assert (t.data_ptr() - offset) % 256 == 0 and t.is_contiguous()
    return t.reshape(x.shape)


def quantize(x: np.ndarray) -> np.ndarray:
    """A simple test-side Q4_K quantizer (for NMSE only; not ggml's): float [N, K] -> uint8 [N, K/256, 144].
    Per sub-block lo = min(0, min x), scale = (max(0, max x) - lo) / 15, mval = -lo; d = f16(max scale / 63),
    dmin = f16(max mval / 63); sc = rint(scale / d), m = rint(mval / dmin);
    q = clip(rint((x + dmin m) / (d sc)), 0, 15); zero wherever a divisor is 0."""
    x = np.asarray(x, np.float64)
    n, k = x.shape
    xs = x.reshape(n, k // QK_K, 8, 32)
    lo = np.minimum(0.0, xs.min(-1))
    scale = (np.maximum(0.0, xs.max(-1)) - lo) / 15.0
    mval = -lo
    d = (scale.max(-1) / 63.0).astype(np.float16)
    dmin = (mval.max(-1) / 63.0).astype(np.float16)
    d64, dmin64 = d.astype(np.float64)[..., None], dmin.astype(np.float64)[..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = np.where(d64 != 0, np.rint(scale / d64), 0.0)
        m = np.where(dmin64 != 0, np.rint(mval / dmin64), 0.0)
        sc, m = np.clip(sc, 0, 63), np.clip(m, 0, 63)
        div = (d64 * sc)[..., None]
        q = np.where(div != 0, np.rint((xs + (dmin64 * m)[..., None]) / div), 0.0)
    q = np.clip(q, 0, 15)
    return build(d, dmin, sc.astype(np.uint8), m.astype(np.uint8), q.astype(np.uint8))
