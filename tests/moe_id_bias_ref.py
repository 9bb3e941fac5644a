"""Shared by tests/test_moe_id_bias_cpu.py, tests/test_gpu_moe_prefill_bias.py and tests/test_gpu_moe_batch_bias.py: the
model of qg_gemm_w4a8_moe_prefill_bias / qg_gemm_w4a8_moe_batch_bias. Imports without torch.

The entries compute, per slot s = t * n_used + u with e = ids[t, u],
    C[s, n] = product(B[e][n], A[t * a_rows + u % a_rows]) + bias[e, n]
the addition one rounded fp32 operation on the finished product, absent where bias is None, and +0.0f for an id outside
[0, n_expert). `add_bias` is that addition in NumPy float32 on products that come from elsewhere (the library's eager
call, the old entry, the host twin); `mxfp4_chain_f32` is the MXFP4 product itself as the host twin and the decode GEMV
order it: one fp32 accumulator per output, blocks in order, (d_a * scale(e)) * float(sumi) per block.

The bound of a biased MFMA output against the float64 model c64 + bias: the product's own bound, tol(mag, K, W) of the
type's tests (W = 8 for mxfp4_mmq: an output is the sum of at most 8 K-slice partials), plus 2^-24 |c64 + bias| for the
one rounded addition: half an ulp at the sum's magnitude (the product's bound is itself twice the fp32 bound, which
covers the second-order term 2^-24 times the product's error). Derived from the formats, not fitted to the kernels.
"""
import numpy as np

import kquant_ref as KR
import moe_ref as MR
import mxfp4_ref as XR

Q4_K, Q6_K, MXFP4 = MR.Q4_K, MR.Q6_K, 39
TYPES = (MXFP4, Q4_K, Q6_K)
BB = dict(MR.BB)
BB[MXFP4] = XR.BYTES
MXFP4_REC_BYTES = 48            # LDS bytes per (gathered row, block) of the MXFP4 decode GEMV
MAX_LDS_BYTES = 160 * 1024
MMQ_W = {MXFP4: XR.MMQ_W, Q4_K: 16, Q6_K: 8}   # the MFMA families' extra partial sums per output


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def be(t):
    return 256 if t in (Q4_K, Q6_K) else 32


def expert_bytes(t, n, k):
    return n * (k // be(t)) * BB[t]


def ref_mod(t):
    """The NumPy contract of a type: gemm(aq, bq) -> (c64, sumi, mag) and tol(mag, k, w)."""
    return XR if t == MXFP4 else KR if t == Q4_K else MR.QR


def random_experts(rng, t, n_expert, n, k):
    """uint8 [n_expert, n, blocks, block bytes], every expert different."""
    if t == MXFP4:
        return XR.random_mxfp4(rng, n_expert * n, k).reshape(n_expert, n, k // 32, XR.BYTES)
    return MR.random_experts(rng, t, n_expert, n, k)


def random_bias(rng, n_expert, n, stride, guard=True):
    """float32 [n_expert + 2, stride]: the experts' rows are 1 .. n_expert; rows 0 and n_expert + 1 and the columns from
    n on hold NaN, so an id clamped into the buffer or a wrong stride shows as NaN. Values of the order of the random
    experts' products (10^2 .. 10^4), both signs."""
    assert stride > n
    b = rng.uniform(-3000.0, 3000.0, (n_expert + 2, stride)).astype(np.float32)
    if guard:
        b[0], b[-1], b[:, n:] = np.nan, np.nan, np.nan
    return b


def add_bias(p, bias, ids, n_expert):
    """p float32 [T, n_used, N], bias float32 [n_expert, >= N] or None, ids int [T, >= n_used] -> float32(p + bias[e])
    for the slots whose id is in range, +0.0f rows for the others (p's are zeros there already). None: p itself."""
    p = np.ascontiguousarray(p, np.float32)
    if bias is None:
        return p
    T, n_used, N = p.shape
    out = p.copy()
    for t in range(T):
        for u in range(n_used):
            e = int(ids[t, u])
            if 0 <= e < n_expert:
                out[t, u] = p[t, u] + np.asarray(bias[e, :N], np.float32)
    assert out.dtype == np.float32
    return out


def mxfp4_chain_f32(aq, bq):
    """float32 [M, N]: sum over blocks in order of (d_a * scale(e)) * float(sumi), every operation rounded to fp32."""
    da, _, _ = XR.q8_1_fields(aq)
    _, sumi = XR._terms(aq, bq)
    ds = da.astype(np.float32)[:, None, :] * XR.scale(bq[..., 0]).astype(np.float32)[None]
    assert ds.dtype == np.float32
    acc = np.zeros(sumi.shape[:2], np.float32)
    for b in range(sumi.shape[2]):
        acc = acc + ds[:, :, b] * sumi[:, :, b].astype(np.float32)
    assert acc.dtype == np.float32
    return acc


def moe_chain_f32(aq_rows, experts, bias, ids, n_used, a_rows):
    """The MXFP4 model of a whole call: aq_rows [T * a_rows, K/32, 36], experts [n_expert, N, K/32, 17], bias
    [n_expert, >= N] or None, ids [T, >= n_used] -> float32 [T, n_used, N]."""
    n_expert, N = experts.shape[:2]
    T = ids.shape[0]
    p = np.zeros((T, n_used, N), np.float32)
    for t in range(T):
        for u in range(n_used):
            e = int(ids[t, u])
            if 0 <= e < n_expert:
                p[t, u] = mxfp4_chain_f32(aq_rows[t * a_rows + u % a_rows][None], experts[e])[0]
    return add_bias(p, bias, ids, n_expert)


def biased_tol(t, c64, mag, bias_row, k):
    """(reference float64, bound) of one expert's biased MFMA outputs: c64, mag [rows, N] of the type's gemm model,
    bias_row float32 [N] or None."""
    tol = ref_mod(t).tol(mag, k, MMQ_W[t])
    if bias_row is None:
        return c64, tol
    ref = c64 + np.asarray(bias_row, np.float32).astype(np.float64)[None]
    return ref, tol + 2.0 ** -24 * np.abs(ref)


# ---- the launch forms -------------------------------------------------------------------------------------------------
def mxfp4_form(k):
    """(LPR, WGS, ONE) of the MXFP4 decode GEMV for K (kq_gemv_form_units(K / 32)): the ladder qg_moe_config names."""
    units = k // 32
    lpr, wgs = (64, 1024) if units >= 64 else (16, 512) if units >= 16 else (4, 256)
    return lpr, wgs, int(units <= lpr)


def batch_rows(slots, n_expert, k, t=MXFP4):
    """R of the batch entry: per = ceil(slots / n_expert) -> 2 / 4 / 8, halved until R rows' records fit 160 KiB; 0: none."""
    per = -(-slots // n_expert)
    r = 2 if per <= 2 else 4 if per <= 4 else 8
    row = k // 32 * MXFP4_REC_BYTES if t == MXFP4 else k // 256 * MR.KQ_REC_BYTES[t]
    while r >= 2 and r * row > MAX_LDS_BYTES:
        r //= 2
    return r if r >= 2 else 0


def max_tiles(slots, n_expert, r):
    return slots // r + min(n_expert + 1, slots)


def prefill_form_rg1(slots, n_expert):
    """(TT, RG) of the prefill's general rule where it does not depend on the device: per <= 16 -> (1, 1), per <= 32 ->
    (2, 1); beyond that TT = 4 and RG is 1 or 4 by the CU count (None)."""
    per = -(-slots // n_expert)
    return (1, 1) if per <= 16 else (2, 1) if per <= 32 else (4, None)
