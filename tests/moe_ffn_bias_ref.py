"""Shared by tests/test_moe_ffn_bias_cpu.py and tests/test_gpu_moe_ffn_bias.py: the float32 model of
qg_gemm_w4a8_moe_glu_bias / qg_gemm_w4a8_moe_down_bias on top of the products of qg_gemm_w4a8_moe, gpt-oss's clamped
SwiGLU in float64 with its bound, and the launch form and LDS need of the MXFP4 down entry. Imports without torch.

The OAI bound. The entry computes, each step one rounded fp32 operation,
    x = fminf(g, limit); y = fminf(fmaxf(u, -limit), limit)          (exact: selections)
    p = alpha * (-x); e = expf(p); s = 1.0f + e; q = x / s; z = y + 1.0f; c = q * z
and the reference r = x / (1 + exp(alpha * -x)) * (y + 1) is evaluated in float64 from the float32 g, u, alpha, limit.
Relative errors, in ulps of 2^-23:
  * p is one rounded product, relative 2^-24. exp turns the absolute error |p| 2^-24 of its argument into the relative
    error |alpha x| 2^-24 of e: 0.5 |alpha x| ulp. This is the term swiglu_tol does not have (there p = -g is exact).
  * expf is within 1 ulp: 1.
  * both errors of e reach s = 1 + e scaled by e / (1 + e) <= 1; the addition itself rounds: 0.5.
  * the division is correctly rounded: 0.5.   * z = y + 1 rounds: 0.5.   * the final product rounds: 0.5.
Sum: 3 + 0.5 |alpha x| ulp, against swiglu_tol's 2.5. swiglu_tol allows 4 ulp for its 2.5, a margin factor of 1.6, and
that factor is kept: |c - r| <= 1.6 (3 + 0.5 |alpha x|) 2^-23 |r| + absolute term.
The absolute term restates swiglu_tol's 2^-120 (1 + |u|): once p > 88.72, expf overflows and the entry gives q = +-0
while the true |q| = |x| e^-p = (p / |alpha|) e^-p <= (88.73 / |alpha|) e^-88.72 < 2^-121 / min(1, |alpha|); |y + 1|
<= 1 + limit. So 2^-120 (1 + limit) / min(1, |alpha|), which also covers results below the normal range.
Nothing here is fitted to the kernel's error.
"""
import numpy as np

import kquant_ref as KR
import moe_glu_ref as GR
import moe_ref as MR
import mxfp4_ref as XR

REGLU, SWIGLU, SWIGLU_OAI = 0, 2, 3
MXFP4 = 39
MXFP4_REC_BYTES = 48        # LDS bytes per (activation row, block) of the MXFP4 decode GEMV (MXFP4_REC_DW * 4)
MAX_LDS_BYTES = 160 * 1024
OAI_MARGIN = 4.0 / 2.5      # swiglu_tol's 4 ulp over its derived 2.5


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def add_bias(p, bias, ids, n_expert):
    """p float32 [T, n_used, N] (the slots' products), bias float32 [n_expert, >= N] or None, ids int [T, >= n_used]
    -> p + bias[ids[t, u], :N] as np.float32 addition (one rounding) for the slots whose id is in range; the others
    are returned as they are. None: p itself (no add, -0.0f stays -0.0f)."""
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


def zero_bad(c, ids, n_expert):
    """The GLU entry's slots with an id out of range: +0.0f."""
    c = np.array(c, np.float32)
    T, n_used, _ = c.shape
    bad = ~((ids[:T, :n_used] >= 0) & (ids[:T, :n_used] < n_expert))
    c[bad] = 0.0
    return c


def glu_model(g, u, bias_gate, bias_up, ids, n_expert, op=REGLU):
    """The bits of qg_gemm_w4a8_moe_glu_bias for REGLU from the products g, u of qg_gemm_w4a8_moe; for the other ops the
    biased (g, u) to hand to the bounds. Returns (c or None, g + bg, u + bu)."""
    gb, ub = add_bias(g, bias_gate, ids, n_expert), add_bias(u, bias_up, ids, n_expert)
    c = zero_bad(GR.reglu(gb, ub), ids, n_expert) if op == REGLU else None
    return c, gb, ub


def swiglu_oai64(g, u, alpha, limit):
    """float64 from the float32 g, u, alpha, limit: x = min(g, limit), y = clip(u, -limit, limit),
    x / (1 + exp(alpha * -x)) * (y + 1) (exp overflows to inf for alpha * -x > 709: -0 * (y + 1))."""
    g, u = np.asarray(g, np.float32).astype(np.float64), np.asarray(u, np.float32).astype(np.float64)
    a, lim = float(np.float32(alpha)), float(np.float32(limit))
    x, y = np.minimum(g, lim), np.clip(u, -lim, lim)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(a * -x)) * (y + 1.0)


def oai_tol(r, g, alpha, limit):
    """The bound derived in the module docstring."""
    a, lim = float(np.float32(alpha)), float(np.float32(limit))
    x = np.minimum(np.asarray(g, np.float32).astype(np.float64), lim)
    ulps = OAI_MARGIN * (3.0 + 0.5 * np.abs(a * x))
    return ulps * 2.0 ** -23 * np.abs(r) + 2.0 ** -120 * (1.0 + lim) / min(1.0, abs(a))


def assert_oai(c, g, u, alpha, limit, what="", factor=1.0):
    """c float32 against factor times the bound (2 where both sides carry an expf); prints the largest err / bound of
    the plain bound. Returns it."""
    r = swiglu_oai64(g, u, alpha, limit)
    assert np.isfinite(r).all(), what
    err = np.abs(np.asarray(c, np.float32).astype(np.float64) - r)
    ratio = float((err / oai_tol(r, g, alpha, limit)).max()) if err.size else 0.0
    print(f"swiglu_oai {what} alpha={alpha} limit={limit}: max err / bound = {ratio:.4f}")
    assert np.isfinite(np.asarray(c)).all() and ratio <= factor, (what, ratio)
    return ratio


def oai_regions(g, u, limit):
    """Counts of the clamp regions among (g, u): g > limit, u > limit, u < -limit, and neither operand clamped."""
    g, u = np.asarray(g, np.float32), np.asarray(u, np.float32)
    lim = np.float32(limit)
    return {"g_hi": int((g > lim).sum()), "u_hi": int((u > lim).sum()), "u_lo": int((u < -lim).sum()),
            "free": int(((g <= lim) & (np.abs(u) <= lim)).sum())}


def assert_all_regions(g, u, limit, what=""):
    r = oai_regions(g, u, limit)
    assert all(v > 0 for v in r.values()), (what, r)
    return r


def small_experts(rng, t, n_expert, n, k):
    """uint8 [n_expert, n, blocks, block bytes] of MXFP4 / Q4_K / Q6_K like the random experts of moe_ref / mxfp4_ref,
    with the scale fields redrawn so that a product with random Q8_1 rows is of the order of 1 (theirs are 10^2 ..
    10^4): with biases of the order of the OAI limit, g and u then fall on both sides of every clamp."""
    if t == MXFP4:
        w = XR.random_mxfp4(rng, n_expert * n, k)
        w[..., 0] = rng.integers(116, 124, w.shape[:-1], dtype=np.uint8)
        return w.reshape(n_expert, n, k // 32, 17)
    w = MR.random_experts(rng, t, n_expert, n, k)
    fields = ((0, 2), (2, 4)) if t == MR.Q4_K else ((208, 210),)
    for lo, hi in fields:  # d (and dmin): f16
        w[..., lo:hi] = KR._f16_bytes(rng.uniform(-2e-4, 2e-4, w.shape[:-1]))
    return w


def mxfp4_form(k):
    """(LPR, WGS, ONE) of the MXFP4 decode GEMV for K (kq_gemv_form_units(K / 32)): the ladder qg_moe_config names."""
    units = k // 32
    lpr, wgs = (64, 1024) if units >= 64 else (16, 512) if units >= 16 else (4, 256)
    return lpr, wgs, int(units <= lpr)


def down_sw_rpb(n_used, lpr, wgs):
    """SW: the largest power of two <= min(n_used, WGS / 64); RPB = (WGS / 64 / SW) * (64 / LPR) (qg.h)."""
    w, sw = wgs // 64, 1
    while 2 * sw <= n_used and 2 * sw <= w:
        sw *= 2
    return sw, w // sw * (64 // lpr)


def mxfp4_down_lds(n_used, k):
    """n_used * (K/32 * MXFP4_REC_DW * 4 + 4 RPB): the records of the token's n_used rows and its n_used x RPB products."""
    lpr, wgs, _ = mxfp4_form(k)
    return n_used * (k // 32 * MXFP4_REC_BYTES + 4 * down_sw_rpb(n_used, lpr, wgs)[1])


def mxfp4_down_max_k(n_used):
    """The largest K (a multiple of 32) whose need fits 160 KiB; the need grows with K within a form and the forms'
    RPB terms are far below one block's record, so the first K that does not fit ends the search."""
    k = 32
    while mxfp4_down_lds(n_used, k + 32) <= MAX_LDS_BYTES:
        k += 32
    return k
