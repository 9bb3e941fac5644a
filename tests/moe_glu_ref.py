"""Shared by tests/test_moe_glu_cpu.py and tests/test_gpu_moe_glu.py: the two ops of qg_gemm_w4a8_moe_glu from the
float32 g and u of the two products, and the SwiGLU bound. Imports without torch."""
import numpy as np

REGLU, SWIGLU = 0, 2


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def reglu(g, u):
    """float32, the bits the entry must give: (g > 0 ? g : 0.0f) * u, one rounded multiplication."""
    g, u = np.asarray(g, np.float32), np.asarray(u, np.float32)
    return (np.where(g > 0, g, np.float32(0)).astype(np.float32) * u).astype(np.float32)


def swiglu64(g, u):
    """r = g / (1 + exp(-g)) * u in float64 from the float32 g and u (exp overflows to inf for g < -709: r = -0 * u)."""
    g, u = np.asarray(g, np.float32).astype(np.float64), np.asarray(u, np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g)) * u


def swiglu_tol(r, u):
    """|c - r| <= 4 * 2^-23 |r| + 2^-120 (1 + |u|): expf within 1 ulp, one add, one correctly rounded division and one
    multiplication come to at most 2.5 ulp, the factor 4 is margin over that; the absolute term covers g < -88.72, where
    expf(-g) overflows and the entry gives +-0 while the true |silu(g)| <= 88.73 e^-88.72 < 2^-121 (and results below
    the normal range)."""
    return 4.0 * 2.0 ** -23 * np.abs(r) + 2.0 ** -120 * (1.0 + np.abs(np.asarray(u, np.float32).astype(np.float64)))


def assert_swiglu(c, g, u, what=""):
    """c float32 against the bound; prints the largest err / tol. Returns it."""
    r = swiglu64(g, u)
    assert np.isfinite(r).all(), what
    err = np.abs(np.asarray(c, np.float32).astype(np.float64) - r)
    ratio = float((err / swiglu_tol(r, u)).max()) if err.size else 0.0
    print(f"swiglu {what}: max err / tol = {ratio:.4f}")
    assert np.isfinite(np.asarray(c)).all() and ratio <= 1.0, (what, ratio)
    return ratio
