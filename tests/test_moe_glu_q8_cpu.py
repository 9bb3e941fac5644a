"""qg_gemm_w4a8_moe_glu_q8_1 without a GPU: the surface, the validation order on fake pointers (refused before a launch),
the config line against qg_moe_glu_config, and the host twin against quantize-twin(glu-twin) and against float64."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import moe_ref as MR
from moe_glu_ref import REGLU, SWIGLU
from moe_ref import Q4_K, Q6_K, ROW_TYPES

FORMS = {256: ("4", "1", "1"), 512: ("4", "0", "1"), 1024: ("16", "1", "1"), 1280: ("16", "0", "1"),
         4096: ("64", "1", "2"), 4352: ("64", "0", "2")}  # K -> LPR, ONE, P


def test_surface():
    import quant_gemm
    import quant_gemm._lib as L
    import quant_gemm.host as H
    new = {"qg_gemm_w4a8_moe_glu_q8_1", "qg_moe_glu_q8_1_config"}
    nm = lambda path: subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    assert new <= set(re.findall(r" T (qg_\w+)", nm(L.LIB_PATH))) and new <= set(L.SIGNATURES)
    assert " T qg_gemm_w4a8_moe_glu_q8_1_cpu" in nm(H.LIB_PATH) and "qg_gemm_w4a8_moe_glu_q8_1_cpu" in H.SIGNATURES
    assert {"gemm_w4a8_moe_glu_q8_1", "moe_glu_q8_1_config"} <= set(quant_gemm.__all__) and callable(H.gemm_w4a8_moe_glu_q8_1)


def call(A=4096, Bg=4096, Bu=8192, n_expert=4, ids=4096, ids_stride=2, Hq=4096, T=1, n_used=2, N=32, K=256, t=Q4_K, op=SWIGLU):
    import quant_gemm._lib as L
    p = lambda v: None if v is None else ctypes.c_void_p(v)
    return L.load().qg_gemm_w4a8_moe_glu_q8_1(p(A), p(Bg), p(Bu), n_expert, p(ids), ids_stride, p(Hq), T, n_used, N, K, t, op, None)


def test_validation_order():
    """The float entry's order with H where C stood; N = 48 is refused last. No pointer is dereferenced."""
    assert call(T=-1, K=33, t=9) == -1 and call(K=33, t=9) == -2 and call(K=288) == -2
    for t in ROW_TYPES + (11, 23, 39, 13):  # the 32-element types, Q3_K, IQ4_XS, MXFP4, an id without a block
        assert call(t=t, T=0, A=None) == -3 and call(t=t) == -3, t
    for kw in ({"T": 0}, {"n_used": 0}, {"N": 0}):
        assert call(A=None, Bg=None, Bu=None, ids=None, Hq=None, n_expert=0, ids_stride=-3, op=1, **kw) == 0
    assert call(Hq=None, A=4098, N=48) == -1 and call(Hq=4098, n_expert=0, N=48) == -4 and call(Hq=4097, N=48) == -4
    assert call(Bu=4104, op=1, N=48) == -4 and call(ids_stride=1, N=48, op=1) == -1 and call(n_expert=0, N=48) == -1
    assert call(T=65536, n_used=1, ids_stride=1) == -3 and call(op=1) == -3 and call(op=3) == -3
    for t in (Q4_K, Q6_K):
        k0 = (160 * 1024 // MR.KQ_REC_BYTES[t] + 1) * 256
        assert call(K=k0, t=t) == -3  # LDS beyond 160 KiB
        assert call(N=48, t=t) == -3 and call(N=8, t=t) == -3 and call(N=33, t=t) == -3


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
@pytest.mark.parametrize("k", sorted(FORMS))
def test_config_line(t, k):
    import quant_gemm as qg
    for n in (32, 96, 160, 4096):
        fam, f = MR.cfg_fields(qg.moe_glu_q8_1_config(2, 3, n, k, t))
        g = MR.cfg_fields(qg.moe_glu_config(2, 3, n, k, t))[1]
        assert fam == ("q4k_gemv" if t == Q4_K else "q6k_gemv") and qg.moe_glu_q8_1_config(2, 3, n, k, t).startswith("moe_glu_q8:")
        assert (f["LPR"], f["WGS"], f["ONE"]) == (g["LPR"], g["WGS"], g["ONE"]) and (f["LPR"], f["ONE"], f["P"]) == FORMS[k]
        rpb = int(f["WGS"]) // 64 * (64 // int(f["LPR"]))
        qb = max(32, rpb)
        assert int(f["P"]) == qb // rpb and f["grid"] == f"{(n + qb - 1) // qb}x6"
        assert int(f["lds"]) == k // 256 * MR.KQ_REC_BYTES[t] + 4 * qb == int(g["lds"]) + 4 * qb


def f64_case(t):  # both test files' float64 case: T = 1, n_used = 2, N = 64, K = 1280, ids (2, 0)
    rng = np.random.default_rng([t, 64, 1280])
    return (MR.random_experts(rng, t, 3, 64, 1280), MR.random_experts(rng, t, 3, 64, 1280), MR.random_act(rng, 1, 1280),
            np.array([[2, 0]], np.int32))


def check_against_f64(h_q8, t, case):
    """|q f16(d) - h64| <= (9/16) (amax64 + max e) / 127 + e per block (1/2: rounding to an integer; 1/16 = 128 * 2^-11:
    d's f16 rounding; e: the ReGLU bound of the two decode products); d must be a normal f16 (asserted)."""
    gate, up, a, ids = case
    R = MR.KR if t == Q4_K else MR.QR
    for u, ex in enumerate(ids[0]):
        (G, _, mg), (U, _, mu) = R.gemm(a[:1], gate[ex]), R.gemm(a[:1], up[ex])
        tg, tu = R.tol(mg, 1280, 0), R.tol(mu, 1280, 0)
        h64 = (np.maximum(G, 0.0) * U).reshape(2, 32)
        e = (tg * np.abs(U) + np.abs(G) * tu + tg * tu).reshape(2, 32) + 2.0 ** -24 * np.abs(h64)
        amax = np.abs(h64).max(axis=1, keepdims=True)
        assert (amax / 127 >= 2.0 ** -14).all() and (amax / 127 <= 65504).all()
        blk = np.ascontiguousarray(h_q8[0, u])
        dq = blk[:, 4:].view(np.int8).astype(np.float64) * blk[:, 0:2].copy().view(np.float16).astype(np.float64)
        err, bound = np.abs(dq - h64), 9 / 16 * (amax + e.max(axis=1, keepdims=True)) / 127 + e
        print(f"t={t} slot {u}: max err / bound = {(err / bound).max():.4f}")
        assert (err <= bound).all()


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
def test_host_twin(t):
    """Byte-equal to quantize-twin(glu-twin), out-of-range ids (zero bytes) among them, and inside the float64 bound."""
    import quant_gemm.host as H
    rng = np.random.default_rng([t, 9])
    gate, up, a = MR.random_experts(rng, t, 4, 96, 512), MR.random_experts(rng, t, 4, 96, 512), MR.random_act(rng, 2, 512)
    ids = np.array([[0, -1, 3, 1], [4, 2, 2, 1]], np.int32)
    for op in (REGLU, SWIGLU):
        h = H.gemm_w4a8_moe_glu_q8_1(a, gate, up, ids, 2, 3, 96, 512, t, op)
        assert h.shape == (2, 3, 3, 36) and np.array_equal(h, H.quantize_q8_1(H.gemm_w4a8_moe_glu(a, gate, up, ids, 2, 3, 96, 512, t, op)))
        assert not h[0, 1].any() and not h[1, 0].any() and h[0, 0].any()
    case = f64_case(t)
    check_against_f64(H.gemm_w4a8_moe_glu_q8_1(case[2], case[0], case[1], case[3], 1, 2, 64, 1280, t, REGLU), t, case)
