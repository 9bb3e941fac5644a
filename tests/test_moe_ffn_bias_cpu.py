"""qg_gemm_w4a8_moe_glu_bias / qg_gemm_w4a8_moe_down_bias without a GPU: the exported symbols, the validation codes of
the new refusals and their order against their neighbours (on fake pointers that every call refuses before a launch),
type 39 in the two new config queries and still -3 in the two old ones, the config lines against qg_moe_config and the
documented SW / RPB / LDS rules, and the two host twins against the float32 model of moe_ffn_bias_ref on the products of
qg_gemm_w4a8_moe_cpu (ReGLU and down: bits; SWIGLU_OAI: the derived bound)."""
import ctypes
import functools
import math
import os
import re
import subprocess

import numpy as np
import pytest

import moe_down_ref as DR
import moe_ffn_bias_ref as FR
import moe_glu_ref as GR
import moe_ref as MR
from moe_ffn_bias_ref import MXFP4, REGLU, SWIGLU, SWIGLU_OAI, bits
from moe_ref import Q4_K, Q6_K, ROW_TYPES

P = ctypes.c_void_p
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = (MXFP4, Q4_K, Q6_K)
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def so():
    import quant_gemm._lib as L
    return L.load()


@pytest.fixture(scope="module")
def H():
    import quant_gemm.host as H
    H.load()
    return H


# ---------------------------------------------------------------------------- surface
def test_new_symbols_are_exported(H):
    import quant_gemm
    import quant_gemm._lib as L
    import quant_gemm.ggml as G
    new = {"qg_gemm_w4a8_moe_glu_bias", "qg_moe_glu_bias_config", "qg_gemm_w4a8_moe_down_bias", "qg_moe_down_bias_config",
           "qg_mul_mat_id_glu_bias_from_view", "qg_mul_mat_id_down_bias_from_view"}
    twins = {"qg_gemm_w4a8_moe_glu_bias_cpu", "qg_gemm_w4a8_moe_down_bias_cpu"}
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert new <= set(re.findall(r" T (qg_\w+)", nm)) and new <= set(L.SIGNATURES)
    nm = subprocess.run(["nm", "-D", "--defined-only", H.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert twins <= set(re.findall(r" T (qg_\w+)", nm)) and twins <= set(H.SIGNATURES)
    assert {"gemm_w4a8_moe_glu_bias", "moe_glu_bias_config", "gemm_w4a8_moe_down_bias", "moe_down_bias_config",
            "GLU_SWIGLU_OAI"} <= set(quant_gemm.__all__)
    assert quant_gemm.GLU_SWIGLU_OAI == 3 == H.GLU_SWIGLU_OAI == SWIGLU_OAI
    assert callable(G.mul_mat_id_glu_bias_from_ggml) and callable(G.mul_mat_id_down_bias_from_ggml)
    assert callable(H.gemm_w4a8_moe_glu_bias) and callable(H.gemm_w4a8_moe_down_bias)
    hdr = open(os.path.join(REPO, "include", "qg", "qg.h")).read()
    assert re.search(r"#define QG_GLU_SWIGLU_OAI\s+3\b", hdr)
    for sym in new:
        assert re.search(rf"\bint {sym}\(", hdr), sym
    hh = open(os.path.join(REPO, "include", "qg", "qg_host.h")).read()
    for sym in twins:
        assert re.search(rf"\bint {sym}\(", hh), sym


# ---------------------------------------------------------------------------- validation
def glu(so, A=4096, Bg=4096, Bu=8192, bg=4096, bu=4096, bias_stride=0, n_expert=4, ids=4096, ids_stride=2, C=4096, ldc=0, T=1,
        n_used=2, N=8, K=256, t=MXFP4, op=SWIGLU_OAI, alpha=1.702, limit=7.0):
    p = lambda v: None if v is None else P(v)
    return so.qg_gemm_w4a8_moe_glu_bias(p(A), p(Bg), p(Bu), p(bg), p(bu), bias_stride, n_expert, p(ids), ids_stride, p(C), ldc,
                                        T, n_used, N, K, t, op, alpha, limit, None)


def down(so, A=4096, B=4096, bias=4096, bias_stride=0, n_expert=4, ids=4096, ids_stride=2, W=4096, w_stride=2, C=4096, ldc=0,
         T=1, n_used=2, N=8, K=256, t=MXFP4):
    p = lambda v: None if v is None else P(v)
    return so.qg_gemm_w4a8_moe_down_bias(p(A), p(B), p(bias), bias_stride, n_expert, p(ids), ids_stride, p(W), w_stride, p(C),
                                         ldc, T, n_used, N, K, t, None)


# what a later check refuses, so that a call whose earlier checks all pass still launches nothing on the fake pointers
LATE = {"T": 65536, "n_used": 1, "ids_stride": 1}  # more than 65535 slots / tokens: -3, after every -1 and -4


def test_glu_validation_codes_and_their_order(so):
    """Every call here is refused (or empty) before anything is enqueued: the pointers are never dereferenced."""
    assert glu(so, **LATE) == -3 and glu(so, op=SWIGLU, **LATE) == -3  # the baseline of the calls below
    # the order of qg_gemm_w4a8_moe_glu up to the type, with 39 among the types and its granule of 32
    assert glu(so, T=-1, K=33) == -1 and glu(so, K=33) == -2 and glu(so, K=0) == -2
    assert glu(so, K=288, t=Q4_K) == -2 and glu(so, K=288, t=Q6_K) == -2 and glu(so, K=288, **LATE) == -3
    for t in ROW_TYPES + (9, 13, 26, 0, 1, 5, 38, 40):
        assert glu(so, t=t, T=0, A=None) == -3 and glu(so, t=t) == -3, t
    for t in TYPES:
        assert glu(so, A=None, Bg=None, Bu=None, bg=4097, ids=None, C=None, bias_stride=-1, alpha=NAN, t=t, N=0) == 0
    # a null bias is no null pointer; a null required pointer comes before any alignment
    assert glu(so, bg=None, bu=None, **LATE) == -3 and glu(so, bg=None, **LATE) == -3 and glu(so, bu=None, **LATE) == -3
    assert glu(so, A=None, bg=4098) == -1 and glu(so, C=None, bu=4097) == -1
    # a non-null bias off 4 B: ALIGN beside the other pointers, before every INVALID_ARG that follows
    for kw in ({"bg": 4097}, {"bg": 4098}, {"bu": 4099}, {"bu": 4098, "bg": None}):
        for later in ({}, {"ids_stride": 1}, {"n_expert": 0}, {"bias_stride": -1}, {"alpha": NAN}, {"op": 1}, LATE):
            assert glu(so, **kw, **later) == -4, (kw, later)
            assert glu(so, t=Q4_K, **kw, **later) == -4, (kw, later)
    # MXFP4 weights need no alignment (Q4_K 16 B, Q6_K 2 B as ever)
    assert glu(so, Bg=4097, Bu=8195, **LATE) == -3
    assert glu(so, Bg=4104, t=Q4_K, **LATE) == -4 and glu(so, Bu=4097, t=Q6_K, **LATE) == -4
    # bias_stride: INVALID_ARG beside ids_stride, whether or not a bias is given, before every UNSUPPORTED
    for bs in (-1, 1, 7, -2 ** 40):
        for later in ({}, {"op": 1}, LATE, {"bg": None, "bu": None}):
            assert glu(so, bias_stride=bs, **later) == -1, (bs, later)
    assert glu(so, bias_stride=8, **LATE) == -3 and glu(so, bias_stride=0, **LATE) == -3 and glu(so, bias_stride=2 ** 40, **LATE) == -3
    # alpha and limit: read for the OAI op alone, INVALID_ARG before every UNSUPPORTED
    bad = ({"alpha": NAN}, {"alpha": INF}, {"alpha": -INF}, {"limit": NAN}, {"limit": INF}, {"limit": 0.0}, {"limit": -7.0})
    for kw in bad:
        assert glu(so, **kw) == -1 and glu(so, **kw, **LATE) == -1, kw
        for op in (SWIGLU, REGLU):
            assert glu(so, op=op, **kw, **LATE) == -3, kw
        assert glu(so, op=1, **kw) == -3, kw
    assert glu(so, alpha=-1.0, limit=1e-30, **LATE) == -3
    # the neighbours keep their codes
    assert glu(so, ids_stride=1) == -1 and glu(so, n_expert=0) == -1 and glu(so, ldc=7) == -1 and glu(so, ldc=-8) == -1
    # the entry's own refusals: an unknown glu_op, the LDS records of one row beyond 160 KiB
    for op in (1, 4, -1, 2 ** 31 - 1):
        for t in TYPES:
            assert glu(so, op=op, t=t) == -3, (op, t)
    assert glu(so, K=(FR.MAX_LDS_BYTES // FR.MXFP4_REC_BYTES + 1) * 32) == -3
    for t in (Q4_K, Q6_K):
        assert glu(so, K=(FR.MAX_LDS_BYTES // MR.KQ_REC_BYTES[t] + 1) * 256, t=t) == -3


def test_down_validation_codes_and_their_order(so):
    assert down(so, **LATE) == -3
    assert down(so, T=-1, K=33) == -1 and down(so, K=33) == -2 and down(so, K=288, t=Q4_K) == -2 and down(so, K=288, **LATE) == -3
    for t in ROW_TYPES + (9, 13, 26, 0, 1, 5, 38, 40):
        assert down(so, t=t, T=0, A=None) == -3 and down(so, t=t) == -3, t
    for t in TYPES:
        assert down(so, A=None, B=None, bias=4097, ids=None, W=4099, C=None, bias_stride=-1, t=t, n_used=0) == 0
    assert down(so, bias=None, **LATE) == -3 and down(so, bias=None, W=None, **LATE) == -3
    assert down(so, ids=None, bias=4098) == -1
    for later in ({}, {"ids_stride": 1}, {"w_stride": 1}, {"bias_stride": 3}, LATE):
        assert down(so, bias=4098, **later) == -4 and down(so, bias=4097, t=Q6_K, **later) == -4, later
    assert down(so, B=4099, **LATE) == -3 and down(so, B=4104, t=Q4_K, **LATE) == -4
    for bs in (-1, 1, 7):
        for later in ({}, LATE, {"bias": None}, {"K": 2 ** 20}):
            assert down(so, bias_stride=bs, **later) == -1, (bs, later)
    assert down(so, bias_stride=8, **LATE) == -3 and down(so, bias_stride=9, **LATE) == -3
    assert down(so, ids_stride=1) == -1 and down(so, w_stride=1) == -1 and down(so, ldc=7) == -1
    assert down(so, w_stride=1, W=None, **LATE) == -3  # (w_stride is not looked at without weights)
    # T is what 65535 bounds, not the slots
    assert down(so, T=65536, n_used=2) == -3
    # the LDS need: the formula's first K that does not fit
    for n_used in (1, 2, 5):
        k = FR.mxfp4_down_max_k(n_used) + 32
        assert down(so, n_used=n_used, ids_stride=n_used, w_stride=n_used, K=k) == -3


# ---------------------------------------------------------------------------- the config lines
def cfg(so, name, T, n_used, N, K, t):
    buf = ctypes.create_string_buffer(256)
    rc = getattr(so, name)(T, n_used, N, K, t, buf, 256)
    return rc, buf.value.decode()


def test_type_39_is_the_new_queries_alone(so):
    for n_used in (1, 4):
        assert cfg(so, "qg_moe_glu_config", 3, n_used, 64, 512, MXFP4) == (-3, "")
        assert cfg(so, "qg_moe_down_config", 3, n_used, 64, 512, MXFP4) == (-3, "")
        rc, line = cfg(so, "qg_moe_glu_bias_config", 3, n_used, 64, 512, MXFP4)
        assert rc == 0 and line.startswith("moe_glu:mxfp4_gemv "), (rc, line)
        rc, line = cfg(so, "qg_moe_down_bias_config", 3, n_used, 64, 512, MXFP4)
        assert rc == 0 and line.startswith("moe_down:mxfp4_gemv ") and " SW=" in line, (rc, line)
    for t in ROW_TYPES:
        assert cfg(so, "qg_moe_glu_bias_config", 3, 2, 64, 512, t)[0] == -3
        assert cfg(so, "qg_moe_down_bias_config", 3, 2, 64, 512, t)[0] == -3


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
def test_kquant_config_lines_are_the_old_entries(so, t):
    for k in (256, 512, 1024, 2304, 4096):
        for n_used in (1, 3, 8):
            for n in (1, 300, 4096):
                a, b = cfg(so, "qg_moe_glu_bias_config", 3, n_used, n, k, t), cfg(so, "qg_moe_glu_config", 3, n_used, n, k, t)
                assert a == b and a[0] == 0, (a, b)
                a, b = cfg(so, "qg_moe_down_bias_config", 3, n_used, n, k, t), cfg(so, "qg_moe_down_config", 3, n_used, n, k, t)
                assert a == b and a[0] == 0, (a, b)


@pytest.mark.parametrize("units", [3, 9, 16, 29, 64, 90, 91])
def test_mxfp4_config_lines(so, units):
    k = 32 * units
    lpr, wgs, one = FR.mxfp4_form(k)
    for n in (1, 67, 300, 2880):
        rc, ref = cfg(so, "qg_moe_config", 3, 2, n, k, MXFP4)
        assert rc == 0 and ref.startswith("moe:mxfp4_gemv ")
        rc, line = cfg(so, "qg_moe_glu_bias_config", 3, 2, n, k, MXFP4)
        assert rc == 0 and line.startswith("moe_glu:mxfp4_gemv ")
        assert line.split(" ")[1:] == ref.split(" ")[1:], (line, ref)  # LPR, WGS, ONE, grid, lds
        f = MR.cfg_fields(ref)[1]
        assert (int(f["LPR"]), int(f["WGS"]), int(f["ONE"])) == (lpr, wgs, one), ref
        for n_used in (1, 3, 4, 8, 16):
            rc, line = cfg(so, "qg_moe_down_bias_config", 5, n_used, n, k, MXFP4)
            assert rc == 0, (rc, line)
            v = DR.launch(line)
            sw, rpb = FR.down_sw_rpb(n_used, lpr, wgs)
            assert v["family"] == "mxfp4_gemv" and (v["LPR"], v["WGS"], v["ONE"]) == (lpr, wgs, one), line
            assert (v["SW"], v["RPB"]) == (sw, rpb) and sw <= min(n_used, wgs // 64) < 2 * sw, line
            assert v["grid"] == f"{math.ceil(n / rpb)}x5" and v["lds"] == FR.mxfp4_down_lds(n_used, k), line


@pytest.mark.parametrize("n_used", [1, 3, 4, 8, 16])
def test_mxfp4_down_lds_bound_is_exact(so, n_used):
    k = FR.mxfp4_down_max_k(n_used)
    assert FR.mxfp4_down_lds(n_used, k) <= FR.MAX_LDS_BYTES < FR.mxfp4_down_lds(n_used, k + 32)
    rc, line = cfg(so, "qg_moe_down_bias_config", 2, n_used, 100, k, MXFP4)
    assert rc == 0 and int(MR.cfg_fields(line)[1]["lds"]) == FR.mxfp4_down_lds(n_used, k), (rc, line)
    assert cfg(so, "qg_moe_down_bias_config", 2, n_used, 100, k + 32, MXFP4) == (-3, "")
    hdr = open(os.path.join(REPO, "include", "qg", "qg.h")).read()
    assert re.search(rf"\b{k}\b", hdr), f"qg.h does not give the largest MXFP4 K for n_used = {n_used}: {k}"


# ---------------------------------------------------------------------------- the host twins
N_EXPERT, T, N_USED, N = 5, 3, 4, 41
BIAS_STRIDE = N + 5


@functools.lru_cache(maxsize=None)
def operands(t, k):
    """Experts (gate, up, down), activations (a row per token; a row per slot), ids with -1 and n_expert among them,
    biases with a gap after each row, router weights. Host arrays, shared, never modified."""
    rng = np.random.default_rng([t, k])
    w = np.stack([FR.small_experts(rng, t, N_EXPERT, N, k) for _ in range(3)])
    a1, an = MR.random_act(rng, T, k), MR.random_act(rng, T * N_USED, k)
    ids = np.full((T, N_USED + 3), 12345, np.int32)
    ids[:, :N_USED] = rng.integers(0, N_EXPERT, (T, N_USED))
    ids[0, 1], ids[T - 1, 0] = -1, N_EXPERT
    bias = rng.uniform(-10.0, 10.0, (3, N_EXPERT, BIAS_STRIDE)).astype(np.float32)
    bias[:, :, N:] = np.nan  # the gap is never read
    rw = rng.uniform(0.05, 1.0, (T, N_USED + 2)).astype(np.float32)
    rw[0, 1] = np.nan  # the weight of an id out of range is never read
    return w, a1, an, ids, bias, rw


@pytest.mark.parametrize("k", [96, 512])
@pytest.mark.parametrize("t", TYPES)
def test_glu_twin(H, t, k):
    if t != MXFP4 and k % 256:
        k = 768
    w, a1, _, ids, bias, _ = operands(t, k)
    g = H.gemm_w4a8_moe(a1, w[0], ids, T, N_USED, N, k, t)
    u = H.gemm_w4a8_moe(a1, w[1], ids, T, N_USED, N, k, t)
    run = lambda bg, bu, op, **kw: H.gemm_w4a8_moe_glu_bias(a1, w[0], w[1], bg, bu, ids, T, N_USED, N, k, t, op, **kw)
    outs = []
    for bg, bu in ((bias[0], bias[1]), (None, bias[1]), (bias[0], None), (None, None)):
        want, gb, ub = FR.glu_model(g, u, bg, bu, ids, N_EXPERT, REGLU)
        got = run(bg, bu, REGLU)
        assert np.array_equal(bits(got), bits(want))
        assert (bits(got[0, 1]) == 0).all() and (bits(got[T - 1, 0]) == 0).all()  # +0.0f: no bias on a bad id
        outs.append(got)
        GR.assert_swiglu(FR.zero_bad(run(bg, bu, SWIGLU), ids, N_EXPERT), FR.zero_bad(gb, ids, N_EXPERT),
                         FR.zero_bad(ub, ids, N_EXPERT), f"twin t={t} k={k}")
    assert not any(np.array_equal(bits(outs[i]), bits(outs[j])) for i in range(4) for j in range(i))
    if t != MXFP4:  # null biases: the old twin, bit for bit
        for op in (REGLU, SWIGLU):
            assert np.array_equal(bits(run(None, None, op)), bits(H.gemm_w4a8_moe_glu(a1, w[0], w[1], ids, T, N_USED, N, k, t, op)))
    _, gb, ub = FR.glu_model(g, u, bias[0], bias[1], ids, N_EXPERT, SWIGLU_OAI)
    ok = (ids[:, :N_USED] >= 0) & (ids[:, :N_USED] < N_EXPERT)
    for alpha, limit in ((1.702, 7.0), (1.0, 0.5)):
        FR.assert_all_regions(gb[ok], ub[ok], limit, f"t={t} k={k}")
        got = run(bias[0], bias[1], SWIGLU_OAI, alpha=alpha, limit=limit)
        assert (bits(got[~ok]) == 0).all()
        FR.assert_oai(got[ok], gb[ok], ub[ok], alpha, limit, f"twin t={t} k={k}")
        assert np.abs(got).max() <= limit * (1.0 + limit) * 1.001


@pytest.mark.parametrize("k", [96, 512])
@pytest.mark.parametrize("t", TYPES)
def test_down_twin(H, t, k):
    if t != MXFP4 and k % 256:
        k = 768
    w, _, an, ids, bias, rw = operands(t, k)
    d = H.gemm_w4a8_moe(an, w[2], ids, T, N_USED, N, k, t, a_rows=N_USED)
    outs = []
    for b in (bias[2], None):
        for weights in (rw[:, :N_USED], None):
            want = DR.fold(FR.add_bias(d, b, ids, N_EXPERT), ids, weights, N_EXPERT)
            got = H.gemm_w4a8_moe_down_bias(an, w[2], b, ids, None if weights is None else rw, T, N_USED, N, k, t)
            assert np.isfinite(got).all() and np.array_equal(bits(got), bits(want))
            outs.append(got)
    assert not np.array_equal(bits(outs[0]), bits(outs[2]))
    if t != MXFP4:
        assert np.array_equal(bits(outs[2]), bits(H.gemm_w4a8_moe_down(an, w[2], ids, rw, T, N_USED, N, k, t)))
    # a token whose ids are all out of range: a row of +0.0f, its bias unread
    bad = ids.copy()
    bad[1, :N_USED] = (-1, N_EXPERT, -2 ** 31, 2 ** 31 - 1)
    got = H.gemm_w4a8_moe_down_bias(an, w[2], bias[2], bad, rw, T, N_USED, N, k, t)
    assert (bits(got[1]) == 0).all() and np.array_equal(bits(got[2]), bits(outs[0][2]))


def test_twin_validation(H):
    so = H.load()
    one = np.zeros(4096, np.uint8)
    p = P(one.ctypes.data)
    call = lambda **kw: so.qg_gemm_w4a8_moe_glu_bias_cpu(p, p, p, p, p, kw.get("bs", 0), 1, p, 1, p, 0, 1, 1, 8, kw.get("K", 32),
                                                         kw.get("t", MXFP4), kw.get("op", REGLU), kw.get("alpha", 1.0),
                                                         kw.get("limit", 1.0), 1)
    assert call() == 0 and call(K=33) == -2 and call(t=2) == -3 and call(bs=7) == -1 and call(bs=-1) == -1 and call(op=1) == -3
    assert call(op=SWIGLU_OAI, alpha=NAN) == -1 and call(op=SWIGLU_OAI, limit=0.0) == -1 and call(op=SWIGLU, limit=0.0) == 0
    dcall = lambda **kw: so.qg_gemm_w4a8_moe_down_bias_cpu(p, p, p, kw.get("bs", 0), 1, p, 1, None, 1, p, 0, 1, 1, 8,
                                                           kw.get("K", 32), kw.get("t", MXFP4), 1)
    assert dcall() == 0 and dcall(K=33) == -2 and dcall(t=2) == -3 and dcall(bs=7) == -1 and dcall(K=32, t=Q4_K) == -2
