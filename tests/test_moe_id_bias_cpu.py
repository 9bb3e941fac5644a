"""qg_gemm_w4a8_moe_prefill_bias / qg_gemm_w4a8_moe_batch_bias without a GPU: the exported symbols, the validation codes
of the new refusals and their order against their neighbours (on fake pointers that every call refuses before a launch),
type 39 in the two new config queries and still -3 in the two old ones and the two old entries, the config lines and the
R thresholds of the batch entry, and the host twin qg_gemm_w4a8_moe_bias_cpu against the NumPy model of
moe_id_bias_ref."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import moe_id_bias_ref as BR
import moe_ref as MR
from moe_id_bias_ref import MXFP4, Q4_K, Q6_K, TYPES, bits
from moe_ref import ROW_TYPES

P = ctypes.c_void_p
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("qg_gemm_w4a8_moe_prefill_bias", "qg_gemm_w4a8_moe_batch_bias")
BIG = 1 << 40  # a workspace size every shape here fits


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
    new = {"qg_gemm_w4a8_moe_prefill_bias", "qg_moe_prefill_bias_config", "qg_gemm_w4a8_moe_batch_bias",
           "qg_moe_batch_bias_config", "qg_mul_mat_id_bias_from_view_ws", "qg_mul_mat_id_bias_from_view_batch"}
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert new <= set(re.findall(r" T (qg_\w+)", nm)) and new <= set(L.SIGNATURES)
    nm = subprocess.run(["nm", "-D", "--defined-only", H.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "qg_gemm_w4a8_moe_bias_cpu" in re.findall(r" T (qg_\w+)", nm) and "qg_gemm_w4a8_moe_bias_cpu" in H.SIGNATURES
    assert {"gemm_w4a8_moe_prefill_bias", "moe_prefill_bias_config", "gemm_w4a8_moe_batch_bias",
            "moe_batch_bias_config"} <= set(quant_gemm.__all__)
    assert callable(G.mul_mat_id_bias_from_ggml_ws) and callable(G.mul_mat_id_bias_from_ggml_batch)
    assert callable(H.gemm_w4a8_moe_bias)
    hdr = open(os.path.join(REPO, "include", "qg", "qg.h")).read()
    for sym in new:
        assert re.search(rf"\bint {sym}\(", hdr), sym
    assert re.search(r"\bint qg_gemm_w4a8_moe_bias_cpu\(", open(os.path.join(REPO, "include", "qg", "qg_host.h")).read())


# ---------------------------------------------------------------------------- validation
def call(so, entry, A=4096, a_rows=1, B=4096, bias=4096, bias_stride=0, n_expert=4, ids=4096, ids_stride=2, C=4096, ldc=0, T=1,
         n_used=2, N=8, K=256, t=MXFP4, ws=4096, wsb=BIG):
    p = lambda v: None if v is None else P(v)
    return getattr(so, entry)(p(A), a_rows, p(B), p(bias), bias_stride, n_expert, p(ids), ids_stride, p(C), ldc, T, n_used, N, K,
                              t, p(ws), wsb, None)


# what a later check refuses, so that a call whose earlier checks all pass still launches nothing on the fake pointers
LATE = {"T": 65536, "n_used": 1, "ids_stride": 1}  # more than 65535 slots: -3, after every -1 and -4


@pytest.mark.parametrize("entry", ENTRIES)
def test_validation_codes_and_their_order(so, entry):
    """Every call here is refused (or empty) before anything is enqueued: the pointers are never dereferenced."""
    c = functools.partial(call, so, entry)
    assert c(**LATE) == -3  # the baseline of the calls below
    # the order of the entry beside it up to the type, with 39 among the types and its granule of 32
    assert c(T=-1, K=33) == -1 and c(K=33) == -2 and c(K=0) == -2 and c(K=288, **LATE) == -3
    for t in (Q4_K, Q6_K):  # the K-quants still need K % 256 == 0
        assert c(K=288, t=t) == -2 and c(K=32, t=t) == -2 and c(K=256, t=t, **LATE) == -3
    for t in ROW_TYPES + (9, 13, 26, 0, 1, 5, 38, 40):
        assert c(t=t, T=0, A=None) == -3 and c(t=t) == -3, t
    for t in TYPES:  # an empty call is QG_OK whatever the rest holds
        assert c(A=None, B=None, bias=4097, ids=None, C=None, ws=None, wsb=0, bias_stride=-1, t=t, N=0) == 0
        assert c(T=0, t=t) == 0 and c(n_used=0, ids_stride=0, t=t) == 0
    # a null bias is no null pointer; a null required pointer comes before any alignment
    assert c(bias=None, **LATE) == -3
    assert c(A=None, bias=4098) == -1 and c(C=None, bias=4097) == -1 and c(ids=None, bias=4097) == -1
    # a non-null bias off 4 B: ALIGN beside the other pointers, before every INVALID_ARG and the workspace checks
    for b in (4097, 4098, 4099):
        for later in ({}, {"ids_stride": 1}, {"n_expert": 0}, {"bias_stride": -1}, {"a_rows": 3}, {"ws": None}, {"ws": 4100},
                      {"wsb": 0}, {"n_expert": 4097}, LATE):
            assert c(bias=b, **later) == -4, (b, later)
            assert c(bias=b, t=Q4_K, **later) == -4 and c(bias=b, t=Q6_K, **later) == -4, (b, later)
    assert c(A=4098, **LATE) == -4 and c(ids=4097, **LATE) == -4
    # MXFP4 weights need no alignment and any expert stride (Q4_K 16 B, Q6_K 2 B as ever)
    for off in (1, 2, 3):
        assert c(B=4096 + off, **LATE) == -3 and c(B=4096 + off, N=1, K=32, **LATE) == -3
    assert c(B=4104, t=Q4_K, **LATE) == -4 and c(B=4097, t=Q6_K, **LATE) == -4
    # bias_stride: INVALID_ARG beside ids_stride, whether or not a bias is given, before the workspace and every UNSUPPORTED
    for bs in (-1, 1, 7, -2 ** 40):
        for later in ({}, LATE, {"bias": None}, {"ws": 4100}, {"ws": None}, {"wsb": 0}, {"n_expert": 4097}):
            assert c(bias_stride=bs, **later) == -1, (bs, later)
    assert c(bias_stride=8, **LATE) == -3 and c(bias_stride=0, **LATE) == -3 and c(bias_stride=2 ** 40, **LATE) == -3
    # the neighbours keep their codes
    assert c(ids_stride=1) == -1 and c(n_expert=0) == -1 and c(ldc=7) == -1 and c(ldc=-8) == -1 and c(a_rows=3) == -1
    # the workspace: null INVALID_ARG, off 16 B ALIGN, short INVALID_ARG -- all before the UNSUPPORTED shapes
    size = getattr(so, entry.replace("_bias", "") + "_workspace_size")
    for later in (LATE, {"n_expert": 4097}, {"n_expert": 4097, "T": 7}):  # (each refused later: nothing is launched)
        kw = dict(later)
        T, n_used, n_expert = kw.get("T", 1), kw.get("n_used", 2), kw.get("n_expert", 4)
        need = size(T, n_used, n_expert)
        assert need > 0
        assert c(ws=None, **kw) == -1 and c(ws=4100, **kw) == -4 and c(ws=4104, **kw) == -4
        assert c(wsb=need - 1, **kw) == -1 and c(wsb=0, **kw) == -1 and c(wsb=need, **kw) == -3
    # then the unsupported shapes: more than 65535 slots, more than 4096 experts
    assert c(T=65536, n_used=1, ids_stride=1) == -3 and c(T=32768, n_used=2) == -3
    assert c(n_expert=4097, **LATE) == -3
    assert c(n_expert=4097, T=0) == 0


def test_old_entries_still_refuse_type_39(so):
    fake = P(4096)
    for name in ("qg_gemm_w4a8_moe_prefill", "qg_gemm_w4a8_moe_batch"):
        f = getattr(so, name)
        assert f(fake, 1, fake, 4, fake, 2, fake, 0, 1, 2, 8, 256, MXFP4, fake, BIG, None) == -3
        assert f(fake, 1, fake, 4, fake, 2, fake, 0, 0, 2, 8, 256, MXFP4, fake, BIG, None) == -3  # (even when empty)
        assert f(fake, 1, fake, 4, fake, 2, fake, 0, 65536, 2, 8, 256, Q4_K, fake, BIG, None) == -3


def test_batch_entry_refuses_a_k_whose_two_rows_do_not_fit(so):
    assert call(so, ENTRIES[1], K=54624) == -3 and call(so, ENTRIES[1], K=54624, bias_stride=3) == -1
    assert call(so, ENTRIES[1], K=54592, **LATE) == -3


# ---------------------------------------------------------------------------- the config lines
def cfg(so, name, T, n_used, n_expert, N, K, t):
    buf = ctypes.create_string_buffer(256)
    rc = getattr(so, name)(T, n_used, n_expert, N, K, t, buf, 256)
    return rc, buf.value.decode()


def test_type_39_is_the_new_queries_alone(so):
    for n_used in (1, 4):
        assert cfg(so, "qg_moe_prefill_config", 3, n_used, 8, 64, 512, MXFP4) == (-3, "")
        assert cfg(so, "qg_moe_batch_config", 3, n_used, 8, 64, 512, MXFP4) == (-3, "")
        rc, line = cfg(so, "qg_moe_prefill_bias_config", 3, n_used, 8, 64, 512, MXFP4)
        assert rc == 0 and line.startswith("moe:mxfp4_mmq "), (rc, line)
        rc, line = cfg(so, "qg_moe_batch_bias_config", 3, n_used, 8, 64, 512, MXFP4)
        assert rc == 0 and line.startswith("moeb:mxfp4_gemv "), (rc, line)
    for t in ROW_TYPES:
        assert cfg(so, "qg_moe_prefill_bias_config", 3, 2, 8, 64, 512, t)[0] == -3
        assert cfg(so, "qg_moe_batch_bias_config", 3, 2, 8, 64, 512, t)[0] == -3


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
def test_kquant_config_lines_are_the_old_entries(so, t):
    for k in (256, 512, 1024, 2304, 4096):
        for T, n_used, n_expert in ((3, 1, 8), (40, 2, 4), (300, 4, 8), (64, 8, 128)):
            for n in (1, 300, 4096):
                for kind in ("prefill", "batch"):
                    a = cfg(so, f"qg_moe_{kind}_bias_config", T, n_used, n_expert, n, k, t)
                    b = cfg(so, f"qg_moe_{kind}_config", T, n_used, n_expert, n, k, t)
                    assert a == b and a[0] == 0, (a, b)
        assert cfg(so, "qg_moe_prefill_bias_config", 3, 1, 8, 64, k + 32, t)[0] == -2


@pytest.mark.parametrize("per", [1, 16, 17, 32, 33])
def test_prefill_config_line(so, per):
    """moe:mxfp4_mmq TT=.. RG=.. KS=.. R=.. grid=XxY: the general rule of the entry beside it on the expected rows per
    expert (no Q6_K exception: K <= 1024 too), KS = 8 / RG, R = 16 TT, X the row tiles of 16 RG, Y moe_max_tiles."""
    n_expert = 3
    for n_used in (1, 2):
        for k in (96, 1024, 2912):
            for n in (1, 17, 2880):
                T = -(-(per * n_expert - n_expert + 1) // n_used)
                slots = T * n_used
                if -(-slots // n_expert) != per:
                    continue
                rc, line = cfg(so, "qg_moe_prefill_bias_config", T, n_used, n_expert, n, k, MXFP4)
                assert rc == 0 and line.startswith("moe:mxfp4_mmq "), (rc, line)
                f = MR.cfg_fields(line)[1]
                tt, rg = int(f["TT"]), int(f["RG"])
                want = BR.prefill_form_rg1(slots, n_expert)
                assert tt == want[0] and (rg == want[1] if want[1] else rg in (1, 4)), (line, want)
                assert int(f["KS"]) == 8 // rg and int(f["R"]) == 16 * tt
                assert f["grid"] == f"{-(-n // (16 * rg))}x{BR.max_tiles(slots, n_expert, 16 * tt)}", line
                # the K-quants' rule at the same slots (Q4_K has no exception of its own)
                ref = MR.cfg_fields(cfg(so, "qg_moe_prefill_config", T, n_used, n_expert, n, 2816, Q4_K)[1])[1]
                assert (f["TT"], f["RG"]) == (ref["TT"], ref["RG"])


@pytest.mark.parametrize("units", list(range(3, 92, 8)) + [15, 16, 17, 63, 64, 65, 90])
def test_batch_config_line(so, units):
    """moeb:mxfp4_gemv R=.. LPR=.. WGS=.. ONE=.. grid=XxY lds=..: LPR / WGS / ONE those of qg_moe_config for the same K,
    R by the expected rows per expert, lds = R * K/32 * 48."""
    k = 32 * units
    lpr, wgs, one = BR.mxfp4_form(k)
    rpb = wgs // 64 * (64 // lpr)
    rc, single = so_moe_config(so, 3, 2, 67, k)
    assert rc == 0 and single.startswith("moe:mxfp4_gemv ")
    s = MR.cfg_fields(single)[1]
    assert (int(s["LPR"]), int(s["WGS"]), int(s["ONE"])) == (lpr, wgs, one)
    for T, n_used, n_expert in ((1, 1, 1), (4, 2, 4), (9, 1, 3), (16, 4, 8), (64, 4, 32)):
        slots = T * n_used
        r = BR.batch_rows(slots, n_expert, k)
        for n in (1, rpb - 1, rpb + 1, 2880):
            rc, line = cfg(so, "qg_moe_batch_bias_config", T, n_used, n_expert, n, k, MXFP4)
            assert rc == 0 and line.startswith("moeb:mxfp4_gemv "), (rc, line)
            f = MR.cfg_fields(line)[1]
            assert (int(f["R"]), int(f["LPR"]), int(f["WGS"]), int(f["ONE"])) == (r, lpr, wgs, one), line
            assert f["grid"] == f"{-(-n // rpb)}x{BR.max_tiles(slots, n_expert, r)}", line
            assert int(f["lds"]) == r * units * 48, line


def so_moe_config(so, T, n_used, N, K):
    buf = ctypes.create_string_buffer(256)
    rc = so.qg_moe_config(T, n_used, N, K, MXFP4, buf, 256)
    return rc, buf.value.decode()


@pytest.mark.parametrize("k,r,r_next", [(13632, 8, 4), (27296, 4, 2), (54592, 2, 0)])
def test_batch_r_thresholds_are_exact(so, k, r, r_next):
    """R rows of K/32 records of 48 B fit 160 KiB up to these K and not 32 elements further; qg.h states them."""
    assert r * (k // 32) * 48 <= BR.MAX_LDS_BYTES < r * (k // 32 + 1) * 48
    rc, line = cfg(so, "qg_moe_batch_bias_config", 64, 1, 1, 8, k, MXFP4)  # 64 rows on one expert: R = 8 where it fits
    assert rc == 0 and int(MR.cfg_fields(line)[1]["R"]) == r and int(MR.cfg_fields(line)[1]["lds"]) == r * (k // 32) * 48
    rc, line = cfg(so, "qg_moe_batch_bias_config", 64, 1, 1, 8, k + 32, MXFP4)
    if r_next:
        assert rc == 0 and int(MR.cfg_fields(line)[1]["R"]) == r_next, line
    else:
        assert (rc, line) == (-3, "")
    assert BR.batch_rows(64, 1, k) == r and BR.batch_rows(64, 1, k + 32) == r_next
    hdr = open(os.path.join(REPO, "include", "qg", "qg.h")).read()
    assert re.search(rf"\b{k}\b", hdr), f"qg.h does not give the threshold {k}"


# ---------------------------------------------------------------------------- the host twin
N_EXPERT, T, N_USED, N = 5, 3, 4, 41
BIAS_STRIDE = N + 5


@functools.lru_cache(maxsize=None)
def operands(t, k):
    """Experts, activations (a row per token; a row per slot), ids with -1 and n_expert among them in a wider array,
    a bias with a NaN gap after each row. Host arrays, shared, never modified."""
    rng = np.random.default_rng([t, k])
    w = BR.random_experts(rng, t, N_EXPERT, N, k)
    a1, an = MR.random_act(rng, T, k), MR.random_act(rng, T * N_USED, k)
    ids = np.full((T, N_USED + 3), 12345, np.int32)
    ids[:, :N_USED] = rng.integers(0, N_EXPERT, (T, N_USED))
    ids[0, 1], ids[T - 1, 0] = -1, N_EXPERT
    bias = BR.random_bias(rng, N_EXPERT, N, BIAS_STRIDE)[1:-1]
    return w, a1, an, ids, np.ascontiguousarray(bias)


@pytest.mark.parametrize("k", [96, 512, 2912])
@pytest.mark.parametrize("t", TYPES)
def test_host_twin(H, t, k):
    if t != MXFP4 and k % 256:
        k = 768
    w, a1, an, ids, bias = operands(t, k)
    for a_rows, a in ((1, a1), (N_USED, an)):
        old = H.gemm_w4a8_moe(a, w, ids, T, N_USED, N, k, t, a_rows=a_rows)
        none = H.gemm_w4a8_moe_bias(a, w, None, ids, T, N_USED, N, k, t, a_rows=a_rows)
        assert np.array_equal(bits(none), bits(old))  # a null bias: qg_gemm_w4a8_moe_cpu, bit for bit
        got = H.gemm_w4a8_moe_bias(a, w, bias, ids, T, N_USED, N, k, t, a_rows=a_rows, threads=3)
        assert np.isfinite(got).all()  # neither the NaN gap nor a row of another expert was read
        assert np.array_equal(bits(got), bits(BR.add_bias(old, bias, ids, N_EXPERT)))
        assert (bits(got[0, 1]) == 0).all() and (bits(got[T - 1, 0]) == 0).all()  # +0.0f: no bias on a bad id
        assert not np.array_equal(bits(got), bits(old))
        if t == MXFP4:  # the whole float32 chain in NumPy, product and add
            assert np.array_equal(bits(got), bits(BR.moe_chain_f32(a, w, bias, ids, N_USED, a_rows)))
        # and against the float64 contract: the decode order's bound (W = 0) plus the add's half ulp
        R = BR.ref_mod(t)
        for tt in range(T):
            for u in range(N_USED):
                e = int(ids[tt, u])
                if 0 <= e < N_EXPERT:
                    c64, _, mag = R.gemm(a[tt * a_rows + u % a_rows][None], w[e])
                    ref = c64[0] + bias[e, :N].astype(np.float64)
                    err = np.abs(got[tt, u].astype(np.float64) - ref)
                    assert (err <= R.tol(mag[0], k, 0) + 2.0 ** -24 * np.abs(ref)).all()


def test_twin_validation(H):
    so = H.load()
    one = np.zeros(4096, np.uint8)
    p = P(one.ctypes.data)
    c = lambda **kw: so.qg_gemm_w4a8_moe_bias_cpu(kw.get("A", p), kw.get("a_rows", 1), p, p, kw.get("bs", 0), 1, p, 1, p, 0, 1, 1, 8,
                                                  kw.get("K", 32), kw.get("t", MXFP4), 1)
    assert c() == 0 and c(K=33) == -2 and c(t=2) == -3 and c(bs=7) == -1 and c(bs=-1) == -1 and c(K=32, t=Q4_K) == -2
    assert c(A=None, bs=7) == -1 and c(a_rows=2) == -1 and c(bs=8) == 0
