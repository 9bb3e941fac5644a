"""qg_gemm_w4a8_moe without a GPU: the exported symbols, the validation codes and their order (on fake pointers
that every call refuses before a launch), qg_moe_config against qg_debug_config, and the host twin
qg_gemm_w4a8_moe_cpu against per-slot qg_gemm_w4a8_cpu_mt (bits) and against the NumPy / oracle models (W = 0)."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import moe_ref as MR
from moe_ref import ALL_TYPES, Q4_0, Q4_K, Q6_K, Q8_0, ROW_TYPES

P = ctypes.c_void_p
CONFIG_K = (256, 512, 1024, 2304, 4096, 4352)  # 512: LPR = 4 with the unit loop (super-block types)


@pytest.fixture(scope="module")
def so():
    import quant_gemm._lib as L
    return L.load()


@pytest.fixture(scope="module")
def H():
    import quant_gemm.host as H
    H.load()
    return H


def test_new_symbols_are_exported(H):
    import quant_gemm
    import quant_gemm._lib as L
    import quant_gemm.ggml as G
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (qg_\w+)", nm))
    assert {"qg_gemm_w4a8_moe", "qg_moe_config", "qg_mul_mat_id_from_view"} <= exported
    assert {"qg_gemm_w4a8_moe", "qg_moe_config", "qg_mul_mat_id_from_view"} <= set(L.SIGNATURES)
    assert "qg_gemm_w4a8_moe_cpu" in H.SIGNATURES and hasattr(H.load(), "qg_gemm_w4a8_moe_cpu")
    assert {"gemm_w4a8_moe", "moe_config"} <= set(quant_gemm.__all__)
    assert callable(G.mul_mat_id_from_ggml) and callable(H.gemm_w4a8_moe)


@pytest.mark.parametrize("kind", ["gemv", "mmq"])
@pytest.mark.parametrize("tag", ["q4k", "q6k"])
def test_kquant_body_exists_once_and_both_entries_include_it(tag, kind):
    """The body of each Q4_K / Q6_K kernel is one text, csrc/qg_<tag>_<kind>_body.inc, included by the shipped kernel
    and by its expert-indexed (gemv) / expert-grouped (mmq) twin: both files include it, and the lambda that defines
    the body occurs in no other file under csrc/, so the MoE entries cannot carry a copy of it."""
    import glob
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.cpp-quant-gemm_amd", "csrc")
    body = f"qg_{tag}_{kind}_body.inc"
    moe_file = {"gemv": "qg_moe.hip", "mmq": "qg_moe_prefill.hip"}[kind]
    for f in (f"qg_{tag}_{kind}.hip", moe_file):
        assert open(os.path.join(csrc, f)).read().count(f'#include "{body}"\n') == 1, f
    # the GEMV's marker carries the type's unit size (the row GEMV of the 32-element types has a do_unit of its own);
    # the prefill's is the same text in both types, so its holders are the two types' bodies
    marker = {"gemv": f"auto do_unit = [&](const uint32_t (&w)[{tag.upper()}_UNIT_DW]", "mmq": "auto load_weights = [&]"}[kind]
    want = {body: 1} if kind == "gemv" else {"qg_q4k_mmq_body.inc": 1, "qg_q6k_mmq_body.inc": 1}
    holders = {os.path.basename(f): open(f).read().count(marker) for f in glob.glob(os.path.join(csrc, "*")) if os.path.isfile(f)}
    assert {f: n for f, n in holders.items() if n} == want


def moe(so, A=4096, a_rows=1, B=4096, n_expert=4, ids=4096, ids_stride=2, C=4096, ldc=0, T=1, n_used=2, N=8, K=256, t=Q4_0):
    p = lambda v: None if v is None else P(v)
    return so.qg_gemm_w4a8_moe(p(A), a_rows, p(B), n_expert, p(ids), ids_stride, p(C), ldc, T, n_used, N, K, t, None)


def test_validation_codes_and_their_order(so):
    """Every call here is refused (or empty) before anything is enqueued: the pointers are never dereferenced."""
    # 1 negative size, before K
    for kw in ({"T": -1}, {"n_used": -1}, {"N": -1}):
        assert moe(so, K=33, t=9, **kw) == -1
    # 2 K granule, before the type: 32 for the block types, 256 for Q4_K / Q6_K
    assert moe(so, K=33, t=9) == -2 and moe(so, K=0) == -2 and moe(so, K=-256) == -2
    assert moe(so, K=288, t=Q4_K, B=4096) == -2 and moe(so, K=4128, t=Q6_K) == -2
    # 3 type, before empty
    for t in (9, 0, 1, 5, 13, 26):
        assert moe(so, K=256, t=t, T=0, A=None) == -3
    # 4 empty: nothing touched, whatever the rest is
    for kw in ({"T": 0}, {"n_used": 0}, {"N": 0}):
        assert moe(so, A=None, B=None, ids=None, C=None, a_rows=7, n_expert=0, ids_stride=-3, ldc=-1, **kw) == 0
    # 5 null pointer, before alignment
    for kw in ({"A": None}, {"B": None}, {"ids": None}, {"C": None}):
        other = {"B": 4097} if "B" not in kw else {"A": 4098}
        assert moe(so, **kw, **other) == -1
    # 6 alignment: A and ids 4 B; B 4 B (32-element types), 16 B (Q4_K), 2 B (Q6_K); before the entry's own checks
    assert moe(so, A=4098, a_rows=3) == -4 and moe(so, ids=4098, n_expert=0) == -4
    for t in ROW_TYPES:
        assert moe(so, B=4098, t=t, ldc=3) == -4
    assert moe(so, B=4104, t=Q4_K) == -4 and moe(so, B=4100, t=Q4_K) == -4
    assert moe(so, B=4097, t=Q6_K) == -4
    assert moe(so, B=4098, t=Q6_K, a_rows=3) == -1  # 2 B is enough for Q6_K: on to the entry's checks
    # the entry's own: INVALID_ARG
    assert moe(so, a_rows=3) == -1 and moe(so, a_rows=0) == -1 and moe(so, a_rows=-1) == -1
    assert moe(so, ids_stride=1) == -1 and moe(so, ids_stride=-1) == -1
    assert moe(so, n_expert=0) == -1 and moe(so, n_expert=-2) == -1
    assert moe(so, ldc=7) == -1 and moe(so, ldc=-8) == -1
    # ... before the unsupported shapes
    assert moe(so, K=4128, a_rows=3) == -1
    assert moe(so, K=4128) == -3                                           # odd K/32
    assert moe(so, T=8192, n_used=8, ids_stride=8, a_rows=8) == -3         # 65536 slots
    assert moe(so, T=65536, n_used=1, ids_stride=1) == -3


def moe_cfg(so, T, n_used, N, K, t):
    buf = ctypes.create_string_buffer(256)
    rc = so.qg_moe_config(T, n_used, N, K, t, buf, 256)
    return rc, buf.value.decode()


def test_moe_config_arguments(so):
    assert so.qg_moe_config(1, 1, 8, 256, Q4_0, None, 0) == -1
    assert moe_cfg(so, -1, 1, 8, 33, Q4_0)[0] == -1 and moe_cfg(so, 1, 1, 8, 33, Q4_0)[0] == -2
    assert moe_cfg(so, 1, 1, 8, 256, 9)[0] == -3
    assert moe_cfg(so, 0, 2, 8, 256, Q4_0) == (0, "")


@pytest.mark.parametrize("t", ALL_TYPES)
@pytest.mark.parametrize("k", CONFIG_K)
def test_moe_config_names_the_single_calls_kernel(so, t, k):
    """The family and LPR / BPL / ONE(U) of qg_debug_config(1, N, K, t); N = 20000 takes the single call's 512-thread
    N >= 16384 rule, which changes neither."""
    import quant_gemm as qg
    for n in (1, 300, 4096, 20000):
        rc, cfg = moe_cfg(so, 3, 2, n, k, t)
        assert rc == 0 and cfg.startswith("moe:"), (rc, cfg)
        single = qg.debug_config(1, n, k, t)
        assert MR.kernel_choice(cfg) == MR.kernel_choice(single), (cfg, single)
        assert MR.cfg_fields(single)[1]["MT"] == "1"
        fam, f = MR.cfg_fields(cfg)
        assert f["grid"].endswith("x6"), cfg  # the slot is grid.y
        assert qg.moe_config(3, 2, n, k, t) == cfg


@pytest.mark.parametrize("t", ROW_TYPES)
def test_moe_config_refuses_where_auto_leaves_the_gemv(so, t):
    import quant_gemm as qg
    for k in (4128, 32, 96, 4096 + 32):
        assert not qg.debug_config(1, 64, k, t).startswith("gemv "), k
        assert moe_cfg(so, 1, 2, 64, k, t) == (-3, "")
    for k in (64, 4096 + 64):
        assert qg.debug_config(1, 64, k, t).startswith("gemv ") and moe_cfg(so, 1, 2, 64, k, t)[0] == 0
    # the records of one activation row past 160 KiB (112 bytes per 64 elements)
    kmax = (160 * 1024 // 112) * 64
    assert moe_cfg(so, 1, 2, 64, kmax, t)[0] == 0 and moe_cfg(so, 1, 2, 64, kmax + 64, t) == (-3, "")


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
def test_moe_config_refuses_beyond_the_lds_records(so, t):
    """The first K whose records exceed 160 KiB: AUTO at M = 1 leaves the decode GEMV there, and so does the entry."""
    import quant_gemm as qg
    fam = "q4k_gemv" if t == Q4_K else "q6k_gemv"
    k0 = (160 * 1024 // MR.KQ_REC_BYTES[t] + 1) * 256
    assert qg.debug_config(1, 8, k0 - 256, t).startswith(fam + " ")
    assert not qg.debug_config(1, 8, k0, t).startswith(fam + " ")
    rc, cfg = moe_cfg(so, 2, 2, 8, k0 - 256, t)
    assert rc == 0 and cfg.startswith("moe:" + fam + " ") and f" lds={(k0 - 256) // 256 * MR.KQ_REC_BYTES[t]}" in cfg
    assert moe_cfg(so, 2, 2, 8, k0, t) == (-3, "")


def test_moe_config_slot_limit(so):
    assert moe_cfg(so, 65535, 1, 8, 256, Q4_0)[0] == 0 and moe_cfg(so, 13107, 5, 8, 256, Q4_K)[0] == 0
    assert moe_cfg(so, 65536, 1, 8, 256, Q4_0) == (-3, "")
    assert moe_cfg(so, 8192, 8, 8, 256, Q6_K) == (-3, "")
    assert moe_cfg(so, 2 ** 30, 2 ** 30, 8, 256, Q8_0) == (-3, "")


# ---------------------------------------------------------------------------- the host twin
def host_case(t, a_rows, seed=0):
    T, n_used, n_expert, n, k = 3, 2, 4, 5, 512
    rng = np.random.default_rng([t, a_rows, seed])
    w = MR.random_experts(rng, t, n_expert, n, k)
    a = MR.random_act(rng, T * a_rows, k).reshape(T, a_rows, k // 32, 36)
    ids = rng.integers(0, n_expert, (T, n_expert)).astype(np.int32)  # row stride n_expert > n_used
    ids[0, :2] = (3, 3)        # repeated inside a token
    ids[2, 0] = ids[1, 0]      # repeated across tokens
    ids[1, 1] = -1
    ids[2, 1] = n_expert
    return T, n_used, n_expert, n, k, w, a, ids


@pytest.mark.parametrize("t", ALL_TYPES)
@pytest.mark.parametrize("a_rows", [1, 2])
def test_host_twin_equals_the_single_call_per_slot(H, O, t, a_rows):
    T, n_used, n_expert, n, k, w, a, ids = host_case(t, a_rows)
    c = H.gemm_w4a8_moe(a, w, ids, T, n_used, n, k, t, a_rows=a_rows, threads=1)
    assert c.shape == (T, n_used, n)
    for threads in (2, 7):
        c2 = H.gemm_w4a8_moe(a, w, ids, T, n_used, n, k, t, a_rows=a_rows, threads=threads)
        assert np.array_equal(c.view(np.uint32), c2.view(np.uint32))
    for tt in range(T):
        for u in range(n_used):
            e = int(ids[tt, u])
            if not 0 <= e < n_expert:
                assert (c[tt, u].view(np.uint32) == 0).all()  # +0.0f
                continue
            row = a[tt, u % a_rows]
            want = H.gemm_w4a8(row[None], w[e], 1, n, k, t, threads=1)[0]
            assert np.array_equal(c[tt, u].view(np.uint32), want.view(np.uint32)), (tt, u)
            MR.assert_close_to_model(O, c[tt, u], row, w[e], t)
    assert (c[1, 1] == 0).all() and (c[2, 1] == 0).all() and np.abs(c[0]).min() > 0


def test_host_twin_strided_output_and_codes(H):
    T, n_used, n_expert, n, k, w, a, ids = host_case(Q8_0, 1)
    dense = H.gemm_w4a8_moe(a, w, ids, T, n_used, n, k, Q8_0)
    ldc = n + 3
    buf = np.full((T * n_used + 2, ldc), -7.0, np.float32)
    fn = H.load().qg_gemm_w4a8_moe_cpu
    p = lambda x: P(x.ctypes.data)
    args = lambda **kw: dict(dict(A=p(a), a_rows=1, B=p(w), n_expert=n_expert, ids=p(ids), ids_stride=n_expert,
                                  C=P(buf.ctypes.data + 4 * ldc), ldc=ldc, T=T, n_used=n_used, N=n, K=k, t=Q8_0, threads=2), **kw)
    call = lambda **kw: fn(*args(**kw).values())
    assert call() == 0
    assert np.array_equal(buf[1:-1, :n].reshape(T, n_used, n).view(np.uint32), dense.view(np.uint32))
    assert (buf[0] == -7.0).all() and (buf[-1] == -7.0).all() and (buf[:, n:] == -7.0).all()
    assert call(T=-1, K=33) == -1 and call(K=33, t=9) == -2 and call(t=9, T=0) == -3 and call(K=288, t=Q4_K) == -2
    assert call(T=0, A=None, a_rows=9) == 0 and call(A=None) == -1
    assert call(a_rows=3) == -1 and call(ids_stride=1) == -1 and call(n_expert=0) == -1 and call(ldc=n - 1) == -1
