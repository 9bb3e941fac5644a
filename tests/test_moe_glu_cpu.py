"""qg_gemm_w4a8_moe_glu without a GPU: the exported symbols, the validation codes and their order (on fake pointers
that every call refuses before a launch), qg_moe_glu_config against qg_moe_config, the kernel file's includes of the
two decode GEMV bodies, and the host twin qg_gemm_w4a8_moe_glu_cpu against the two ops applied to the g and u of
qg_gemm_w4a8_moe_cpu (ReGLU: bits; SwiGLU: the bound of moe_glu_ref.swiglu_tol)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import moe_glu_ref as GR
import moe_ref as MR
from moe_glu_ref import REGLU, SWIGLU, bits
from moe_ref import Q4_K, Q6_K, ROW_TYPES

P = ctypes.c_void_p
CONFIG_K = (256, 512, 1024, 2304, 4096, 4352)  # 512: LPR = 4 with the unit loop (super-block types)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.cpp-quant-gemm_amd", "csrc")


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
    new = {"qg_gemm_w4a8_moe_glu", "qg_moe_glu_config", "qg_mul_mat_id_glu_from_view"}
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert new <= set(re.findall(r" T (qg_\w+)", nm)) and new <= set(L.SIGNATURES)
    nm = subprocess.run(["nm", "-D", "--defined-only", H.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "qg_gemm_w4a8_moe_glu_cpu" in set(re.findall(r" T (qg_\w+)", nm))
    assert "qg_gemm_w4a8_moe_glu_cpu" in H.SIGNATURES and hasattr(H.load(), "qg_gemm_w4a8_moe_glu_cpu")
    assert {"gemm_w4a8_moe_glu", "moe_glu_config", "GLU_REGLU", "GLU_SWIGLU"} <= set(quant_gemm.__all__)
    assert (quant_gemm.GLU_REGLU, quant_gemm.GLU_SWIGLU) == (0, 2) == (H.GLU_REGLU, H.GLU_SWIGLU)
    assert callable(quant_gemm.gemm_w4a8_moe_glu) and callable(G.mul_mat_id_glu_from_ggml) and callable(H.gemm_w4a8_moe_glu)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "qg", "qg.h")).read()
    assert re.search(r"#define QG_GLU_REGLU\s+0\b", hdr) and re.search(r"#define QG_GLU_SWIGLU\s+2\b", hdr)


@pytest.mark.parametrize("tag", ["q4k", "q6k"])
def test_kernel_file_includes_the_decode_body(tag):
    """qg_moe_glu.hip runs the decode GEMV's own text (the gate pass and the up pass call one function that includes it)
    and carries no copy of it; it is built into the library."""
    text = open(os.path.join(CSRC, "qg_moe_glu.hip")).read()
    assert text.count(f'#include "qg_{tag}_gemv_body.inc"\n') >= 1
    assert "auto do_unit" not in text and "auto load_unit" not in text
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert " qg_moe_glu.hip " in mk and " qg_moe_glu.hpp " in mk


# ---------------------------------------------------------------------------- validation
def glu(so, A=4096, Bg=4096, Bu=8192, n_expert=4, ids=4096, ids_stride=2, C=4096, ldc=0, T=1, n_used=2, N=8, K=256, t=Q4_K,
        op=SWIGLU):
    p = lambda v: None if v is None else P(v)
    return so.qg_gemm_w4a8_moe_glu(p(A), p(Bg), p(Bu), n_expert, p(ids), ids_stride, p(C), ldc, T, n_used, N, K, t, op, None)


def test_validation_codes_and_their_order(so):
    """Every call here is refused (or empty) before anything is enqueued: the pointers are never dereferenced."""
    # 1 negative size, before K
    for kw in ({"T": -1}, {"n_used": -1}, {"N": -1}):
        assert glu(so, K=33, t=9, **kw) == -1
    # 2 K granule, before the type: 256 for Q4_K / Q6_K, 32 for every other type id
    assert glu(so, K=33, t=9) == -2 and glu(so, K=0) == -2 and glu(so, K=-256) == -2
    assert glu(so, K=288, t=Q4_K) == -2 and glu(so, K=4128, t=Q6_K) == -2 and glu(so, K=33, t=ROW_TYPES[0]) == -2
    # 3 type, before the empty call: the five 32-element types are none of this entry's
    for t in ROW_TYPES + (9, 13, 26, 0, 1, 5):
        assert glu(so, K=256, t=t, T=0, A=None) == -3, t
        assert glu(so, K=256, t=t) == -3, t
    # 4 empty: nothing touched, whatever the rest is (a glu_op the entry does not have among it)
    for kw in ({"T": 0}, {"n_used": 0}, {"N": 0}):
        for t in (Q4_K, Q6_K):
            assert glu(so, A=None, Bg=None, Bu=None, ids=None, C=None, n_expert=0, ids_stride=-3, ldc=-1, op=1, t=t, **kw) == 0
    # 5 null pointer, before alignment
    for kw in ({"A": None}, {"Bg": None}, {"Bu": None}, {"ids": None}, {"C": None}):
        other = {"Bg": 4097} if "Bg" not in kw else {"A": 4098}
        assert glu(so, **kw, **other) == -1, kw
    # 6 alignment: A and ids 4 B; B_gate and B_up alike 16 B (Q4_K), 2 B (Q6_K); before the entry's own checks
    assert glu(so, A=4098, n_expert=0) == -4 and glu(so, ids=4098, n_expert=0) == -4
    for kw in ({"Bg": 4104}, {"Bg": 4100}, {"Bu": 4104}, {"Bu": 4100}, {"Bu": 4098}):
        assert glu(so, t=Q4_K, ldc=3, op=1, **kw) == -4, kw
    assert glu(so, Bg=4097, t=Q6_K, op=1) == -4 and glu(so, Bu=4097, t=Q6_K, op=1) == -4
    assert glu(so, Bu=4098, t=Q6_K, ids_stride=1) == -1 and glu(so, Bg=4098, Bu=4102, t=Q6_K, ids_stride=1) == -1  # 4n + 2 is enough
    # the arguments: INVALID_ARG, before the glu_op and the unsupported shapes
    for op in (SWIGLU, REGLU, 1):
        assert glu(so, ids_stride=1, op=op) == -1 and glu(so, ids_stride=-1, op=op) == -1
        assert glu(so, n_expert=0, op=op) == -1 and glu(so, n_expert=-2, op=op) == -1
        assert glu(so, ldc=7, op=op) == -1 and glu(so, ldc=-8, op=op) == -1
        assert glu(so, ldc=7, T=65536, n_used=1, ids_stride=1, op=op) == -1
    # the entry's own refusals, all UNSUPPORTED with nothing launched
    for op in (1, 3, -1, 4, 2 ** 31 - 1):
        for t in (Q4_K, Q6_K):
            assert glu(so, op=op, t=t) == -3, op
    for op in (SWIGLU, REGLU):
        assert glu(so, T=8192, n_used=8, ids_stride=8, op=op) == -3        # 65536 slots
        assert glu(so, T=65536, n_used=1, ids_stride=1, op=op) == -3
        for t in (Q4_K, Q6_K):                                             # the LDS records beyond 160 KiB: off the GEMV
            k0 = (160 * 1024 // MR.KQ_REC_BYTES[t] + 1) * 256
            assert glu(so, K=k0, t=t, op=op) == -3


# ---------------------------------------------------------------------------- the config line
def glu_cfg(so, T, n_used, N, K, t):
    buf = ctypes.create_string_buffer(256)
    rc = so.qg_moe_glu_config(T, n_used, N, K, t, buf, 256)
    return rc, buf.value.decode()


def moe_cfg(so, T, n_used, N, K, t):
    buf = ctypes.create_string_buffer(256)
    rc = so.qg_moe_config(T, n_used, N, K, t, buf, 256)
    return rc, buf.value.decode()


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
@pytest.mark.parametrize("k", CONFIG_K)
def test_glu_config_names_the_decode_entrys_launch(so, t, k):
    import quant_gemm as qg
    fam = "q4k_gemv" if t == Q4_K else "q6k_gemv"
    for n in (1, 300, 4096, 20000):
        rc, cfg = glu_cfg(so, 3, 2, n, k, t)
        assert rc == 0 and cfg.startswith(f"moe_glu:{fam} "), (rc, cfg)
        rc2, ref = moe_cfg(so, 3, 2, n, k, t)
        assert rc2 == 0 and ref.startswith(f"moe:{fam} ")
        assert cfg.split(" ")[1:] == ref.split(" ")[1:], (cfg, ref)  # LPR, WGS, ONE, grid, lds
        f = MR.cfg_fields(cfg)[1]
        assert set(f) == {"LPR", "WGS", "ONE", "grid", "lds"} and f["grid"].endswith("x6")
        assert qg.moe_glu_config(3, 2, n, k, t) == cfg


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
@pytest.mark.parametrize("k", CONFIG_K)
def test_glu_config_names_the_single_calls_kernel(so, t, k):
    """The family and LPR / ONE of qg_debug_config(1, N, K, t): each pass of a slot runs the single M = 1 call's
    instantiation."""
    import quant_gemm as qg
    for n in (1, 300, 4096):
        rc, cfg = glu_cfg(so, 3, 2, n, k, t)
        single = qg.debug_config(1, n, k, t)
        assert rc == 0 and MR.kernel_choice(cfg) == MR.kernel_choice(single), (cfg, single)
        assert MR.cfg_fields(single)[1]["MT"] == "1"


def test_glu_config_codes(so):
    assert so.qg_moe_glu_config(1, 1, 8, 256, Q4_K, None, 0) == -1
    assert glu_cfg(so, -1, 1, 8, 33, Q4_K)[0] == -1 and glu_cfg(so, 1, 1, 8, 288, Q4_K)[0] == -2
    for t in ROW_TYPES + (9,):
        assert glu_cfg(so, 1, 1, 8, 256, t) == (-3, "")
    assert glu_cfg(so, 0, 2, 8, 256, Q6_K) == (0, "")
    assert glu_cfg(so, 65535, 1, 8, 256, Q4_K)[0] == 0 and glu_cfg(so, 65536, 1, 8, 256, Q4_K) == (-3, "")
    for t in (Q4_K, Q6_K):
        k0 = (160 * 1024 // MR.KQ_REC_BYTES[t] + 1) * 256
        rc, cfg = glu_cfg(so, 2, 2, 8, k0 - 256, t)
        assert rc == 0 and f" lds={(k0 - 256) // 256 * MR.KQ_REC_BYTES[t]}" in cfg
        assert glu_cfg(so, 2, 2, 8, k0, t) == (-3, "")


# ---------------------------------------------------------------------------- the host twin
def host_case(t, seed=0, scale=None):
    """Gate and up experts drawn one after the other from one generator (every expert different); ids with a row stride
    n_expert > n_used, repeated inside a token and across tokens, -1 and n_expert."""
    T, n_used, n_expert, n, k = 3, 2, 4, 7, 512
    rng = np.random.default_rng([t, seed, 17])
    gate, up = MR.random_experts(rng, t, n_expert, n, k), MR.random_experts(rng, t, n_expert, n, k)
    a = MR.random_act(rng, T, k)
    if scale is not None:  # d_a of every block: brings g into the range where silu bends
        a[..., 0:2] = np.ascontiguousarray(np.full(a.shape[:2], scale, np.float16)).view(np.uint8).reshape(a.shape[:2] + (2,))
    ids = rng.integers(0, n_expert, (T, n_expert)).astype(np.int32)
    ids[0, :2] = (3, 3)
    ids[2, 0] = ids[1, 0]
    ids[1, 1] = -1
    ids[2, 1] = n_expert
    return T, n_used, n_expert, n, k, gate, up, a, ids


def products(H, case, t):
    T, n_used, n_expert, n, k, gate, up, a, ids = case
    g = H.gemm_w4a8_moe(a, gate, ids, T, n_used, n, k, t, a_rows=1)
    u = H.gemm_w4a8_moe(a, up, ids, T, n_used, n, k, t, a_rows=1)
    assert not np.array_equal(bits(g), bits(u))
    return g, u


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
def test_host_twin_reglu_bits(H, t):
    case = host_case(t)
    T, n_used, n_expert, n, k, gate, up, a, ids = case
    g, u = products(H, case, t)
    c = H.gemm_w4a8_moe_glu(a, gate, up, ids, T, n_used, n, k, t, REGLU)
    assert c.shape == (T, n_used, n) and c.dtype == np.float32
    assert np.array_equal(bits(c), bits(GR.reglu(g, u)))
    assert (g > 0).any() and (g < 0).any() and (c != 0).any()
    # swapped operands give other bits; the same tensor twice gives relu(g) * g
    assert not np.array_equal(bits(H.gemm_w4a8_moe_glu(a, up, gate, ids, T, n_used, n, k, t, REGLU)), bits(c))
    assert np.array_equal(bits(H.gemm_w4a8_moe_glu(a, gate, gate, ids, T, n_used, n, k, t, REGLU)), bits(GR.reglu(g, g)))


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
@pytest.mark.parametrize("scale", [None, 2.0 ** -9, 2.0 ** -12])
def test_host_twin_swiglu_bound(H, t, scale):
    case = host_case(t, seed=1, scale=scale)
    T, n_used, n_expert, n, k, gate, up, a, ids = case
    g, u = products(H, case, t)
    c = H.gemm_w4a8_moe_glu(a, gate, up, ids, T, n_used, n, k, t, SWIGLU)
    print(f"g in [{g.min():.4g}, {g.max():.4g}]")
    GR.assert_swiglu(c, g, u, f"host t={t} scale={scale}")
    assert np.array_equal(bits(c), bits(H.gemm_w4a8_moe_glu(a, gate, up, ids, T, n_used, n, k, t)))  # the default op


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
@pytest.mark.parametrize("op", [REGLU, SWIGLU])
def test_host_twin_out_of_range_ids_and_threads(H, t, op):
    T, n_used, n_expert, n, k, gate, up, a, ids = host_case(t, seed=2)
    c = H.gemm_w4a8_moe_glu(a, gate, up, ids, T, n_used, n, k, t, op, threads=1)
    assert (bits(c[1, 1]) == 0).all() and (bits(c[2, 1]) == 0).all()  # +0.0f
    assert np.abs(c[0]).max() > 0
    for threads in (2, 7):
        assert np.array_equal(bits(c), bits(H.gemm_w4a8_moe_glu(a, gate, up, ids, T, n_used, n, k, t, op, threads=threads)))


def test_host_twin_strided_output_and_codes(H):
    t = Q4_K
    T, n_used, n_expert, n, k, gate, up, a, ids = host_case(t, seed=3)
    dense = H.gemm_w4a8_moe_glu(a, gate, up, ids, T, n_used, n, k, t, REGLU)
    ldc = n + 3
    buf = np.full((T * n_used + 2, ldc), -7.0, np.float32)
    fn = H.load().qg_gemm_w4a8_moe_glu_cpu
    p = lambda x: P(x.ctypes.data)
    args = lambda **kw: dict(dict(A=p(a), Bg=p(gate), Bu=p(up), n_expert=n_expert, ids=p(ids), ids_stride=n_expert,
                                  C=P(buf.ctypes.data + 4 * ldc), ldc=ldc, T=T, n_used=n_used, N=n, K=k, t=t, op=REGLU,
                                  threads=2), **kw)
    call = lambda **kw: fn(*args(**kw).values())
    assert call() == 0
    assert np.array_equal(bits(buf[1:-1, :n].reshape(T, n_used, n)), bits(dense))
    assert (buf[0] == -7.0).all() and (buf[-1] == -7.0).all() and (buf[:, n:] == -7.0).all()
    assert call(T=-1, K=33) == -1 and call(K=33, t=9) == -2 and call(K=288) == -2
    assert call(t=9, T=0) == -3 and call(t=2) == -3 and call(t=8, T=0) == -3
    assert call(T=0, A=None, op=1) == 0
    assert call(A=None) == -1 and call(Bg=None) == -1 and call(Bu=None) == -1 and call(ids=None) == -1 and call(C=None) == -1
    assert call(ids_stride=1, op=1) == -1 and call(n_expert=0) == -1 and call(ldc=n - 1) == -1 and call(ldc=-1) == -1
    assert call(op=1) == -3 and call(op=3) == -3 and call(op=-1) == -3
