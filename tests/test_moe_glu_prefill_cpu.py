"""qg_gemm_w4a8_moe_glu_prefill without a GPU: the exported symbols, the validation codes and their order (on fake
pointers that every call refuses before a launch) and qg_moe_glu_prefill_config against qg_moe_prefill_config."""
import ctypes
import itertools
import re
import subprocess

import pytest

import moe_ref as MR
from moe_ref import Q4_K, Q6_K, ROW_TYPES

P = ctypes.c_void_p
BIG, MAX_EXPERTS, SWIGLU = 1 << 40, 4096, 2  # a workspace_bytes that is never too small; qg.h


@pytest.fixture(scope="module")
def so():
    import quant_gemm._lib as L
    return L.load()


def test_new_symbols_are_exported():
    import quant_gemm
    import quant_gemm._lib as L
    import quant_gemm.ggml as G
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r" T (qg_\w+)", nm))
    new = {"qg_gemm_w4a8_moe_glu_prefill", "qg_moe_glu_prefill_config", "qg_mul_mat_id_glu_from_view_ws"}
    assert new <= exported and new <= set(L.SIGNATURES) and callable(G.mul_mat_id_glu_from_ggml_ws)
    assert {"gemm_w4a8_moe_glu_prefill", "moe_glu_prefill_config"} <= set(quant_gemm.__all__)
    header = open(L.LIB_PATH.replace("llama.cpp-quant-gemm_amd/quant_gemm/libqg_hip.so", "include/qg/qg.h")).read()
    for s in new:
        assert re.search(rf"\b{s}\(", header), s


def glu(so, A=4096, Bg=4096, Bu=8192, n_expert=4, ids=4096, ids_stride=2, C=4096, ldc=0, T=1, n_used=2, N=8, K=256, t=Q4_K,
        op=SWIGLU, ws=4096, ws_bytes=BIG):
    p = lambda v: None if v is None else P(v)
    return so.qg_gemm_w4a8_moe_glu_prefill(p(A), p(Bg), p(Bu), n_expert, p(ids), ids_stride, p(C), ldc, T, n_used, N, K, t, op,
                                           p(ws), ws_bytes, None)


def test_validation_codes_and_their_order(so):
    """Every call here is refused (or empty) before anything is enqueued: the pointers are never dereferenced."""
    size = so.qg_gemm_w4a8_moe_prefill_workspace_size
    # negative sizes, then the K granule (256 for Q4_K / Q6_K, 32 for a type the entry does not take), then the type
    assert all(glu(so, K=33, t=9, **kw) == -1 for kw in ({"T": -1}, {"n_used": -1}, {"N": -1}))
    assert all(glu(so, **kw) == -2 for kw in ({"K": 33, "t": 9}, {"K": 0}, {"K": -256}, {"K": 288}, {"K": 4128, "t": Q6_K}))
    for t in ROW_TYPES + (9, 11, 13, 23, 26, 39, 0, 1, 5):
        assert glu(so, K=256, t=t, T=0, A=None) == -3 and glu(so, K=288, t=t) == -3
    # empty: nothing touched, whatever the rest is -- a null workspace and an unknown op included
    for kw in ({"T": 0}, {"n_used": 0}, {"N": 0}):
        assert glu(so, A=None, Bg=None, Bu=None, ids=None, C=None, n_expert=0, ids_stride=-3, ldc=-1, ws=None, ws_bytes=0,
                   op=7, **kw) == 0
    # null pointers, then alignment: A and ids 4 B; both weight pointers 16 B (Q4_K), 2 B (Q6_K)
    for kw in ({"A": None}, {"Bg": None}, {"Bu": None}, {"ids": None}, {"C": None}):
        assert glu(so, **kw, **({"Bg": 4097} if "Bg" not in kw else {"A": 4098})) == -1
    assert glu(so, A=4098, n_expert=0) == -4 and glu(so, ids=4098, n_expert=0) == -4
    assert all(glu(so, **kw) == -4 for kw in ({"Bg": 4104}, {"Bu": 4104}, {"Bg": 4097, "t": Q6_K}, {"Bu": 4097, "t": Q6_K}))
    assert glu(so, Bg=4098, Bu=4102, t=Q6_K, n_expert=0) == -1  # 2 B is enough for Q6_K: on to the entry's checks
    # ids_stride, n_expert, ldc: INVALID_ARG, before the workspace
    assert glu(so, ids_stride=1, ws=4100) == -1 and glu(so, n_expert=0, ws=4100) == -1 and glu(so, n_expert=-2) == -1
    assert glu(so, ldc=7, ws=4100) == -1 and glu(so, ldc=-8) == -1
    # the workspace: null, then its alignment, then its size -- before the unsupported shapes and the op
    need = size(1, 2, 4)
    assert need > 0 and glu(so, ws=None, op=1) == -1
    assert all(glu(so, ws=4096 + off, ws_bytes=0, op=1) == -4 for off in (1, 2, 4, 8))
    assert glu(so, ws_bytes=need - 1, op=1) == -1 and glu(so, ws_bytes=0) == -1
    big = dict(T=8192, n_used=8, ids_stride=8)  # 65536 slots
    assert glu(so, ws=None, **big) == -1 and glu(so, ws=4100, **big) == -4
    assert glu(so, ws_bytes=size(8192, 8, 4) - 1, **big) == -1 and glu(so, ws_bytes=size(8192, 8, 4), **big) == -3
    assert glu(so, T=65536, n_used=1, ids_stride=1) == -3 and glu(so, n_expert=MAX_EXPERTS + 1) == -3
    assert glu(so, n_expert=MAX_EXPERTS + 1, ws_bytes=size(1, 2, MAX_EXPERTS + 1) - 1, op=1) == -1
    # the op, last: after everything above has passed, with exactly the workspace the size function names
    for op in (1, 3, 4, -1, 7):
        assert glu(so, op=op, ws_bytes=need) == -3
        assert glu(so, op=op, ws_bytes=need - 1) == -1 and glu(so, op=op, ldc=7) == -1 and glu(so, op=op, Bu=4104) == -4


def cfg(so, T, n_used, n_expert, N, K, t, sym="qg_moe_glu_prefill_config"):
    buf = ctypes.create_string_buffer(256)
    return getattr(so, sym)(T, n_used, n_expert, N, K, t, buf, 256), buf.value.decode()


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
def test_config_follows_the_prefill_entrys_rg(so, t):
    """RG and KS are those of qg_moe_prefill_config for the shape, over shapes that reach its four forms (and Q6_K's
    rule at K <= 1024); R = 16 TT and grid = ceil(N / 16 RG) x moe_max_tiles(slots, n_expert, R)."""
    seen, shapes = set(), list(itertools.product((1, 7, 33, 200, 4096), (1, 2, 8), (1, 3, 8, 130, 1024), (1, 65, 8129, 14336), (1280,)))
    shapes += [(T, 2, e, 129, K) for K in (256, 768, 1024) for T, e in ((1, 8), (33, 3), (4096, 1))]
    for T, n_used, n_expert, N, K in shapes:
        rc, s = cfg(so, T, n_used, n_expert, N, K, t)
        rc0, s0 = cfg(so, T, n_used, n_expert, N, K, t, "qg_moe_prefill_config")
        assert rc == 0 and rc0 == 0, (T, n_used, n_expert, N, K, s, s0)
        (fam, f), (fam0, f0) = MR.cfg_fields(s), MR.cfg_fields(s0)
        assert s.startswith("moe_glu:") and fam == fam0 == ("q4k_mmq" if t == Q4_K else "q6k_mmq")
        assert (f["RG"], f["KS"]) == (f0["RG"], f0["KS"]), (s, s0)
        tt, rg, r, slots = int(f["TT"]), int(f["RG"]), int(f["R"]), T * n_used
        assert tt in (1, 2, 4) and tt <= int(f0["TT"]) and r == 16 * tt and int(f["KS"]) == 8 // rg
        assert f["grid"] == f"{-(-N // (16 * rg))}x{slots // r + min(n_expert + 1, slots)}", s
        seen.add((int(f0["TT"]), rg))
    assert seen == {(1, 1), (2, 1), (4, 1), (4, 4)}
