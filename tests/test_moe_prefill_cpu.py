"""qg_gemm_w4a8_moe_prefill without a GPU: the exported symbols, the validation codes and their order (on fake
pointers that every call refuses before a launch), qg_moe_prefill_config (refusals, the grid's upper bound, the
form rule) and the workspace size function."""
import ctypes
import re
import subprocess

import pytest

import moe_ref as MR
from moe_ref import Q4_K, Q6_K, ROW_TYPES

P = ctypes.c_void_p
BIG = 1 << 40  # a workspace_bytes that is never too small
MAX_EXPERTS, MAX_SLOTS, WS_ALIGN = 4096, 65535, 16  # qg.h


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
    new = {"qg_gemm_w4a8_moe_prefill", "qg_gemm_w4a8_moe_prefill_workspace_size", "qg_moe_prefill_config",
           "qg_debug_moe_prefill_plan", "qg_mul_mat_id_from_view_ws"}
    assert new <= exported and new <= set(L.SIGNATURES)
    assert {"gemm_w4a8_moe_prefill", "moe_prefill_workspace_size", "moe_prefill_config"} <= set(quant_gemm.__all__)
    assert callable(G.mul_mat_id_from_ggml_ws)
    header = open(L.LIB_PATH.replace("llama.cpp-quant-gemm_amd/quant_gemm/libqg_hip.so", "include/qg/qg.h")).read()
    for s in new:
        assert re.search(rf"\b{s}\(", header), s


def pre(so, A=4096, a_rows=1, B=4096, n_expert=4, ids=4096, ids_stride=2, C=4096, ldc=0, T=1, n_used=2, N=8, K=256, t=Q4_K,
        ws=4096, ws_bytes=BIG):
    p = lambda v: None if v is None else P(v)
    return so.qg_gemm_w4a8_moe_prefill(p(A), a_rows, p(B), n_expert, p(ids), ids_stride, p(C), ldc, T, n_used, N, K, t,
                                       p(ws), ws_bytes, None)


def test_validation_codes_and_their_order(so):
    """Every call here is refused (or empty) before anything is enqueued: the pointers are never dereferenced."""
    size = so.qg_gemm_w4a8_moe_prefill_workspace_size
    # 1 negative size, before K
    for kw in ({"T": -1}, {"n_used": -1}, {"N": -1}):
        assert pre(so, K=33, t=9, **kw) == -1
    # 2 K granule, before the type: 256 for Q4_K / Q6_K, 32 for a type the entry does not take
    assert pre(so, K=33, t=9) == -2 and pre(so, K=0) == -2 and pre(so, K=-256) == -2
    assert pre(so, K=288, t=Q4_K) == -2 and pre(so, K=4128, t=Q6_K) == -2
    # 3 type, before empty: the five row types are refused here, and so is everything that is no weight type
    for t in ROW_TYPES + (9, 0, 1, 5, 13, 26):
        assert pre(so, K=256, t=t, T=0, A=None) == -3
        assert pre(so, K=288, t=t) == -3
    # 4 empty: nothing touched, whatever the rest is -- a null workspace included
    for kw in ({"T": 0}, {"n_used": 0}, {"N": 0}):
        assert pre(so, A=None, B=None, ids=None, C=None, a_rows=7, n_expert=0, ids_stride=-3, ldc=-1, ws=None, ws_bytes=0,
                   **kw) == 0
    # 5 null pointer, before alignment
    for kw in ({"A": None}, {"B": None}, {"ids": None}, {"C": None}):
        other = {"B": 4097} if "B" not in kw else {"A": 4098}
        assert pre(so, **kw, **other) == -1
    # 6 alignment: A and ids 4 B; B 16 B (Q4_K), 2 B (Q6_K); before the entry's own checks
    assert pre(so, A=4098, a_rows=3) == -4 and pre(so, ids=4098, n_expert=0) == -4
    assert pre(so, B=4104, t=Q4_K) == -4 and pre(so, B=4097, t=Q6_K) == -4
    assert pre(so, B=4098, t=Q6_K, a_rows=3) == -1  # 2 B is enough for Q6_K: on to the entry's checks
    # 7 the entry's own: INVALID_ARG, before the workspace
    assert pre(so, a_rows=3, ws=None) == -1 and pre(so, a_rows=0, ws=4100) == -1
    assert pre(so, ids_stride=1, ws=4100) == -1 and pre(so, n_expert=0, ws=4100) == -1 and pre(so, n_expert=-2) == -1
    assert pre(so, ldc=7, ws=4100) == -1 and pre(so, ldc=-8) == -1
    # 8 the workspace: null, then its alignment, then its size -- before the unsupported shapes
    need = size(1, 2, 4)
    assert need > 0
    assert pre(so, ws=None) == -1
    for off in (1, 2, 4, 8):
        assert pre(so, ws=4096 + off, ws_bytes=0) == -4
    assert pre(so, ws_bytes=need - 1) == -1
    assert pre(so, ws_bytes=0) == -1
    assert pre(so, T=8192, n_used=8, ids_stride=8, ws=None) == -1
    assert pre(so, T=8192, n_used=8, ids_stride=8, ws=4100) == -4
    assert pre(so, T=8192, n_used=8, ids_stride=8, ws_bytes=size(8192, 8, 4) - 1) == -1
    # 9 the unsupported shapes
    assert pre(so, T=8192, n_used=8, ids_stride=8, ws_bytes=size(8192, 8, 4)) == -3       # 65536 slots
    assert pre(so, T=65536, n_used=1, ids_stride=1) == -3
    assert pre(so, n_expert=MAX_EXPERTS + 1) == -3
    assert pre(so, n_expert=MAX_EXPERTS + 1, ws_bytes=size(1, 2, MAX_EXPERTS + 1) - 1) == -1


def cfg(so, T, n_used, n_expert, N, K, t):
    buf = ctypes.create_string_buffer(256)
    rc = so.qg_moe_prefill_config(T, n_used, n_expert, N, K, t, buf, 256)
    return rc, buf.value.decode()


def test_config_arguments_and_refusals(so):
    assert so.qg_moe_prefill_config(1, 1, 4, 8, 256, Q4_K, None, 0) == -1
    assert cfg(so, -1, 1, 4, 8, 33, Q4_K)[0] == -1 and cfg(so, 1, 1, 4, 8, 288, Q4_K)[0] == -2
    for t in ROW_TYPES + (9,):
        assert cfg(so, 4, 2, 4, 8, 256, t) == (-3, "")
    assert cfg(so, 0, 2, 4, 8, 256, Q4_K) == (0, "")
    assert cfg(so, 4, 2, 0, 8, 256, Q4_K)[0] == -1
    assert cfg(so, 65536, 1, 4, 8, 256, Q6_K)[0] == -3 and cfg(so, 4, 2, MAX_EXPERTS + 1, 8, 256, Q6_K)[0] == -3
    assert cfg(so, 65535, 1, MAX_EXPERTS, 8, 256, Q6_K)[0] == 0
    assert cfg(so, 8, 128, 1024, 8, 256, Q4_K)[0] == 0  # 1024 experts are served


FORMS = {(1, 1), (2, 1), (4, 1), (4, 4)}


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
def test_config_names_family_form_and_the_grids_upper_bound(so, t):
    """The string carries the family, TT, RG, KS = 8 / RG, R = 16 TT and grid = ceil(N / 16 RG) x (floor(slots / R) +
    min(n_expert + 1, slots)); the form follows slots / n_expert (rounded up): <= 16 rows (1, 1), <= 32 (2, 1), beyond
    (4, 4) where ceil(N / 64) ceil(slots / 64) fills the CUs (256 without a device), else (4, 1). Q6_K at K <= 1024
    takes (4, 4) whatever the slots are."""
    import itertools
    seen = set()
    for K in (256, 768, 1024):
        for T, n_expert in ((1, 8), (33, 3), (4096, 1)):
            assert ("TT=4 RG=4" in cfg(so, T, 2, n_expert, 129, K, t)[1]) == (t == Q6_K or T == 4096)
    for T, n_used, n_expert, N in itertools.product((1, 7, 33, 200, 4096), (1, 2, 8), (1, 3, 8, 130, 1024), (1, 65, 8129, 14336)):
        rc, s = cfg(so, T, n_used, n_expert, N, 1280, t)
        assert rc == 0, (T, n_used, n_expert, N, s)
        fam, f = MR.cfg_fields(s)
        assert s.startswith("moe:") and fam == ("q4k_mmq" if t == Q4_K else "q6k_mmq")
        tt, rg, ks, r = int(f["TT"]), int(f["RG"]), int(f["KS"]), int(f["R"])
        assert (tt, rg) in FORMS and ks == 8 // rg and r == 16 * tt
        slots = T * n_used
        assert f["grid"] == f"{-(-N // (16 * rg))}x{slots // r + min(n_expert + 1, slots)}", s
        per = -(-slots // n_expert)
        fill = -(-N // 64) * -(-slots // 64) >= 256
        assert (tt, rg) == ((1, 1) if per <= 16 else (2, 1) if per <= 32 else (4, 4) if fill else (4, 1)), s
        seen.add((tt, rg))
    assert seen == FORMS


def test_workspace_size_is_monotone_and_covers_the_tables(so):
    size = so.qg_gemm_w4a8_moe_prefill_workspace_size
    assert size(0, 2, 4) == 0 and size(2, 0, 4) == 0 and size(2, 2, 0) == 0 and size(-1, 2, 4) == 0
    vals = (1, 2, 3, 15, 16, 17, 100, 1024)
    for a in vals:
        for b in vals:
            for e in (1, 2, 7, 130, 1024, 4096):
                s = size(a, b, e)
                slots = a * b
                # counts, two lists of the slots, a 16-B record per tile of the smallest size (16 rows)
                assert s >= 4 * ((e + 1) + 2 * slots + 4 * (slots // 16 + min(e + 1, slots)))
                assert s % WS_ALIGN == 0
                assert size(a + 1, b, e) >= s and size(a, b + 1, e) >= s and size(a, b, e + 1) >= s
                assert size(b, a, e) == s  # (a function of the slots and the experts)
    assert size(65535, 1, 4096) < 2 ** 21
