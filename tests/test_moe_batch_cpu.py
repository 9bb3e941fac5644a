"""qg_gemm_w4a8_moe_batch without a GPU: the exported symbols, the validation codes and their order (on fake pointers
that every call refuses before a launch), qg_moe_batch_config (refusals, LPR / ONE of the decode entry, the rule for
the rows per tile with its LDS cap, the grid's upper bound), the workspace size function, the prefill's size function
unchanged, and the one text of each GEMV body."""
import ctypes
import os
import re
import subprocess

import pytest

import moe_ref as MR
from moe_ref import Q4_K, Q6_K, ROW_TYPES

P = ctypes.c_void_p
BIG = 1 << 40  # a workspace_bytes that is never too small
MAX_EXPERTS, MAX_SLOTS, WS_ALIGN, LDS_MAX, MIN_R = 4096, 65535, 16, 160 * 1024, 2  # qg.h
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "llama.cpp-quant-gemm_amd", "csrc")


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
    new = {"qg_gemm_w4a8_moe_batch", "qg_gemm_w4a8_moe_batch_workspace_size", "qg_moe_batch_config",
           "qg_mul_mat_id_from_view_batch"}
    assert new <= exported and new <= set(L.SIGNATURES)
    assert {"gemm_w4a8_moe_batch", "moe_batch_workspace_size", "moe_batch_config"} <= set(quant_gemm.__all__)
    assert callable(G.mul_mat_id_from_ggml_batch)
    header = open(L.LIB_PATH.replace("llama.cpp-quant-gemm_amd/quant_gemm/libqg_hip.so", "include/qg/qg.h")).read()
    for s in new:
        assert re.search(rf"\b{s}\(", header), s


def bat(so, A=4096, a_rows=1, B=4096, n_expert=4, ids=4096, ids_stride=2, C=4096, ldc=0, T=1, n_used=2, N=8, K=256, t=Q4_K,
        ws=4096, ws_bytes=BIG):
    p = lambda v: None if v is None else P(v)
    return so.qg_gemm_w4a8_moe_batch(p(A), a_rows, p(B), n_expert, p(ids), ids_stride, p(C), ldc, T, n_used, N, K, t,
                                     p(ws), ws_bytes, None)


def test_validation_codes_and_their_order(so):
    """Every call here is refused (or empty) before anything is enqueued: the pointers are never dereferenced."""
    size = so.qg_gemm_w4a8_moe_batch_workspace_size
    # 1 negative size, before K
    for kw in ({"T": -1}, {"n_used": -1}, {"N": -1}):
        assert bat(so, K=33, t=9, **kw) == -1
    # 2 K granule, before the type: 256 for Q4_K / Q6_K, 32 for a type the entry does not take
    assert bat(so, K=33, t=9) == -2 and bat(so, K=0) == -2 and bat(so, K=-256) == -2
    assert bat(so, K=288, t=Q4_K) == -2 and bat(so, K=4128, t=Q6_K) == -2
    # 3 type, before empty: the five row types are refused here, and so is everything that is no weight type
    for t in ROW_TYPES + (9, 0, 1, 5, 13, 26):
        assert bat(so, K=256, t=t, T=0, A=None) == -3
        assert bat(so, K=288, t=t) == -3
    # 4 empty: nothing touched, whatever the rest is -- a null workspace included
    for kw in ({"T": 0}, {"n_used": 0}, {"N": 0}):
        assert bat(so, A=None, B=None, ids=None, C=None, a_rows=7, n_expert=0, ids_stride=-3, ldc=-1, ws=None, ws_bytes=0,
                   **kw) == 0
    # 5 null pointer, before alignment
    for kw in ({"A": None}, {"B": None}, {"ids": None}, {"C": None}):
        other = {"B": 4097} if "B" not in kw else {"A": 4098}
        assert bat(so, **kw, **other) == -1
    # 6 alignment: A and ids 4 B; B 16 B (Q4_K), 2 B (Q6_K); before the entry's own checks
    assert bat(so, A=4098, a_rows=3) == -4 and bat(so, ids=4098, n_expert=0) == -4
    assert bat(so, B=4104, t=Q4_K) == -4 and bat(so, B=4097, t=Q6_K) == -4
    assert bat(so, B=4098, t=Q6_K, a_rows=3) == -1  # 2 B is enough for Q6_K: on to the entry's checks
    # 7 the entry's own: INVALID_ARG, before the workspace
    assert bat(so, a_rows=3, ws=None) == -1 and bat(so, a_rows=0, ws=4100) == -1
    assert bat(so, ids_stride=1, ws=4100) == -1 and bat(so, n_expert=0, ws=4100) == -1 and bat(so, n_expert=-2) == -1
    assert bat(so, ldc=7, ws=4100) == -1 and bat(so, ldc=-8) == -1
    # 8 the workspace: null, then its alignment, then its size -- before the unsupported shapes
    need = size(1, 2, 4)
    assert need > 0
    assert bat(so, ws=None) == -1
    for off in (1, 2, 4, 8):
        assert bat(so, ws=4096 + off, ws_bytes=0) == -4
    assert bat(so, ws_bytes=need - 1) == -1
    assert bat(so, ws_bytes=0) == -1
    assert bat(so, T=8192, n_used=8, ids_stride=8, ws=None) == -1
    assert bat(so, T=8192, n_used=8, ids_stride=8, ws=4100) == -4
    assert bat(so, T=8192, n_used=8, ids_stride=8, ws_bytes=size(8192, 8, 4) - 1) == -1
    k_big = (LDS_MAX // MR.KQ_REC_BYTES[Q4_K] + 1) * 256  # the decode entry's first refused K
    assert bat(so, K=k_big, ws=None) == -1 and bat(so, K=k_big, ws=4100) == -4 and bat(so, K=k_big, ws_bytes=need - 1) == -1
    # 9 the unsupported shapes
    assert bat(so, T=8192, n_used=8, ids_stride=8, ws_bytes=size(8192, 8, 4)) == -3       # 65536 slots
    assert bat(so, T=65536, n_used=1, ids_stride=1) == -3
    assert bat(so, n_expert=MAX_EXPERTS + 1) == -3
    assert bat(so, n_expert=MAX_EXPERTS + 1, ws_bytes=size(1, 2, MAX_EXPERTS + 1) - 1) == -1
    assert bat(so, K=k_big) == -3                                                          # what the decode entry refuses
    # an expert stride off the 16 B of Q4_K cannot occur (144 N K/256); Q6_K has no such stride (2 B)


def cfg(so, T, n_used, n_expert, N, K, t):
    buf = ctypes.create_string_buffer(256)
    rc = so.qg_moe_batch_config(T, n_used, n_expert, N, K, t, buf, 256)
    return rc, buf.value.decode()


def moe_cfg(so, T, n_used, N, K, t):
    buf = ctypes.create_string_buffer(256)
    rc = so.qg_moe_config(T, n_used, N, K, t, buf, 256)
    return rc, buf.value.decode()


def test_config_arguments_and_refusals(so):
    assert so.qg_moe_batch_config(1, 1, 4, 8, 256, Q4_K, None, 0) == -1
    assert cfg(so, -1, 1, 4, 8, 33, Q4_K)[0] == -1 and cfg(so, 1, 1, 4, 8, 288, Q4_K)[0] == -2
    for t in ROW_TYPES + (9,):
        assert cfg(so, 4, 2, 4, 8, 256, t) == (-3, "")
    assert cfg(so, 0, 2, 4, 8, 256, Q4_K) == (0, "")
    assert cfg(so, 4, 2, 0, 8, 256, Q4_K)[0] == -1
    assert cfg(so, 65536, 1, 4, 8, 256, Q6_K)[0] == -3 and cfg(so, 4, 2, MAX_EXPERTS + 1, 8, 256, Q6_K)[0] == -3
    assert cfg(so, 65535, 1, MAX_EXPERTS, 8, 256, Q6_K)[0] == 0
    assert cfg(so, 8, 128, 1024, 8, 256, Q4_K)[0] == 0  # 1024 experts are served
    for t in (Q4_K, Q6_K):
        # the largest K whose records of two rows fit the LDS, and the next; the decode entry serves both
        k2 = LDS_MAX // (MIN_R * MR.KQ_REC_BYTES[t]) * 256
        assert cfg(so, 1, 2, 4, 8, k2, t)[0] == 0 and f" R=2 " in cfg(so, 64, 2, 4, 8, k2, t)[1]
        assert cfg(so, 1, 2, 4, 8, k2 + 256, t) == (-3, "") and moe_cfg(so, 1, 2, 8, k2 + 256, t)[0] == 0


def expected_rows(slots, n_expert, K, t):
    per = -(-slots // n_expert)
    r = 2 if per <= 2 else 4 if per <= 4 else 8
    while r * (K // 256) * MR.KQ_REC_BYTES[t] > LDS_MAX:
        r //= 2
    return r


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
def test_config_names_family_rows_and_the_decode_entrys_kernel_choice(so, t):
    """The string carries the family, R by the stated rule (with the LDS cap), LPR / WGS / ONE of qg_moe_config for the
    same (N, K, type), grid = row tiles x (floor(slots / R) + min(n_expert + 1, slots)) and lds = R K/256 records."""
    import itertools
    seen = set()
    for K in (256, 512, 1024, 1280, 4096, 4352, 15360, 15616, 17152, 17408, 30976, 31232, 34304, 34560):
        for T, n_used, n_expert, N in itertools.product((1, 7, 33, 200), (1, 2, 8), (1, 3, 8, 130, 1024), (1, 65, 4097)):
            rc, s = cfg(so, T, n_used, n_expert, N, K, t)
            assert rc == 0, (T, n_used, n_expert, N, K, s)
            fam, f = MR.cfg_fields(s)
            assert s.startswith("moeb:") and fam == ("q4k_gemv" if t == Q4_K else "q6k_gemv")
            rc1, single = moe_cfg(so, T, n_used, N, K, t)
            assert rc1 == 0 and MR.kernel_choice(s) == MR.kernel_choice(single), (s, single)
            f1 = MR.cfg_fields(single)[1]
            assert f["WGS"] == f1["WGS"]
            slots, r = T * n_used, int(f["R"])
            assert r == expected_rows(slots, n_expert, K, t), s
            rpb = int(f["WGS"]) // 64 * (64 // int(f["LPR"]))
            assert f["grid"] == f"{-(-N // rpb)}x{slots // r + min(n_expert + 1, slots)}", s
            assert int(f["lds"]) == r * (K // 256) * MR.KQ_REC_BYTES[t] <= LDS_MAX, s
            seen.add((r, f["LPR"], f["ONE"]))
    assert {x[0] for x in seen} == {2, 4, 8} and len(seen) == 18, seen  # every instantiation of the type


def test_rows_per_tile_at_the_lds_cap(so):
    """per > 4 asks for R = 8: Q4_K keeps it up to K = 15360 and takes 4 from 15616 on, 2 beyond 30976; Q6_K 17152 /
    17408 and 34304."""
    rows = lambda K, t: int(MR.cfg_fields(cfg(so, 64, 1, 2, 5, K, t)[1])[1]["R"])
    assert [rows(K, Q4_K) for K in (15360, 15616, 30976, 31232)] == [8, 4, 4, 2]
    assert [rows(K, Q6_K) for K in (17152, 17408, 34304, 34560)] == [8, 4, 4, 2]
    # per <= 4 and per <= 2 below the cap
    assert int(MR.cfg_fields(cfg(so, 16, 1, 4, 5, 15616, Q4_K)[1])[1]["R"]) == 4
    assert int(MR.cfg_fields(cfg(so, 8, 1, 4, 5, 15616, Q4_K)[1])[1]["R"]) == 2


def test_workspace_size_is_monotone_and_covers_the_tables(so):
    size = so.qg_gemm_w4a8_moe_batch_workspace_size
    assert size(0, 2, 4) == 0 and size(2, 0, 4) == 0 and size(2, 2, 0) == 0 and size(-1, 2, 4) == 0
    assert size(2, -1, 4) == 0 and size(2, 2, -1) == 0
    vals = (1, 2, 3, 15, 16, 17, 100, 1024)
    for a in vals:
        for b in vals:
            for e in (1, 2, 7, 130, 1024, 4096):
                s = size(a, b, e)
                slots = a * b
                # the header, the counts, two lists of the slots, a 16-B record per tile of the smallest size (2 rows)
                assert s >= 4 * (4 + (e + 1) + 2 * slots + 4 * (slots // MIN_R + min(e + 1, slots)))
                assert s % WS_ALIGN == 0
                assert size(a + 1, b, e) >= s and size(a, b + 1, e) >= s and size(a, b, e + 1) >= s
                assert size(b, a, e) == s  # (a function of the slots and the experts)
                assert s >= so.qg_gemm_w4a8_moe_prefill_workspace_size(a, b, e)
    assert size(65535, 1, 4096) < 2 ** 21


def test_the_prefills_workspace_size_is_unchanged(so):
    """moe_plan_layout's formula, restated: 4 + the bins, the slots twice (each region rounded up to four int32) and
    four int32 per tile of 16 rows."""
    up4 = lambda v: (v + 3) & ~3
    for T, n_used, n_expert in ((1, 1, 1), (16, 2, 8), (64, 8, 128), (33, 3, 130), (1024, 8, 1024), (65535, 1, 4096)):
        slots = T * n_used
        want = 4 * (4 + up4(n_expert + 1) + 2 * up4(slots) + 4 * (slots // 16 + min(n_expert + 1, slots)))
        assert so.qg_gemm_w4a8_moe_prefill_workspace_size(T, n_used, n_expert) == want


@pytest.mark.parametrize("tag", ["q4k", "q6k"])
def test_the_new_file_includes_each_body_once(tag):
    text = open(os.path.join(CSRC, "qg_moe_batch.hip")).read()
    assert text.count(f'#include "qg_{tag}_gemv_body.inc"\n') == 1
    assert "auto do_unit" not in text
