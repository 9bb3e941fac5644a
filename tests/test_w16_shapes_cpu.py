"""The W4A16 / W8A16 GPU tests' shape lists against qg_w16_config, without a GPU: every list must reach the kernel family
its test is named for (tests/test_gpu_w4a16.py, tests/test_gpu_w16d.py and the W16 cases of tests/test_gpu_small_k.py).
The lists are imported, not copied, so a retune that moves a test's shape to another kernel fails here instead of
leaving the GPU test to check something else than it says. On a GPU-less host the dispatch sees 256 CUs, a whole
MI355X's."""
import pytest

import test_gpu_small_k as S
import test_gpu_w16d as D
import test_gpu_w4a16 as A
from test_w16_pick_cpu import FAMILIES, bind, config, fields

TYPES = (2, 8)
ANY_WS = 1 << 40  # the library's per-stream workspace always suffices: as a caller's of any size
SPLIT = ("w16s", "w16sk")


@pytest.fixture(scope="module")
def so():
    import quant_gemm._lib as L
    return bind(L.load())


def shapes_of(test):
    """the (m, n, k) list of the test's parametrize mark"""
    for mark in test.pytestmark:
        if mark.name == "parametrize" and mark.args[0].startswith("m,"):
            return list(mark.args[1])
    raise AssertionError(test.__name__)


def ask(so, shape, t, **kw):
    rc, text = config(so, *shape, t=t, ws=kw.pop("ws", ANY_WS), **kw)
    assert rc == 0 and text, (shape, t, rc)
    return fields(text)


def test_w16d_lists_run_w16d(so):
    for t in TYPES:
        for shape in D.SHAPES + shapes_of(D.test_w16d_two_part_split_error):
            assert ask(so, shape, t)["family"] == "w16d", (shape, t)
        got = [ask(so, s, t) for s in D.SHAPES]
        assert {f["RT"] for f in got} == {1, 2} and {f["NP"] for f in got} == {2, 3}  # 16- and 32-row tiles, K = 256
    assert {ask(so, s, 2)["SB"] for s in D.SHAPES} == {2, 4} and {ask(so, s, 2)["W"] for s in D.SHAPES} == {12, 16}
    assert all(ask(so, s, 2)["NP"] == 2 for s in shapes_of(D.test_w16d_two_part_split_error))


def test_workspace_tests_split_k(so):
    for t in TYPES:
        f = ask(so, A.WS_SHAPE, t)
        assert f["family"] in SPLIT and f["ks"] > 1 and 0 < f["ws"] <= so.qg_gemm_w16_workspace_size(*A.WS_SHAPE)
        assert ask(so, A.WS_SHAPE, t, ws=64)["family"] == "w16mfma"  # "too small -> not used"
    for shape in A.TWO_THREAD_SHAPES + [A.SECOND_STREAM_SHAPE]:
        f = ask(so, shape, 2)
        assert f["family"] in SPLIT and f["ks"] > 1 and f["ws"] > 0, shape


def test_prefill_lists_reach_the_three_prefill_families(so):
    for t in TYPES:
        got = {s: ask(so, s, t) for s in shapes_of(A.test_w16_prefill_split_k)}
        assert {f["family"] for f in got.values()} == {"w16d", "w16s", "w16sk"}
        for family in SPLIT:  # several slices through the workspace; w16_sk_kernel also with one slice and none
            assert max(f["ks"] for f in got.values() if f["family"] == family) > 1
        assert any(f["family"] == "w16sk" and f["ks"] == 1 and f["ws"] == 0 for f in got.values())
        assert {f["RT"] for f in got.values() if f["family"] == "w16sk"} == {4, 8}
        two = {s: ask(so, s, t) for s in shapes_of(A.test_w16_prefill_two_part_split_error)}
        assert {f["family"] for f in two.values()} == {"w16d", "w16s", "w16sk"}
        assert all(f["NP"] == 2 for f in two.values())
        assert {f["TT"] for f in two.values() if f["family"] == "w16s"} == {1, 2}  # "the last two: 32-token tiles"
        flt = [ask(so, (m, 64, k), t) for m, k in shapes_of(A.test_w16_prefill_activations_near_flt_max)]  # n = 64
        assert {f["NP"] for f in flt} == {2, 3} and {f["family"] for f in flt} == {"w16d", "w16s"}


def test_gemv_lists_run_the_gemv(so):
    for t in TYPES:
        small = [ask(so, s, t) for s in shapes_of(S.test_small_k_w16_gemv)]
        assert all(f["family"] == "w16gemv" and f["LPR"] in (16, 32) for f in small)  # the K < 4096 forms
        assert {f["LPR"] for f in small} == {16, 32} and {f["ONEU"] for f in small} == {0, 1}
        assert {f["SIG"] for f in small} == {"m1", "full"}
        mixed = [ask(so, s, t) for s in shapes_of(A.test_w16_matches_oracle)]
        assert {f["family"] for f in mixed} >= {"w16gemv", "w16generic", "w16d", "w16s"}
        assert {f["MT"] for f in mixed if f["family"] == "w16gemv"} == {1, 2, 4, 8}
    n, k = S.TWO_ROWS_NK
    assert ask(so, (1, n, k), 2)["family"] == "w16gemv1r" and ask(so, (1, 4096, k), 2)["family"] == "w16gemv"


def test_misaligned_cases(so):
    assert ask(so, A.UNALIGNED_A_SHAPE, 2, a_off=4)["family"] == "w16generic"
    f = ask(so, A.SK_SMALL_M_SHAPE, 2, b_off=4)
    assert f["family"] == "w16sk" and f["TT"] == 2 and A.SK_SMALL_M_SHAPE[0] <= 64
    assert ask(so, A.SK_SMALL_M_SHAPE, 2)["family"] == "w16d"  # aligned, it would not get there


def test_every_family_has_a_gpu_test(so):
    """The table of profiles/w16_pick/README.md: no kernel family is left to the CPU tests alone."""
    reached = set()
    for t in TYPES:
        for test in (A.test_w16_matches_oracle, A.test_w16_prefill_split_k, A.test_w16_prefill_two_part_split_error,
                     S.test_small_k_w16_gemv):
            reached |= {ask(so, s, t)["family"] for s in shapes_of(test)}
        reached |= {ask(so, A.WS_SHAPE, t, ws=64)["family"]}
    reached |= {ask(so, (1,) + S.TWO_ROWS_NK, 2)["family"], ask(so, A.SK_SMALL_M_SHAPE, 2, b_off=4)["family"]}
    assert reached == set(FAMILIES)
