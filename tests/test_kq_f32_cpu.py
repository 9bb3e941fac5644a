"""qg_gemm_w4a8_f32_kq without a GPU: the exports, the validation codes and their order on fake pointers, and the config
line's instantiation against the single call's (qg_debug_config) over every (MT, LPR, ONE) form."""
import ctypes

import pytest

Q4_K, Q6_K = 12, 14
FAKE = 4096  # never dereferenced: every call here is refused, empty or a config query
MS, KS = (1, 2, 3, 5, 8), (256, 512, 1024, 2304, 4096, 4352)


@pytest.fixture(scope="module")
def so():
    import quant_gemm._lib as L
    return L.load()


def run(so, X=FAKE, B=FAKE, C=FAKE, M=1, N=8, K=256, t=Q4_K):
    return so.qg_gemm_w4a8_f32_kq(X, B, C, M, N, K, t, None)


def test_exported_and_mirrored(so):
    import quant_gemm
    import quant_gemm._lib as L
    for name in ("qg_gemm_w4a8_f32_kq", "qg_f32_kq_config"):
        assert hasattr(so, name) and name in L.SIGNATURES
    assert {"gemm_w4a8_f32_kq", "f32_kq_config"} <= set(quant_gemm.__all__)


def test_validation_codes_and_their_order(so):
    # negative sizes first: before K, the type and the pointers
    assert run(so, M=-1, K=33, t=2, X=None) == -1 and run(so, N=-1, K=33, t=2, X=None) == -1
    # K: a positive multiple of 256, before the type
    for k in (0, -256, 32, 288, 4128):
        assert run(so, K=k, t=2, X=None) == -2, k
    # what no launch of the kernel serves, before the empty call and the pointers
    for t in (11, 23, 39, 2):
        assert run(so, t=t, X=None) == -3 and run(so, t=t, M=0) == -3, t
    assert run(so, M=9, X=None) == -3 and run(so, M=9, N=0, t=Q6_K) == -3
    k4, k6 = 160 * 1024 // 336 * 256, 160 * 1024 // 304 * 256  # the last K whose records of one row fit: Q4_K's, Q6_K's
    assert run(so, K=k4 + 256, X=None) == -3 and run(so, K=k6 + 256, t=Q6_K, X=None) == -3 and run(so, M=2, K=k4, X=None) == -3
    assert run(so, K=k4, X=None) == -1 and run(so, K=k4 + 256, t=Q6_K, X=None) == -1  # these fit: on to the pointers
    # empty: nothing touched, whatever the pointers are
    assert run(so, X=None, B=1, C=2, M=0) == 0 and run(so, X=None, B=None, C=None, N=0, t=Q6_K) == 0
    # null before alignment
    for kw in (dict(X=None), dict(B=None), dict(C=None)):
        assert run(so, **{"B": FAKE + 8, **kw}) == -1, kw
    # alignment: X 16 B, C 4 B, B by the type (Q4_K 16 B, Q6_K 2 B)
    for kw in (dict(X=FAKE + 4), dict(X=FAKE + 8), dict(C=FAKE + 2), dict(B=FAKE + 8), dict(B=FAKE + 1, t=Q6_K)):
        assert run(so, **kw) == -4, kw


def fields(line):
    return {k: v for k, v in (f.split("=") for f in line.split()[1:])}


def test_config_is_the_single_calls_instantiation():
    import quant_gemm as qg
    seen = set()
    for t, fam in ((Q4_K, "q4k"), (Q6_K, "q6k")):
        for m in MS:
            for k in KS:
                got, single = qg.f32_kq_config(m, 67, k, t), qg.debug_config(m, 67, k, t)
                assert got.startswith(fam + "_gemv_f32 MT=") and single.startswith(fam + "_gemv MT="), (got, single)
                g, s = fields(got), fields(single)
                assert list(g) == ["MT", "LPR", "WGS", "ONE", "grid", "lds"] and all(g[f] == s[f] for f in g), (got, single)
                seen.add((t, g["MT"], g["LPR"], g["ONE"]))
    assert len(seen) == 2 * 24, sorted(seen)  # 4 MT x 3 LPR x 2 ONE per type
    assert qg.f32_kq_config(8, 67, 4352, Q4_K) == "q4k_gemv_f32 MT=8 LPR=64 WGS=1024 ONE=0 grid=5 lds=45696"
    assert qg.f32_kq_config(0, 67, 256, Q4_K) == "none" and qg.f32_kq_config(1, 0, 256, Q6_K) == "none"
    buf = ctypes.create_string_buffer(64)
    so = qg._lib.load()
    assert so.qg_f32_kq_config(9, 8, 256, Q4_K, buf, 64) == -3 and so.qg_f32_kq_config(1, 8, 256, Q4_K, None, 0) == -1
