"""qg_gemm_w4a8_moe_glu_batch without a GPU: exports, validation order on fake pointers, config against the batch entry's."""
import ctypes
import re
import subprocess

import pytest

import moe_ref as MR
from moe_ffn_bias_ref import MXFP4, SWIGLU_OAI
from moe_ref import Q4_K, Q6_K

P = ctypes.c_void_p
BIG, MAX_EXPERTS = 1 << 40, 4096  # a workspace_bytes that is never too small; qg.h
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def so():
    import quant_gemm._lib as L
    return L.load()


def test_new_symbols_are_exported():
    import quant_gemm
    import quant_gemm._lib as L
    nm = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    new = {"qg_gemm_w4a8_moe_glu_batch", "qg_moe_glu_batch_config"}
    assert new <= set(re.findall(r" T (qg_\w+)", nm)) and new <= set(L.SIGNATURES)
    assert {"gemm_w4a8_moe_glu_batch", "moe_glu_batch_config"} <= set(quant_gemm.__all__)


def glu(so, A=4096, Bg=4096, Bu=8192, bg=4096, bu=4096, bs=0, n_expert=4, ids=4096, ids_stride=2, C=4096, ldc=0, T=1, n_used=2,
        N=8, K=256, t=Q4_K, op=2, alpha=1.702, limit=7.0, ws=4096, ws_bytes=BIG):
    p = lambda v: None if v is None else P(v)
    return so.qg_gemm_w4a8_moe_glu_batch(p(A), p(Bg), p(Bu), p(bg), p(bu), bs, n_expert, p(ids), ids_stride, p(C), ldc, T,
                                         n_used, N, K, t, op, alpha, limit, p(ws), ws_bytes, None)


def test_validation_codes_and_their_order(so):
    """Every call here is refused (or empty) before anything is enqueued: the pointers are never dereferenced."""
    size = so.qg_gemm_w4a8_moe_batch_workspace_size
    assert all(glu(so, K=33, t=9, **kw) == -1 for kw in ({"T": -1}, {"n_used": -1}, {"N": -1}))  # sizes, then K, then type
    assert all(glu(so, **kw) == -2 for kw in ({"K": 33, "t": 9}, {"K": 0}, {"K": 288}, {"K": 4128, "t": Q6_K}, {"K": 48, "t": MXFP4}))
    for t in set(range(-1, 45)) - {Q4_K, Q6_K, MXFP4}:
        assert glu(so, K=256, t=t, T=0, A=None) == -3 and glu(so, K=288, t=t) == -3
    for kw in ({"T": 0}, {"n_used": 0}, {"N": 0}):  # empty: nothing touched, whatever the rest is
        assert glu(so, A=None, Bg=None, Bu=None, ids=None, C=None, n_expert=0, ids_stride=-3, ldc=-1, bs=-1, ws=None,
                   ws_bytes=0, op=7, **kw) == 0
    for kw in ({"A": None}, {"Bg": None}, {"Bu": None}, {"ids": None}, {"C": None}):  # null before alignment
        assert glu(so, **kw, **({"Bg": 4097} if "Bg" not in kw else {"A": 4098})) == -1
    assert glu(so, bg=None, bu=None, n_expert=0) == -1  # null biases are fine: on to n_expert
    assert all(glu(so, n_expert=0, **kw) == -4 for kw in ({"A": 4098}, {"ids": 4098}, {"Bg": 4104}, {"Bu": 4104}, {"bg": 4098},
                                                        {"bu": 4097}, {"Bg": 4097, "t": Q6_K}))
    assert glu(so, Bg=4097, Bu=4099, K=32, t=MXFP4, n_expert=0) == -1  # MXFP4 at any byte
    # ids_stride, n_expert, ldc, bias_stride, the OAI op's alpha and limit: before the workspace
    for kw in ({"ids_stride": 1}, {"n_expert": 0}, {"ldc": 7}, {"ldc": -8}, {"bs": 7}, {"bs": -1}, {"bs": 7, "bg": None, "bu": None},
               {"op": SWIGLU_OAI, "alpha": NAN}, {"op": SWIGLU_OAI, "limit": 0.0}, {"op": SWIGLU_OAI, "limit": INF}):
        assert glu(so, ws=4100, **kw) == -1, kw
    assert glu(so, alpha=NAN, limit=-1.0, ws=4100) == -4  # read for the third op alone
    need = size(1, 2, 4)  # the workspace: null, its alignment, its size -- before the unsupported shapes and the op
    assert need > 0 and glu(so, ws=None, op=1) == -1 and glu(so, ws_bytes=need - 1, op=1) == -1
    assert all(glu(so, ws=4096 + off, ws_bytes=0, op=1) == -4 for off in (1, 2, 4, 8))
    big = dict(T=8192, n_used=8, ids_stride=8)  # 65536 slots
    assert glu(so, ws_bytes=size(8192, 8, 4) - 1, **big) == -1 and glu(so, ws_bytes=size(8192, 8, 4), **big) == -3
    assert glu(so, n_expert=MAX_EXPERTS + 1) == -3 and glu(so, n_expert=MAX_EXPERTS + 1, ws_bytes=size(1, 2, MAX_EXPERTS + 1) - 1) == -1
    for op in (1, 4, -1, 7):  # the op, last: everything above has passed, with exactly the size function's bytes
        assert glu(so, op=op, ws_bytes=need) == -3 and glu(so, op=op, ws_bytes=need - 1) == -1 and glu(so, op=op, bs=7) == -1


def cfg(so, sym, T, n_used, n_expert, N, K, t):
    buf = ctypes.create_string_buffer(256)
    return getattr(so, sym)(T, n_used, n_expert, N, K, t, buf, 256), buf.value.decode()


@pytest.mark.parametrize("t,ks", [(Q4_K, (256, 512, 1024, 1280, 4096, 4352, 15360, 15616, 30976, 31232, 62464, 62720)),
                                  (Q6_K, (256, 512, 1024, 1280, 4096, 4352, 17152, 17408, 34304, 34560, 68864, 69120)),
                                  (MXFP4, (32, 160, 512, 544, 2048, 2912, 13632, 13664, 27296, 27328, 54592, 54624))])
def test_config_fields_and_lds_thresholds_are_the_batch_entrys(so, t, ks):
    """Every field of the line and every status equal qg_moe_batch_bias_config's, over the (LPR, ONE) ladder, the K at
    which R halves for the LDS and the first K refused, at the slot counts that ask for R = 2, 4 and 8."""
    seen = set()
    for k in ks:
        for T in (3, 8, 40):  # 4 experts, 2 used: 2, 4 and 20 slots per expert
            (rc, s), (rc0, s0) = cfg(so, "qg_moe_glu_batch_config", T, 2, 4, 65, k, t), cfg(so, "qg_moe_batch_bias_config", T, 2, 4, 65, k, t)
            assert rc == rc0 and rc in (0, -3), (k, T, s, s0)
            if rc == 0:
                assert s.startswith("moeb_glu:") and MR.cfg_fields(s) == MR.cfg_fields(s0), (s, s0)
                seen.add(int(MR.cfg_fields(s)[1]["R"]))
    assert seen == {2, 4, 8} and rc == -3  # the last K is beyond the LDS of two rows
