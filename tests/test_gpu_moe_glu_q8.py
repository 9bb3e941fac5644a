"""qg_gemm_w4a8_moe_glu_q8_1 on the GPU against qg.quantize_q8_1(qg.gemm_w4a8_moe_glu(...)), byte for byte, and float64."""
import functools

import numpy as np
import pytest

import moe_ref as MR
from moe_glu_ref import REGLU, SWIGLU
from moe_ref import Q4_K, Q6_K
from test_gpu_moe_glu import dev, host
from test_moe_glu_q8_cpu import FORMS, check_against_f64, f64_case

pytestmark = pytest.mark.gpu
TYPES = (Q4_K, Q6_K)
IDS = np.array([[0, -1, 3, 1], [4, 2, 2, 1]], np.int32)  # ids_stride = 4 > n_used = 3; n_expert = 4: -1 and 4 out of range


@functools.lru_cache(maxsize=None)
def operands(t, n, k):
    rng = np.random.default_rng([t, n, k, 11])
    return dev(MR.random_experts(rng, t, 4, n, k)), dev(MR.random_experts(rng, t, 4, n, k)), dev(MR.random_act(rng, 2, k))


def both(qg, a, gate, up, ids, T, n_used, n, k, t, op, out=None):
    # (the entry's bytes, the composition's bytes)
    got = qg.gemm_w4a8_moe_glu_q8_1(a, gate, up, ids, T, n_used, n, k, t, op, out=out)
    return host(got), host(qg.quantize_q8_1(qg.gemm_w4a8_moe_glu(a, gate, up, ids, T, n_used, n, k, t, op)))


@pytest.mark.parametrize("op", (REGLU, SWIGLU))
@pytest.mark.parametrize("n", (32, 96, 160))
@pytest.mark.parametrize("k", sorted(FORMS))
@pytest.mark.parametrize("t", TYPES)
def test_every_form_bytes(qg, t, k, n, op):
    import torch
    gate, up, a = operands(t, n, k)
    ids = dev(IDS)[:, :3]
    nbytes = 2 * 3 * (n // 32) * 36
    buf = torch.full((nbytes + 128,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[64:64 + nbytes].view(2, 3, n // 32, 36)
    got, ref = both(qg, a, gate, up, ids, 2, 3, n, k, t, op, out=out)
    f = MR.cfg_fields(qg.moe_glu_q8_1_config(2, 3, n, k, t))[1]
    assert (f["LPR"], f["ONE"], f["P"]) == FORMS[k] and len(set(FORMS.values())) == 6, f  # the six forms, one per K
    assert ref.shape == got.shape == (2, 3, n // 32, 36) and np.array_equal(got, ref), f
    assert not got[0, 1].any() and not got[1, 0].any() and got[0, 0].any()
    again, _ = both(qg, a, gate, up, ids, 2, 3, n, k, t, op, out=out)
    whole = host(buf)
    assert np.array_equal(again, got) and (whole[:64] == 0xA5).all() and (whole[64 + nbytes:] == 0xA5).all()


@pytest.mark.parametrize("t", TYPES)
def test_against_float64(qg, t):
    case = f64_case(t)
    gate, up, a, ids = (dev(x) for x in case)
    check_against_f64(host(qg.gemm_w4a8_moe_glu_q8_1(a, gate, up, ids, 1, 2, 64, 1280, t, REGLU)), t, case)


@pytest.mark.parametrize("t", TYPES)
def test_extremes_and_zero_row(qg, t):
    """extremes() of the reference module (up rows rotated by 3): d overflows f16; token 3 is an all-zero activation row."""
    R = MR.KR if t == Q4_K else MR.QR
    aq, bq = R.extremes(np.random.default_rng([t, 2024]), 4, 64, 512)
    aq[3] = 0
    gate = bq.reshape((2, 32) + bq.shape[1:])
    ids = dev(np.array([[0, 1], [1, 0], [0, 0], [1, 0]], np.int32))
    for op in (REGLU, SWIGLU):
        got, ref = both(qg, dev(aq), dev(gate), dev(np.roll(gate, 3, axis=1)), ids, 4, 2, 32, 512, t, op)
        assert np.array_equal(got, ref) and not got[3].any()
    assert np.isinf(ref[..., 0:2].copy().view(np.float16)).any()


@pytest.mark.parametrize("t", TYPES)
def test_captured_follows_the_ids(qg, t):
    """GEMV, the entry, GEMV in one graph: each replay's bytes are the eager call's on the ids the replay finds."""
    import torch
    gate, up, a = operands(t, 96, 1280)
    ids_full, ids2 = dev(IDS), (IDS[::-1] + 1).astype(np.int32).copy()
    ids = ids_full[:, :3]
    rng = np.random.default_rng(78)
    gw, ga = dev(MR.random_experts(rng, MR.Q4_0, 2, 64, 4096)), dev(MR.random_act(rng, 1, 4096))
    gout = torch.zeros((2, 1, 64), dtype=torch.float32, device="cuda")
    out = torch.zeros((2, 3, 3, 36), dtype=torch.uint8, device="cuda")
    refs = []
    for h in (ids2, IDS):
        ids_full.copy_(dev(h))
        refs.append(host(qg.gemm_w4a8_moe_glu_q8_1(a, gate, up, ids, 2, 3, 96, 1280, t, SWIGLU)).copy())
    assert not np.array_equal(refs[0], refs[1])
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        qg.gemm_w4a8(ga, gw[0], 1, 64, 4096, MR.Q4_0, out=gout[0])
        qg.gemm_w4a8_moe_glu_q8_1(a, gate, up, ids, 2, 3, 96, 1280, t, SWIGLU, out=out)
        qg.gemm_w4a8(ga, gw[1], 1, 64, 4096, MR.Q4_0, out=gout[1])
    for h, ref in ((IDS, refs[1]), (ids2, refs[0]), (IDS, refs[1])):
        ids_full.copy_(dev(h))  # in place: the graph holds the pointer
        out.fill_(0xA5)
        g.replay()
        assert np.array_equal(host(out), ref)


def test_into_the_down_entry(qg):
    gate, up, a = operands(Q4_K, 256, 512)
    rng = np.random.default_rng(5)
    down, w = dev(MR.random_experts(rng, Q4_K, 4, 64, 256)), dev(rng.random((2, 3), np.float32))
    ids = dev(IDS)[:, :3]
    hs = [dev(h) for h in both(qg, a, gate, up, ids, 2, 3, 256, 512, Q4_K, SWIGLU)]
    c = [host(qg.gemm_w4a8_moe_down(h, down, ids, w, 2, 3, 64, 256, Q4_K)).view(np.uint32) for h in hs]
    assert np.array_equal(c[0], c[1]) and c[0].any()
