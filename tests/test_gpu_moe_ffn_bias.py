"""qg_gemm_w4a8_moe_glu_bias / qg_gemm_w4a8_moe_down_bias on the GPU (families "moe_glu:mxfp4_gemv",
"moe_down:mxfp4_gemv", and the Q4_K / Q6_K ones with bias): ReGLU and the down fold bit-identical to the float32 model of
moe_ffn_bias_ref on the products of qg_gemm_w4a8_moe, SwiGLU and gpt-oss's clamped SwiGLU within their bounds, ids read
on the device, MXFP4 experts at every byte offset, one kernel node when captured, the three surfaces alike, and the
host twins.

Common setup: 8 experts; ids rows n_used + 3 apart holding -1 and n_expert once there are four slots; bias rows N + 5
apart with NaN in the gap; C with ldc = N + 3 and a sentinel in the gap; the router weights rows n_used + 2 apart.
"""
import ctypes
import functools

import numpy as np
import pytest

import moe_down_ref as DR
import moe_ffn_bias_ref as FR
import moe_glu_ref as GR
import moe_ref as MR
import mxfp4_ref as XR
from moe_ffn_bias_ref import MXFP4, REGLU, SWIGLU, SWIGLU_OAI, bits
from moe_ref import Q4_K, Q6_K

pytestmark = pytest.mark.gpu

N_EXPERT = 8
F_SENT = -7.5  # fills an output before a call that must not touch all of it
OAI_PAIRS = ((1.702, 7.0), (1.0, 0.5))
GLU_K = (96, 288, 512, 928, 2048, 2880, 2912)  # LPR 4 / 16 / 64, each loop-free and looped, and an odd unit count
SLOTS = ((1, 1), (3, 2), (9, 8))  # (T, n_used)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def operands(t, T, n_used, n, k, small=False):
    """Host arrays of one FFN step, shared and never modified: experts [3 = gate, up, down][8, n, blocks, bytes],
    activations (a row per token; a row per slot), ids, biases [3][8, n + 5], router weights [T, n_used + 2].
    small: scales drawn so that g and u are of the order of the OAI limits (moe_ffn_bias_ref.small_experts)."""
    rng = np.random.default_rng([t, T, n_used, n, k, small])
    if small:
        w = np.stack([FR.small_experts(rng, t, N_EXPERT, n, k) for _ in range(3)])
    elif t == MXFP4:
        w = XR.random_mxfp4(rng, 3 * N_EXPERT * n, k).reshape(3, N_EXPERT, n, k // 32, 17)
    else:
        w = np.stack([MR.random_experts(rng, t, N_EXPERT, n, k) for _ in range(3)])
    a1, an = MR.random_act(rng, T, k), MR.random_act(rng, T * n_used, k)
    ids = np.full((T, n_used + 3), 12345, np.int32)  # the columns past n_used are never read
    ids[:, :n_used] = rng.integers(0, N_EXPERT, (T, n_used))
    if T * n_used >= 4:
        ids[0, 1], ids[T - 1, 0] = -1, N_EXPERT
    bias = (rng.uniform(-10.0, 10.0, (3, N_EXPERT, n + 5)) * (1.0 if small else 64.0)).astype(np.float32)
    bias[:, :, n:] = np.nan  # the gap is never read
    rw = rng.uniform(0.05, 1.0, (T, n_used + 2)).astype(np.float32)
    for tt in range(T):
        for u in range(n_used):
            if not 0 <= ids[tt, u] < N_EXPERT:
                rw[tt, u] = np.nan  # the weight of an id out of range is never read
    return w, a1, an, ids, bias, rw


class Step:
    """The operands on the device. MXFP4 experts start 1, 2 and 3 bytes past a 256-B line (gate, up, down)."""

    def __init__(self, t, T, n_used, n, k, small=False, ops=None):
        import torch
        self.t, self.T, self.n_used, self.n, self.k = t, T, n_used, n, k
        w, a1, an, ids, bias, rw = ops if ops is not None else operands(t, T, n_used, n, k, small)
        self.h = (w, a1, an, ids, bias, rw)
        self.ids_h, self.bias_h, self.rw_h = ids, bias, rw
        put = (lambda x, o: XR.dev_at(x, o)) if t == MXFP4 else (lambda x, o: dev(x))
        self.gate, self.up, self.down = put(w[0], 1), put(w[1], 2), put(w[2], 3)
        self.a1, self.an = dev(a1), dev(an)
        self.ids_full = dev(ids)
        self.ids = self.ids_full[:, :n_used]
        self.bias_full = dev(bias)
        self.bg, self.bu, self.bd = (self.bias_full[i][:, :n] for i in range(3))
        self.rw_full = dev(rw)
        self.rw = self.rw_full[:, :n_used]
        assert self.ids.stride(0) == n_used + 3 and self.bg.stride(0) == n + 5 and self.rw.stride(0) == n_used + 2
        self.cbuf = torch.full((T, n_used, n + 3), F_SENT, dtype=torch.float32, device="cuda")
        self.c = self.cbuf[:, :, :n]
        self.ybuf = torch.full((T, n + 3), F_SENT, dtype=torch.float32, device="cuda")
        self.y = self.ybuf[:, :n]

    def ok(self, ids_h=None):
        i = (self.ids_h if ids_h is None else ids_h)[:, :self.n_used]
        return (i >= 0) & (i < N_EXPERT)

    def products(self, qg, gate=None, up=None):
        """g and u of qg_gemm_w4a8_moe on the gate and the up experts."""
        args = (self.ids, self.T, self.n_used, self.n, self.k, self.t)
        return (host(qg.gemm_w4a8_moe(self.a1, self.gate if gate is None else gate, *args)).copy(),
                host(qg.gemm_w4a8_moe(self.a1, self.up if up is None else up, *args)).copy())

    def d(self, qg):
        return host(qg.gemm_w4a8_moe(self.an, self.down, self.ids, self.T, self.n_used, self.n, self.k, self.t,
                                     a_rows=self.n_used)).copy()

    def glu(self, qg, bg, bu, op, alpha=1.702, limit=7.0, gate=None, up=None):
        """The entry into the strided C; returns the N columns after checking that the gap kept the sentinel."""
        self.cbuf.fill_(F_SENT)
        qg.gemm_w4a8_moe_glu_bias(self.a1, self.gate if gate is None else gate, self.up if up is None else up, bg, bu, self.ids,
                                  self.T, self.n_used, self.n, self.k, self.t, op, alpha, limit, out=self.c)
        got = host(self.cbuf)
        assert (got[:, :, self.n:] == F_SENT).all()
        return got[:, :, :self.n].copy()

    def dn(self, qg, bias, weights):
        self.ybuf.fill_(F_SENT)
        qg.gemm_w4a8_moe_down_bias(self.an, self.down, bias, self.ids, weights, self.T, self.n_used, self.n, self.k, self.t,
                                   out=self.y)
        got = host(self.ybuf)
        assert (got[:, self.n:] == F_SENT).all()
        return got[:, :self.n].copy()


def rpb_of(cfg):
    f = MR.cfg_fields(cfg)[1]
    return int(f["WGS"]) // 64 * (64 // int(f["LPR"]))


def covers_all_offsets(s, x):
    if (s.n * (s.k // 32)) % 2 == 1:  # an odd expert stride: consecutive experts at all four bytes of a dword
        assert {x[e].data_ptr() % 4 for e in range(4)} == {0, 1, 2, 3}
        return True
    return False


# ---------------------------------------------------------------------------- 1. GLU, every form, exact
@pytest.mark.parametrize("k", GLU_K)
def test_glu_every_form_is_exact(qg, k):
    cfg = qg.moe_glu_bias_config(3, 2, 100, k, MXFP4)
    assert cfg.startswith("moe_glu:mxfp4_gemv ") and cfg.split(" ")[1:4] == qg.moe_config(3, 2, 100, k, MXFP4).split(" ")[1:4]
    rpb = rpb_of(cfg)
    odd = 0
    for n in (rpb - 1, rpb, rpb + 3):
        for T, n_used in SLOTS:
            s = Step(MXFP4, T, n_used, n, k)
            odd += covers_all_offsets(s, s.gate) and covers_all_offsets(s, s.up)
            g, u = s.products(qg)
            want, gb, ub = FR.glu_model(g, u, s.bias_h[0], s.bias_h[1], s.ids_h, N_EXPERT)
            got = s.glu(qg, s.bg, s.bu, REGLU)
            assert np.array_equal(bits(got), bits(want)), (n, T, n_used)
            assert (bits(got[~s.ok()]) == 0).all()  # +0.0f, not -0.0f, and no bias
            assert not np.array_equal(bits(got), bits(FR.zero_bad(GR.reglu(g, u), s.ids_h, N_EXPERT)))  # the bias is in
    if k == 2912:
        assert odd  # N = RPB - 1 = 15 rows of 91 blocks
    # one slot against the model too, so that "identical" is not "identically wrong"
    w, a1, _, ids, bias, _ = s.h
    t, us = T - 1, n_used - 1
    e = int(ids[t, us])
    assert 0 <= e < N_EXPERT
    g64, _, gmag = XR.gemm(a1[t][None], w[0][e])
    u64, _, umag = XR.gemm(a1[t][None], w[1][e])
    gb64, ub64 = g64[0] + bias[0][e, :n].astype(np.float64), u64[0] + bias[1][e, :n].astype(np.float64)
    r = np.maximum(gb64, 0.0) * ub64
    tg, tu = XR.tol(gmag[0], k, 0) + 2.0 ** -24 * np.abs(gb64), XR.tol(umag[0], k, 0) + 2.0 ** -24 * np.abs(ub64)
    tol = tg * np.abs(ub64) + tu * np.abs(gb64) + tg * tu + 2.0 ** -23 * np.abs(r)
    assert (np.abs(got[t, us].astype(np.float64) - r) <= tol).all()


# ---------------------------------------------------------------------------- 2. each bias null, gate / up swapped
def test_each_bias_null_in_turn_and_gate_up_swapped(qg):
    s = Step(MXFP4, 3, 2, 19, 2912)
    g, u = s.products(qg)
    b = s.bias_h
    outs = []
    for dbg, dbu, hbg, hbu in ((s.bg, s.bu, b[0], b[1]), (None, s.bu, None, b[1]), (s.bg, None, b[0], None),
                               (None, None, None, None), (s.bu, s.bg, b[1], b[0])):
        got = s.glu(qg, dbg, dbu, REGLU)
        assert np.array_equal(bits(got), bits(FR.glu_model(g, u, hbg, hbu, s.ids_h, N_EXPERT)[0]))
        outs.append(got)
    got = s.glu(qg, s.bu, s.bg, REGLU, gate=s.up, up=s.gate)  # the operands swapped whole: reglu(u + bu, g + bg)
    assert np.array_equal(bits(got), bits(FR.glu_model(u, g, b[1], b[0], s.ids_h, N_EXPERT)[0]))
    outs.append(got)
    assert not any(np.array_equal(bits(outs[i]), bits(outs[j])) for i in range(len(outs)) for j in range(i))


# ---------------------------------------------------------------------------- 3. SwiGLU and SwiGLU_OAI
def test_swiglu_and_swiglu_oai_within_their_bounds(qg):
    s = Step(MXFP4, 3, 4, 41, 2880, small=True)
    g, u = s.products(qg)
    _, gb, ub = FR.glu_model(g, u, s.bias_h[0], s.bias_h[1], s.ids_h, N_EXPERT, SWIGLU)
    ok = s.ok()
    got = s.glu(qg, s.bg, s.bu, SWIGLU)
    assert (bits(got[~ok]) == 0).all()
    GR.assert_swiglu(got[ok], gb[ok], ub[ok], "glu_bias SWIGLU")
    for alpha, limit in OAI_PAIRS:
        FR.assert_all_regions(gb[ok], ub[ok], limit)
        got = s.glu(qg, s.bg, s.bu, SWIGLU_OAI, alpha, limit)
        assert np.isfinite(got).all() and (bits(got[~ok]) == 0).all()
        FR.assert_oai(got[ok], gb[ok], ub[ok], alpha, limit, "gpu")


# ---------------------------------------------------------------------------- 4. the K-quants through the new entry
@pytest.mark.parametrize("k", [256, 2304])
@pytest.mark.parametrize("t", [Q4_K, Q6_K])
def test_kquants_through_the_glu_entry(qg, t, k):
    assert qg.moe_glu_bias_config(3, 2, 35, k, t) == qg.moe_glu_config(3, 2, 35, k, t)
    s = Step(t, 3, 2, 35, k)
    for op in (REGLU, SWIGLU):
        old = host(qg.gemm_w4a8_moe_glu(s.a1, s.gate, s.up, s.ids, s.T, s.n_used, s.n, s.k, t, op)).copy()
        assert np.array_equal(bits(s.glu(qg, None, None, op)), bits(old)), op
    g, u = s.products(qg)
    got = s.glu(qg, s.bg, s.bu, REGLU)
    assert np.array_equal(bits(got), bits(FR.glu_model(g, u, s.bias_h[0], s.bias_h[1], s.ids_h, N_EXPERT)[0]))
    assert not np.array_equal(bits(got), bits(s.glu(qg, None, None, REGLU)))


# ---------------------------------------------------------------------------- 5. down, exact
def check_down(qg, s):
    """With bias and without, the weights strided and null: the bits of the fold of d (+ bias)."""
    d = s.d(qg)
    outs = {}
    for dbias, hbias in ((s.bd, s.bias_h[2]), (None, None)):
        db = FR.add_bias(d, hbias, s.ids_h, N_EXPERT)
        for dw, hw in ((s.rw, s.rw_h), (None, None)):
            got = s.dn(qg, dbias, dw)
            assert np.isfinite(got).all()
            assert np.array_equal(bits(got), bits(DR.fold(db, s.ids_h, hw, N_EXPERT))), (s.T, s.n_used, s.n, s.k)
            outs[(hbias is None, hw is None)] = got
    if s.ok().any():
        assert not np.array_equal(bits(outs[(False, False)]), bits(outs[(True, False)]))
    return outs


@pytest.mark.parametrize("n_used,k", [(u, k) for u in (1, 3, 4, 8) for k in (96, 512, 2880, 2912)] + [(16, 2048)])
def test_down_is_exact(qg, n_used, k):
    v = DR.launch(qg.moe_down_bias_config(3, n_used, 100, k, MXFP4))
    assert v["family"] == "mxfp4_gemv" and v["lds"] == FR.mxfp4_down_lds(n_used, k)
    assert (v["SW"], v["RPB"]) == FR.down_sw_rpb(n_used, v["LPR"], v["WGS"])
    rpb = v["RPB"]
    for T, n in ((1, rpb + 3), (3, rpb - 1), (3, rpb), (3, rpb + 3)):
        if n >= 1:
            s = Step(MXFP4, T, n_used, n, k)
            covers_all_offsets(s, s.down)
            check_down(qg, s)
    # a token whose ids are all out of range: a row of +0.0f; the other tokens as before
    ref = s.dn(qg, s.bd, s.rw)
    bad = s.ids_h.copy()
    bad[1, :n_used] = [(-1, N_EXPERT, -2 ** 31, 2 ** 31 - 1)[u % 4] for u in range(n_used)]
    s.ids_full.copy_(dev(bad))
    got = s.dn(qg, s.bd, s.rw)
    assert (bits(got[1]) == 0).all() and np.array_equal(bits(got[[0, 2]]), bits(ref[[0, 2]]))


@pytest.mark.parametrize("k", [256, 2304])
@pytest.mark.parametrize("t", [Q4_K, Q6_K])
def test_kquants_through_the_down_entry(qg, t, k):
    for n_used in (3, 8):
        assert qg.moe_down_bias_config(3, n_used, 35, k, t) == qg.moe_down_config(3, n_used, 35, k, t)
        s = Step(t, 3, n_used, 35, k)
        outs = check_down(qg, s)
        for null_w in (False, True):
            old = host(qg.gemm_w4a8_moe_down(s.an, s.down, s.ids, None if null_w else s.rw, s.T, n_used, s.n, k, t))
            assert np.array_equal(bits(outs[(True, null_w)]), bits(old))


# ---------------------------------------------------------------------------- 6. extremes
def test_extremes(qg):
    """mxfp4_ref.extremes as experts (expert e: its weight rows rolled by e) and as activations: ReGLU (a product may
    overflow to inf, as in the model) and down exact, OAI finite and within its bound."""
    n, k, T, n_used = 16, 512, 4, 2
    rng = np.random.default_rng(606)
    aq, bq = XR.extremes(rng, n, k)
    w = np.stack([np.stack([np.roll(bq, e + 3 * i, axis=0) for e in range(N_EXPERT)]) for i in range(3)])
    _, _, _, ids, bias, rw = operands(MXFP4, T, n_used, n, k, True)
    an = np.concatenate([aq, aq[::-1]])
    s = Step(MXFP4, T, n_used, n, k, ops=(w, aq, an, ids, bias, rw))
    g, u = s.products(qg)
    assert np.isfinite(g).all() and np.isfinite(u).all() and np.abs(g).max() > 2.0 ** 90
    with np.errstate(over="ignore"):
        want, gb, ub = FR.glu_model(g, u, bias[0], bias[1], ids, N_EXPERT)
    assert not np.isnan(want).any()
    assert np.array_equal(bits(s.glu(qg, s.bg, s.bu, REGLU)), bits(want))
    ok = s.ok()
    for alpha, limit in OAI_PAIRS:
        got = s.glu(qg, s.bg, s.bu, SWIGLU_OAI, alpha, limit)
        assert np.isfinite(got).all() and (bits(got[~ok]) == 0).all()
        FR.assert_oai(got[ok], gb[ok], ub[ok], alpha, limit, "extremes")
    check_down(qg, s)


# ---------------------------------------------------------------------------- 7. capture
def captured_between_two_gemvs(qg, call):
    """GEMV, call, GEMV in one graph: the call is one kernel node of its own between the two GEMV nodes (without it
    they merge into one; with it the merge counts two GEMV nodes, nothing merged, nothing absorbed). Returns the graph."""
    import torch
    qg.set_capture_fusion(1)
    gk, gn = 4096, 64
    rng = np.random.default_rng(78)
    gw, ga = dev(MR.random_experts(rng, MR.Q4_0, 2, gn, gk)), dev(MR.random_act(rng, 1, gk))
    gout = torch.zeros((2, 1, gn), dtype=torch.float32, device="cuda")
    graphs = {}
    for with_call in (False, True):
        torch.cuda.synchronize()
        s0 = qg.capture_fusion_stats()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            qg.gemm_w4a8(ga, gw[0], 1, gn, gk, MR.Q4_0, out=gout[0])
            if with_call:
                call()
            qg.gemm_w4a8(ga, gw[1], 1, gn, gk, MR.Q4_0, out=gout[1])
        s1 = qg.capture_fusion_stats()
        graphs[with_call] = (g, (s1[0] - s0[0], s1[1] - s0[1]))
    assert graphs[False][1] == (1, 1) and graphs[True][1] == (0, 2)
    return graphs[True][0], (ga, gw, gout)


@pytest.mark.parametrize("entry", ["glu", "down"])
def test_captured_one_node_follows_the_ids(qg, entry):
    s = Step(MXFP4, 3, 4, 19, 2912, small=True)
    ids2_h = s.ids_h.copy()
    ids2_h[:, :s.n_used] = (s.ids_h[:, :s.n_used][:, ::-1] + 1) % N_EXPERT
    ids2_h[1, 2] = N_EXPERT  # an id out of range that was in range on the first replay
    if entry == "glu":
        run = lambda: qg.gemm_w4a8_moe_glu_bias(s.a1, s.gate, s.up, s.bg, s.bu, s.ids, s.T, s.n_used, s.n, s.k, MXFP4,
                                                SWIGLU_OAI, out=s.c)
        buf = s.cbuf
    else:
        run = lambda: qg.gemm_w4a8_moe_down_bias(s.an, s.down, s.bd, s.ids, None, s.T, s.n_used, s.n, s.k, MXFP4, out=s.y)
        buf = s.ybuf
    refs = []
    for ids_h in (ids2_h, s.ids_h):
        s.ids_full.copy_(dev(ids_h))
        run()
        refs.append(host(buf).copy())
    assert not np.array_equal(bits(refs[0]), bits(refs[1]))
    # the eager results follow the new ids and the new experts' biases
    if entry == "down":
        for ids_h, ref in zip((ids2_h, s.ids_h), refs):
            s.ids_full.copy_(dev(ids_h))
            want = DR.fold(FR.add_bias(s.d(qg), s.bias_h[2], ids_h, N_EXPERT), ids_h, None, N_EXPERT)
            assert np.array_equal(bits(ref[:, :s.n]), bits(want))
    s.ids_full.copy_(dev(s.ids_h))
    g, keep = captured_between_two_gemvs(qg, run)
    for ids_h, ref in ((s.ids_h, refs[1]), (ids2_h, refs[0])):
        s.ids_full.copy_(dev(ids_h))  # in place: the graph holds the pointer
        buf.fill_(F_SENT)
        g.replay()
        assert np.array_equal(bits(host(buf)), bits(ref))


# ---------------------------------------------------------------------------- 8. the C ABI, the view entry, Python
def tv(G, data, qtype, ne, nb):
    v = G.TensorView()
    v.data, v.type = data, qtype
    v.ne[:], v.nb[:] = ne, nb
    return v


def views(G, s, down):
    row, arow, st = s.k // 32 * 17, s.k // 32 * 36, s.ids.stride(0)
    wv = lambda x: tv(G, x.data_ptr(), G.MXFP4, [s.k, s.n, N_EXPERT, 1], [17, row, row * s.n, row * s.n * N_EXPERT])
    bv = lambda b: tv(G, b.data_ptr(), G.F32, [s.n, N_EXPERT, 1, 1], [4, 4 * (s.n + 5)] + 2 * [4 * (s.n + 5) * N_EXPERT])
    iv = tv(G, s.ids.data_ptr(), G.I32, [s.n_used, s.T, 1, 1], [4, 4 * st, 4 * st * s.T, 4 * st * s.T])
    if down:
        av = tv(G, s.an.data_ptr(), G.Q8_1, [s.k, s.n_used, s.T, 1], [36, arow, arow * s.n_used, arow * s.n_used * s.T])
        rs = s.rw.stride(0)
        rv = tv(G, s.rw.data_ptr(), G.F32, [s.n_used, s.T, 1, 1], [4, 4 * rs, 4 * rs * s.T, 4 * rs * s.T])
        ld = s.y.stride(0)
        ov = tv(G, s.y.data_ptr(), G.F32, [s.n, s.T, 1, 1], [4, 4 * ld, 4 * ld * s.T, 4 * ld * s.T])
        return wv(s.down), bv(s.bd), av, iv, rv, ov
    av = tv(G, s.a1.data_ptr(), G.Q8_1, [s.k, 1, s.T, 1], [36, arow, arow, arow * s.T])
    ov = tv(G, s.c.data_ptr(), G.F32, [s.n, s.n_used, s.T, 1], [4, 4 * s.c.stride(1), 4 * s.c.stride(0), 4 * s.c.stride(0) * s.T])
    return wv(s.gate), wv(s.up), bv(s.bg), bv(s.bu), av, iv, ov


def test_c_abi_view_entry_and_python_agree(qg):
    import torch
    import quant_gemm._lib as L
    import quant_gemm.ggml as G
    P = ctypes.c_void_p
    so = L.load()
    s = Step(MXFP4, 3, 4, 19, 2912, small=True)
    p = lambda x: P(x.data_ptr())
    st = P(torch.cuda.current_stream().cuda_stream)
    ids_stride, bs = s.n_used + 3, s.n + 5
    # GLU
    py = s.glu(qg, s.bg, s.bu, SWIGLU_OAI)
    py_nogate = s.glu(qg, None, s.bu, SWIGLU_OAI)
    s.cbuf.fill_(F_SENT)
    call = lambda **kw: so.qg_gemm_w4a8_moe_glu_bias(p(s.a1), p(s.gate), p(s.up), P(s.bg.data_ptr() + kw.get("boff", 0)), p(s.bu),
                                                     kw.get("bs", bs), N_EXPERT, p(s.ids), ids_stride, p(s.cbuf), s.n + 3, s.T,
                                                     s.n_used, s.n, s.k, kw.get("t", MXFP4), kw.get("op", SWIGLU_OAI), 1.702,
                                                     kw.get("limit", 7.0), st)
    assert call(boff=2) == -4 and call(bs=s.n - 1) == -1 and call(limit=0.0) == -1 and call(op=1) == -3 and call(t=MR.Q8_0) == -3
    assert (host(s.cbuf) == F_SENT).all()
    assert call() == 0
    got = host(s.cbuf)
    assert np.array_equal(bits(got[:, :, :s.n]), bits(py)) and (got[:, :, s.n:] == F_SENT).all()
    for bgv, want in ((True, py), (False, py_nogate)):
        s.cbuf.fill_(F_SENT)
        wg, wu, vbg, vbu, av, iv, ov = views(G, s, False)
        G.mul_mat_id_glu_bias_from_ggml(wg, wu, vbg if bgv else None, vbu, av, iv, ov, SWIGLU_OAI, 1.702, 7.0)
        got = host(s.cbuf)
        assert np.array_equal(bits(got[:, :, :s.n]), bits(want)) and (got[:, :, s.n:] == F_SENT).all()
    s.cbuf.fill_(F_SENT)
    for spoil, code in (("bias_nb0", "unsupported"), ("expert_stride", "unsupported"), ("bias_dims", "invalid"),
                        ("bias_type", "unsupported"), ("bias_strides_differ", "unsupported")):
        wg, wu, vbg, vbu, av, iv, ov = views(G, s, False)
        if spoil == "bias_nb0":
            vbu.nb[0] = 8
        elif spoil == "expert_stride":  # experts a byte further apart than dense: not expressible
            wg.nb[2] += 1
            wu.nb[2] += 1
        elif spoil == "bias_dims":
            vbg.ne[1] = N_EXPERT - 1
        elif spoil == "bias_type":
            vbg.type = G.I32
        else:
            vbu.nb[1] += 4
        with pytest.raises(RuntimeError, match=code):
            G.mul_mat_id_glu_bias_from_ggml(wg, wu, vbg, vbu, av, iv, ov, SWIGLU_OAI, 1.702, 7.0)
    assert (host(s.cbuf) == F_SENT).all()
    # down
    py = s.dn(qg, s.bd, s.rw)
    py_nobias = s.dn(qg, None, s.rw)
    s.ybuf.fill_(F_SENT)
    dcall = lambda **kw: so.qg_gemm_w4a8_moe_down_bias(p(s.an), p(s.down), P(s.bd.data_ptr() + kw.get("boff", 0)), kw.get("bs", bs),
                                                       N_EXPERT, p(s.ids), ids_stride, p(s.rw), s.n_used + 2, p(s.ybuf), s.n + 3,
                                                       s.T, s.n_used, s.n, kw.get("k", s.k), kw.get("t", MXFP4), st)
    assert dcall(boff=1) == -4 and dcall(bs=-1) == -1 and dcall(t=MR.Q4_0) == -3 and dcall(k=s.k + 1) == -2
    assert dcall(k=FR.mxfp4_down_max_k(s.n_used) + 32) == -3
    assert (host(s.ybuf) == F_SENT).all()
    assert dcall() == 0
    got = host(s.ybuf)
    assert np.array_equal(bits(got[:, :s.n]), bits(py)) and (got[:, s.n:] == F_SENT).all()
    for bias_v, want in ((True, py), (False, py_nobias)):
        s.ybuf.fill_(F_SENT)
        wd, vb, av, iv, rv, ov = views(G, s, True)
        G.mul_mat_id_down_bias_from_ggml(wd, vb if bias_v else None, av, iv, rv, ov)
        got = host(s.ybuf)
        assert np.array_equal(bits(got[:, :s.n]), bits(want)) and (got[:, s.n:] == F_SENT).all()
    s.ybuf.fill_(F_SENT)
    for spoil, code in (("bias_nb0", "unsupported"), ("expert_stride", "unsupported"), ("bias_nb1", "unsupported")):
        wd, vb, av, iv, rv, ov = views(G, s, True)
        if spoil == "bias_nb0":
            vb.nb[0] = 2
        elif spoil == "expert_stride":
            wd.nb[2] += 1
        else:
            vb.nb[1] = 4 * s.n - 4
        with pytest.raises(RuntimeError, match=code):
            G.mul_mat_id_down_bias_from_ggml(wd, vb, av, iv, rv, ov)
    assert (host(s.ybuf) == F_SENT).all()
    # the old entries still refuse the type on these very buffers
    assert so.qg_gemm_w4a8_moe_glu(p(s.a1), p(s.gate), p(s.up), N_EXPERT, p(s.ids), ids_stride, p(s.cbuf), s.n + 3, s.T, s.n_used,
                                   s.n, s.k, MXFP4, 2, st) == -3


# ---------------------------------------------------------------------------- 9. the GPU against the host twins
def test_gpu_against_the_host_twins(qg):
    """One shape per entry, K = 64: the twins' products are those of qg_gemm_w4a8_moe_cpu, which adds a row's blocks in
    one chain where the GPU adds them across lanes; with two blocks both orders are the one sum of two terms, so g, u
    and d have the same bits on both sides and ReGLU and down must agree bit for bit (at a longer K the two products
    agree within the contract's bound only, and nothing here could be exact)."""
    import quant_gemm.host as H
    H.load()
    s = Step(MXFP4, 3, 4, 19, 64, small=True)
    w, a1, an, ids, bias, rw = s.h
    b = np.ascontiguousarray(bias)
    twin = lambda op, **kw: H.gemm_w4a8_moe_glu_bias(a1, w[0], w[1], b[0], b[1], ids, s.T, s.n_used, s.n, s.k, MXFP4, op, **kw)
    assert np.array_equal(bits(s.glu(qg, s.bg, s.bu, REGLU)), bits(twin(REGLU)))
    g, u = s.products(qg)
    _, gb, ub = FR.glu_model(g, u, bias[0], bias[1], ids, N_EXPERT, SWIGLU_OAI)
    ok = s.ok()
    for alpha, limit in OAI_PAIRS:
        got, tw = s.glu(qg, s.bg, s.bu, SWIGLU_OAI, alpha, limit), twin(SWIGLU_OAI, alpha=alpha, limit=limit)
        assert (bits(got[~ok]) == 0).all() and (bits(tw[~ok]) == 0).all()
        FR.assert_oai(got[ok], gb[ok], ub[ok], alpha, limit, "gpu")
        FR.assert_oai(tw[ok], gb[ok], ub[ok], alpha, limit, "twin")
        # GPU against twin: both sides carry an expf error, so twice the bound between them
        r = FR.swiglu_oai64(gb[ok], ub[ok], alpha, limit)
        assert (np.abs(got[ok].astype(np.float64) - tw[ok]) <= 2.0 * FR.oai_tol(r, gb[ok], alpha, limit)).all()
    rw_ok = np.where(np.isfinite(rw), rw, np.float32(0.5))
    s.rw_full.copy_(dev(rw_ok))
    tw = H.gemm_w4a8_moe_down_bias(an, w[2], b[2], ids, rw_ok, s.T, s.n_used, s.n, s.k, MXFP4)
    assert np.array_equal(bits(s.dn(qg, s.bd, s.rw)), bits(tw))
