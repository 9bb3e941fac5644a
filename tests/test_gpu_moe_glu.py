"""qg_gemm_w4a8_moe_glu on the GPU: the gate product, the up product and the GLU of an MoE FFN block in one launch, for
Q4_K and Q6_K experts.

The reference of every case is the library's own qg.gemm_w4a8_moe on the gate experts and on the up experts (its bits
are pinned to the eager single call by tests/test_gpu_moe.py): ReGLU must equal np.where(g > 0, g, 0) * u bit for
bit, SwiGLU must stay within moe_glu_ref.swiglu_tol of g / (1 + exp(-g)) * u computed in float64 from those float32 g
and u. One case per type is also held against the NumPy models, so the module does not rest on the library alone.

Outputs go through out= into the interior of a sentinel-filled [slots + 2, N + pad] buffer (ldc > N, a guard row before
and after): the sentinels must survive, a second launch must give the same buffer bit for bit, and a slot whose id is
outside [0, n_expert) must be N times the bit pattern 0. The ids live in a [T, ids_stride] int32 tensor with
ids_stride > n_used whose spare columns hold other valid ids; gate and up experts are drawn differently, so swapping
them changes the result.
"""
import ctypes
import functools

import numpy as np
import pytest

import moe_glu_ref as GR
import moe_ref as MR
from moe_glu_ref import REGLU, SWIGLU, bits
from moe_ref import Q4_K, Q6_K

pytestmark = pytest.mark.gpu

F_SENT = -12345.0
KQ_K = (256, 1024, 4096, 2304, 4352)      # LPR 4 / 16 / 64 loop-free, then the unit loop at 16 and 64 lanes
SLOTS = ((1, 1), (3, 2), (9, 8))
TYPES = (Q4_K, Q6_K)
OPS = (REGLU, SWIGLU)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def make_ids(rng, T, n_used, n_expert, bad=True):
    """int32 [T, ids_stride], ids_stride = max(n_expert, n_used + 1) > n_used, every column a valid id; an id repeated
    inside a token and one repeated across tokens; with `bad`, -1 and n_expert in the middle of the step."""
    ids = rng.integers(0, n_expert, (T, max(n_expert, n_used + 1))).astype(np.int32)
    slots = T * n_used
    if bad and slots >= 3:
        for s, v in ((slots // 2, -1), (slots // 2 - 1 if slots < 6 else slots // 3, n_expert)):
            ids[s // n_used, s % n_used] = v
    if n_used >= 2:
        ids[0, 1] = ids[0, 0]
    if T >= 2:
        ids[T - 1, n_used - 1] = ids[0, 0]
    return ids


@functools.lru_cache(maxsize=None)
def operands(t, n_expert, n, k, rows, seed=0):
    """Gate experts, up experts (another draw of the same generator) and `rows` activation rows; never modified."""
    rng = np.random.default_rng([t, n_expert, n, k, rows, seed, 5])
    return MR.random_experts(rng, t, n_expert, n, k), MR.random_experts(rng, t, n_expert, n, k), MR.random_act(rng, rows, k)


class Step:
    """One decode step on the device; the reference g and u are computed once, by the decode entry."""

    def __init__(self, t, T, n_used, n, k, n_expert=4, seed=0, woff=None, fill=0, ids=None, bad=True, data=None):
        self.t, self.T, self.n_used, self.n_expert, self.n, self.k = t, T, n_used, n_expert, n, k
        self.gate_h, self.up_h, a_all = operands(t, n_expert, n, k, T + 2, seed) if data is None else data
        self.a_h = a_all[:T]
        self.ids_h = make_ids(np.random.default_rng([seed, T, n_used, n_expert]), T, n_used, n_expert, bad) if ids is None else ids
        put = dev if woff is None else (lambda x: MR.KR.dev_at(x, woff, fill))
        self.gate, self.up = put(self.gate_h), put(self.up_h)
        self.a = dev(a_all)[:T]  # two spare rows behind the tokens'
        self.ids_full = dev(self.ids_h)
        self.ids = self.ids_full[:, :n_used]
        self._gu = None

    def products(self, qg):
        """(g, u) float32 [T, n_used, N]: qg.gemm_w4a8_moe on the gate and on the up experts."""
        if self._gu is None:
            args = (self.ids, self.T, self.n_used, self.n, self.k, self.t)
            self._gu = (host(qg.gemm_w4a8_moe(self.a.unsqueeze(1), self.gate, *args, a_rows=1)).copy(),
                        host(qg.gemm_w4a8_moe(self.a.unsqueeze(1), self.up, *args, a_rows=1)).copy())
        return self._gu

    def launch_guarded(self, qg, op, pad, up=None):
        """(window [T, n_used, N], whole buffer): out= the interior of a sentinel-filled [slots + 2, N + pad] buffer."""
        import torch
        S = self.T * self.n_used
        buf = torch.full((S + 2, self.n + pad), F_SENT, dtype=torch.float32, device="cuda")
        out = buf[1:S + 1, :self.n].unflatten(0, (self.T, self.n_used))
        got = qg.gemm_w4a8_moe_glu(self.a, self.gate, self.up if up is None else up, self.ids, self.T, self.n_used, self.n,
                                   self.k, self.t, op, out=out)
        assert got.data_ptr() == out.data_ptr()
        whole = host(buf)
        return whole[1:S + 1, :self.n].reshape(self.T, self.n_used, self.n).copy(), whole

    def bad_slots(self):
        return [(tt, u) for tt in range(self.T) for u in range(self.n_used) if not 0 <= self.ids_h[tt, u] < self.n_expert]

    def check(self, qg, op, pad=None, what=""):
        pad = 1 + (3 * self.n + self.T + self.k // 32) % 29 if pad is None else pad
        c, whole = self.launch_guarded(qg, op, pad)
        outside = np.ones(whole.shape, bool)
        outside[1:-1, :self.n] = False
        assert (whole[outside] == np.float32(F_SENT)).all(), f"wrote outside the slots' rows (ldc = {self.n + pad})"
        g, u = self.products(qg)
        for tt, uu in self.bad_slots():
            assert (bits(g[tt, uu]) == 0).all() and (bits(c[tt, uu]) == 0).all(), (tt, uu)  # +0.0f, not -0.0f
        cfg = qg.moe_glu_config(self.T, self.n_used, self.n, self.k, self.t)
        if op == REGLU:
            ref = GR.reglu(g, u)
            diff = np.argwhere(bits(c) != bits(ref))
            assert diff.size == 0, f"{len(diff)} outputs differ from relu(g) * u, first {diff[:4].tolist()} ({cfg})"
        else:
            GR.assert_swiglu(c, g, u, f"{cfg} T={self.T} n_used={self.n_used} {what}")
        _, again = self.launch_guarded(qg, op, pad)
        assert np.array_equal(bits(whole), bits(again))
        return c


def rows_per_workgroup(cfg):
    f = MR.cfg_fields(cfg)[1]
    return int(f["WGS"]) // 64 * (64 // int(f["LPR"]))


# ---------------------------------------------------------------------------- 1. every form x row edge x slot count
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("k", KQ_K)
def test_every_form_row_edge_and_slot_count(qg, t, k):
    """Each LPR class, loop-free and with the unit loop, at N = 1 and one either side of a workgroup's rows (read from
    the config line, which must name the decode entry's LPR / WGS / ONE), at 1, 6 and 72 slots, both ops."""
    cfg = qg.moe_glu_config(3, 2, 1, k, t)
    assert cfg.split(" ")[1:] == qg.moe_config(3, 2, 1, k, t).split(" ")[1:], cfg
    rpb = rows_per_workgroup(cfg)
    for n in (1, rpb - 1, rpb + 1):
        for T, n_used in SLOTS:
            assert MR.cfg_fields(qg.moe_glu_config(T, n_used, n, k, t))[1]["grid"] == f"{(n + rpb - 1) // rpb}x{T * n_used}"
            s = Step(t, T, n_used, n, k)
            for op in OPS:
                s.check(qg, op)


def test_swapped_operands_differ(qg):
    s = Step(Q4_K, 3, 2, 9, 512, bad=False)
    a = s.launch_guarded(qg, REGLU, 3)[0]
    s.gate, s.up = s.up, s.gate
    assert not np.array_equal(bits(a), bits(s.launch_guarded(qg, REGLU, 3)[0]))


# ---------------------------------------------------------------------------- 2. against the independent models
@pytest.mark.parametrize("t", TYPES)
def test_reglu_against_the_model(qg, t):
    """|c - relu(G) U| <= tol_g |U| + tol_u |G| + tol_g tol_u + 2^-23 |G U|: G, U the float64 models of the two
    products, tol_* their decode GEMV bounds (W = 0), relu 1-Lipschitz, and one rounded multiplication."""
    R = MR.KR if t == Q4_K else MR.QR
    s = Step(t, 3, 2, 37, 1024)
    c = s.check(qg, REGLU)
    live = 0
    for tt in range(s.T):
        for u in range(s.n_used):
            e = int(s.ids_h[tt, u])
            if not 0 <= e < s.n_expert:
                continue
            row = s.a_h[tt].reshape(1, -1, 36)
            (G, _, mg), (U, _, mu) = R.gemm(row, s.gate_h[e]), R.gemm(row, s.up_h[e])
            tg, tu = R.tol(mg, s.k, 0), R.tol(mu, s.k, 0)
            bound = tg * np.abs(U) + tu * np.abs(G) + tg * tu + 2.0 ** -23 * np.abs(G * U)
            err = np.abs(c[tt, u].astype(np.float64) - (np.maximum(G, 0.0) * U)[0])
            assert (err <= bound[0]).all(), float((err / bound[0]).max())
            live += 1
    assert live >= 4


# ---------------------------------------------------------------------------- 3. the ends of the formats
def extremes_data(t):
    """Experts from the reference module's extremes(): expert 0 of the gate tensor is the extreme classes, one per row;
    the up experts are the same rows rotated by 3 within each expert, so g and u of an output meet two different
    classes. Tokens 0 and 1 (and 2 for Q6_K) are the extreme activation rows."""
    R = MR.KR if t == Q4_K else MR.QR
    n, n_expert, k, T = 16, 2, 512, 3
    aq, bq = R.extremes(np.random.default_rng([t, 2024]), T + 2, n * n_expert, k)
    gate = bq.reshape((n_expert, n) + bq.shape[1:])
    return (gate, np.ascontiguousarray(np.roll(gate, 3, axis=1)), aq), T, n, k, n_expert


@pytest.mark.parametrize("t", TYPES)
def test_extremes(qg, t):
    data, T, n, k, n_expert = extremes_data(t)
    ids = np.array([[0, 1, 1], [1, 0, 0], [0, 0, 1]], np.int32)
    s = Step(t, T, 2, n, k, n_expert=n_expert, ids=ids, data=data)
    g, u = s.products(qg)
    assert np.isfinite(g).all() and np.isfinite(u).all()
    print(f"extremes t={t}: |g| up to {np.abs(g).max():.3g}, |u| up to {np.abs(u).max():.3g}, "
          f"smallest nonzero |g| {np.abs(g[g != 0]).min():.3g}")
    for op in OPS:
        c = s.check(qg, op, what="extremes")
        assert np.isfinite(c).all()


# ---------------------------------------------------------------------------- 4. capture
@pytest.mark.parametrize("t", TYPES)
def test_captured_one_node_follows_the_ids(qg, t):
    """GEMV, GLU, GEMV in one graph: the fused call is one kernel node of its own between the two GEMV nodes (without
    it they merge into one; with it the merge counts two GEMV nodes, nothing merged, nothing absorbed), and a replay
    follows the ids it finds in the buffer."""
    import torch
    qg.set_capture_fusion(1)
    s = Step(t, 3, 2, 33, 1024)
    gk, gn = 4096, 64
    rng = np.random.default_rng(78)
    gw, ga = dev(MR.random_experts(rng, MR.Q4_0, 2, gn, gk)), dev(MR.random_act(rng, 1, gk))
    gout = torch.zeros((2, 1, gn), dtype=torch.float32, device="cuda")
    mout = torch.zeros((s.T, s.n_used, s.n), dtype=torch.float32, device="cuda")
    ids2_h = ((s.ids_h[:, ::-1] + 1) % s.n_expert).astype(np.int32).copy()
    ids2_h[0, 0] = s.n_expert  # an id out of range that was in range on the first replay

    def eager(ids_h):
        s.ids_full.copy_(dev(ids_h))
        return host(qg.gemm_w4a8_moe_glu(s.a, s.gate, s.up, s.ids, s.T, s.n_used, s.n, s.k, t, SWIGLU)).copy()

    ref2, ref1 = eager(ids2_h), eager(s.ids_h)
    assert not np.array_equal(bits(ref1), bits(ref2))

    def step(with_glu):
        qg.gemm_w4a8(ga, gw[0], 1, gn, gk, MR.Q4_0, out=gout[0])
        if with_glu:
            qg.gemm_w4a8_moe_glu(s.a, s.gate, s.up, s.ids, s.T, s.n_used, s.n, s.k, t, SWIGLU, out=mout)
        qg.gemm_w4a8(ga, gw[1], 1, gn, gk, MR.Q4_0, out=gout[1])

    graphs = {}
    for with_glu in (False, True):
        torch.cuda.synchronize()
        s0 = qg.capture_fusion_stats()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step(with_glu)
        s1 = qg.capture_fusion_stats()
        graphs[with_glu] = (g, (s1[0] - s0[0], s1[1] - s0[1]))
    assert graphs[False][1] == (1, 1)
    assert graphs[True][1] == (0, 2)
    g = graphs[True][0]
    for ids_h, ref in ((s.ids_h, ref1), (ids2_h, ref2)):
        s.ids_full.copy_(dev(ids_h))  # in place: the graph holds the pointer
        mout.fill_(F_SENT)
        g.replay()
        assert np.array_equal(bits(host(mout)), bits(ref))


# ---------------------------------------------------------------------------- 5. pointers and aliasing
@pytest.mark.parametrize("t", TYPES)
def test_weights_at_the_alignment_classes(qg, t):
    """B_gate and B_up at the type's smallest offset past a 256-B line, inside a buffer of 0xFF bytes, then of 0x00:
    the checks hold and the surrounding bytes reach no result."""
    off = {Q4_K: 16, Q6_K: 2}[t]
    res = []
    for fill in (0xFF, 0x00):
        s = Step(t, 3, 2, 19, 768, woff=off, fill=fill)
        assert s.gate.data_ptr() % 256 == off and s.up.data_ptr() % 256 == off
        res.append([s.check(qg, op) for op in OPS])
    for a, b in zip(*res):
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("t", TYPES)
def test_aliased_weights(qg, t):
    """B_up is B_gate: relu(g) * g, and silu(g) * g within the bound."""
    s = Step(t, 3, 2, 21, 1024)
    g, _ = s.products(qg)
    c = s.launch_guarded(qg, REGLU, 2, up=s.gate)[0]
    assert np.array_equal(bits(c), bits(GR.reglu(g, g)))
    c = s.launch_guarded(qg, SWIGLU, 2, up=s.gate)[0]
    GR.assert_swiglu(c, g, g, "aliased")


# ---------------------------------------------------------------------------- 6. the C ABI, the view entry, Python
def views(G, s, out, ids=None):
    ids = s.ids if ids is None else ids
    bb, row = MR.BB[s.t], MR.expert_bytes(s.t, 1, s.k)
    arow = s.k // 32 * 36
    ws = []
    for w_t in (s.gate, s.up):
        w = G.TensorView()
        w.data, w.type = w_t.data_ptr(), s.t
        w.ne[:], w.nb[:] = [s.k, s.n, s.n_expert, 1], [bb, row, row * s.n, row * s.n * s.n_expert]
        ws.append(w)
    a, i, o = G.TensorView(), G.TensorView(), G.TensorView()
    a.data, a.type = s.a.data_ptr(), G.Q8_1
    a.ne[:], a.nb[:] = [s.k, 1, s.T, 1], [36, arow, arow, arow * s.T]
    i.data, i.type = ids.data_ptr(), G.I32
    i.ne[:], i.nb[:] = [s.n_used, s.T, 1, 1], [4, 4 * ids.stride(0), 4 * ids.stride(0) * s.T, 4 * ids.stride(0) * s.T]
    o.data, o.type = out.data_ptr(), G.F32
    o.ne[:], o.nb[:] = [s.n, s.n_used, s.T, 1], [4, 4 * out.stride(1), 4 * out.stride(0), 4 * out.stride(0) * s.T]
    return ws[0], ws[1], a, i, o


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("op", OPS)
def test_c_abi_view_entry_and_python_agree(qg, t, op):
    import torch
    import quant_gemm._lib as L
    import quant_gemm.ggml as G
    P = ctypes.c_void_p
    s = Step(t, 3, 2, 21, 512, n_expert=16)
    assert s.ids.stride(0) == 16 and not s.ids.is_contiguous()
    py = host(qg.gemm_w4a8_moe_glu(s.a, s.gate, s.up, s.ids, s.T, s.n_used, s.n, s.k, t, op)).copy()
    if op == REGLU:
        assert np.array_equal(bits(py), bits(GR.reglu(*s.products(qg))))
    # the C ABI on raw pointers, ldc > N
    buf = torch.full((s.T, s.n_used, s.n + 3), F_SENT, dtype=torch.float32, device="cuda")
    st = P(torch.cuda.current_stream().cuda_stream)
    call = lambda k=s.k, goff=0, uoff=0, ldc=s.n + 3, glu_op=op: L.load().qg_gemm_w4a8_moe_glu(
        P(s.a.data_ptr()), P(s.gate.data_ptr() + goff), P(s.up.data_ptr() + uoff), s.n_expert, P(s.ids_full.data_ptr()),
        s.ids_full.stride(0), P(buf.data_ptr()), ldc, s.T, s.n_used, s.n, k, t, glu_op, st)
    # refusals on real buffers: the output untouched
    assert call(k=s.k - 32) == -2 and call(uoff=1) == -4 and call(goff=1) == -4 and call(ldc=s.n - 1) == -1
    assert call(glu_op=1) == -3
    assert (host(buf) == F_SENT).all()
    assert call() == 0
    got = host(buf)
    assert np.array_equal(bits(got[:, :, :s.n]), bits(py)) and (got[:, :, s.n:] == F_SENT).all()
    # the view entry
    buf.fill_(F_SENT)
    out = buf[:, :, :s.n]
    G.mul_mat_id_glu_from_ggml(*views(G, s, out), op)
    got = host(buf)
    assert np.array_equal(bits(got[:, :, :s.n]), bits(py)) and (got[:, :, s.n:] == F_SENT).all()
    # views the entry cannot express: refused, the output untouched
    buf.fill_(F_SENT)
    arow = s.k // 32 * 36
    for spoil in ("act_rows", "up_type", "up_ne", "up_nb", "expert_stride", "ids_type", "glu_op"):
        wg, wu, a, i, o = views(G, s, out)
        glu_op = op
        if spoil == "act_rows":      # b.ne[1] != 1: a row per slot is the down product's, not this entry's
            a.ne[1], a.nb[2], a.nb[3] = 2, 2 * arow, 2 * arow * s.T
        elif spoil == "up_type":
            wu.type = Q6_K if t == Q4_K else Q4_K
        elif spoil == "up_ne":
            wu.ne[2] = s.n_expert - 1
        elif spoil == "up_nb":
            wu.nb[3] += MR.BB[t]
        elif spoil == "expert_stride":
            wg.nb[2] += MR.BB[t]
            wu.nb[2] += MR.BB[t]
        elif spoil == "ids_type":
            i.type = G.F32
        else:
            glu_op = 1
        with pytest.raises(RuntimeError, match="unsupported"):
            G.mul_mat_id_glu_from_ggml(wg, wu, a, i, o, glu_op)
    assert (host(buf) == F_SENT).all()
    with pytest.raises(RuntimeError):
        qg.gemm_w4a8_moe_glu(s.a, s.gate, s.up, s.ids, s.T, s.n_used, s.n, s.k, MR.Q4_0, op)
    with pytest.raises(RuntimeError):
        qg.gemm_w4a8_moe_glu(s.a, s.gate, s.up[:-1], s.ids, s.T, s.n_used, s.n, s.k, t, op)
