"""qg_gemm_w4a8_moe_down on the GPU: the down product of an MoE FFN block with the router-weighted sum over the token's
experts in one launch, for Q4_K and Q6_K experts.

The reference of every case is the library's own qg.gemm_w4a8_moe at a_rows = n_used on the same operands (its bits
are pinned to the eager single call by tests/test_gpu_moe.py), folded in NumPy float32 by moe_down_ref.fold:
acc = +0.0f, then acc = acc + w * d_u per slot in ascending order, the slots whose id is out of range left out. Each
NumPy float32 operation is one rounding, so the comparison is bitwise; no tolerance is involved.

Outputs go through out= into the interior of a sentinel-filled [T + 2, N + pad] buffer (ldc > N, a guard row before and
after): the sentinels must survive and a second launch must give the same buffer bit for bit. The ids live in a
[T, ids_stride] int32 tensor with ids_stride > n_used and the weights in a [T, w_stride] float32 tensor with
w_stride > n_used (another stride than the ids'); the weights at the slots whose id is out of range are NaN, +inf and
-inf, which must reach nothing.
"""
import ctypes
import functools

import numpy as np
import pytest

import moe_down_ref as DR
import moe_ref as MR
from moe_down_ref import bits
from moe_ref import Q4_K, Q6_K

pytestmark = pytest.mark.gpu

F_SENT = -12345.0
KQ_K = (256, 512, 1024, 1280, 4096, 4352)  # LPR 4 / 16 / 64, each loop-free and with the unit loop
N_USED = (1, 2, 3, 8, 9)                   # below W, no power of two, more than one pass per wave at 256 threads
TYPES = (Q4_K, Q6_K)


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


def make_weights(rng, ids, n_used, n_expert):
    """float32 [T, n_used + 3]: router-like weights of both signs, one exact zero; NaN, +inf, -inf where the id names no
    expert and in the spare columns."""
    T = ids.shape[0]
    w = rng.uniform(-1.0, 1.0, (T, n_used + 3)).astype(np.float32)
    w[0, 0] = 0.0
    w[:, n_used:] = np.nan
    i = 0
    for t in range(T):
        for u in range(n_used):
            if not 0 <= ids[t, u] < n_expert:
                w[t, u] = (np.nan, np.inf, -np.inf)[i % 3]
                i += 1
    return w


@functools.lru_cache(maxsize=None)
def operands(t, n_expert, n, k, rows, seed=0):
    """Experts and `rows` activation rows; never modified."""
    rng = np.random.default_rng([t, n_expert, n, k, rows, seed, 9])
    return MR.random_experts(rng, t, n_expert, n, k), MR.random_act(rng, rows, k)


class Step:
    """One decode step on the device; the reference products are computed once, by the decode entry."""

    def __init__(self, t, T, n_used, n, k, n_expert=4, seed=0, woff=None, fill=0, ids=None, bad=True, data=None):
        self.t, self.T, self.n_used, self.n_expert, self.n, self.k = t, T, n_used, n_expert, n, k
        self.b_h, a_all = operands(t, n_expert, n, k, T * n_used + 2, seed) if data is None else data
        self.a_h = a_all[:T * n_used].reshape(T, n_used, k // 32, 36)
        rng = np.random.default_rng([seed, T, n_used, n_expert])
        self.ids_h = make_ids(rng, T, n_used, n_expert, bad) if ids is None else ids
        self.w_h = make_weights(rng, self.ids_h, n_used, n_expert)
        self.b = dev(self.b_h) if woff is None else MR.KR.dev_at(self.b_h, woff, fill)
        self.a = dev(a_all)[:T * n_used].unflatten(0, (T, n_used))  # two spare rows behind the slots'
        self.ids_full, self.w_full = dev(self.ids_h), dev(self.w_h)
        self.ids, self.w = self.ids_full[:, :n_used], self.w_full[:, :n_used]
        self._d = None

    def products(self, qg):
        """d float32 [T, n_used, N]: qg.gemm_w4a8_moe at a_rows = n_used."""
        if self._d is None:
            self._d = host(qg.gemm_w4a8_moe(self.a, self.b, self.ids, self.T, self.n_used, self.n, self.k, self.t,
                                            a_rows=self.n_used)).copy()
        return self._d

    def reference(self, qg, weights=True):
        return DR.fold(self.products(qg), self.ids_h, self.w_h if weights else None, self.n_expert)

    def launch_guarded(self, qg, pad, w="own"):
        """(window [T, N], whole buffer): out= the interior of a sentinel-filled [T + 2, N + pad] buffer."""
        import torch
        buf = torch.full((self.T + 2, self.n + pad), F_SENT, dtype=torch.float32, device="cuda")
        out = buf[1:self.T + 1, :self.n]
        got = qg.gemm_w4a8_moe_down(self.a, self.b, self.ids, self.w if isinstance(w, str) else w, self.T, self.n_used,
                                    self.n, self.k, self.t, out=out)
        assert got.data_ptr() == out.data_ptr()
        whole = host(buf)
        return whole[1:self.T + 1, :self.n].copy(), whole

    def dead_tokens(self):
        return [tt for tt in range(self.T) if not ((0 <= self.ids_h[tt, :self.n_used]) & (self.ids_h[tt, :self.n_used] < self.n_expert)).any()]

    def check(self, qg, pad=None, what=""):
        pad = 1 + (3 * self.n + self.T + self.k // 32) % 29 if pad is None else pad
        cfg = qg.moe_down_config(self.T, self.n_used, self.n, self.k, self.t)
        c, whole = self.launch_guarded(qg, pad)
        outside = np.ones(whole.shape, bool)
        outside[1:-1, :self.n] = False
        assert (whole[outside] == np.float32(F_SENT)).all(), f"wrote outside the tokens' rows (ldc = {self.n + pad}, {cfg})"
        ref = self.reference(qg)
        diff = np.argwhere(bits(c) != bits(ref))
        assert diff.size == 0, (f"{len(diff)} of {c.size} outputs differ from the fold of the decode entry's products, first "
                                f"{diff[:4].tolist()} ({cfg} T={self.T} n_used={self.n_used} N={self.n} {what})")
        assert np.isfinite(c).all()  # the NaN and inf weights of the out-of-range slots reached nothing
        for tt in self.dead_tokens():
            assert (bits(c[tt]) == 0).all(), tt  # +0.0f, not -0.0f
        _, again = self.launch_guarded(qg, pad)
        assert np.array_equal(bits(whole), bits(again))
        # weights = None: the plain sum, bit-equal to passing ones
        import torch
        none = self.launch_guarded(qg, pad, w=None)[0]
        ones = self.launch_guarded(qg, pad, w=torch.ones((self.T, self.n_used), dtype=torch.float32, device="cuda"))[0]
        assert np.array_equal(bits(none), bits(ones)) and np.array_equal(bits(none), bits(self.reference(qg, weights=False)))
        return c


# ---------------------------------------------------------------------------- 1. every form x row edge x slot count
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("k", KQ_K)
def test_every_form_row_edge_and_slot_count(qg, t, k):
    """Each (LPR, ONE) at N = 1 and one either side of a workgroup's rows and at exactly its rows (RPB read from the
    config line, whose LPR / WGS / ONE must be the decode entry's), at n_used = 1, 2, 3, 8, 9 and T = 1, 3; and at
    n_used = 16 where the workgroup has 16 waves, the one SW the list above does not reach."""
    for n_used in N_USED + ((16,) if k >= 4096 else ()):
        f = DR.launch(qg.moe_down_config(1, n_used, 1, k, t))
        ref = MR.cfg_fields(qg.moe_config(1, n_used, 1, k, t))[1]
        assert (f["LPR"], f["WGS"], f["ONE"]) == (int(ref["LPR"]), int(ref["WGS"]), int(ref["ONE"]))
        rpb = f["RPB"]
        for n in sorted({1, max(1, rpb - 1), rpb, rpb + 1}):
            for T in (1, 3):
                g = DR.launch(qg.moe_down_config(T, n_used, n, k, t))
                assert g["grid"] == f"{(n + rpb - 1) // rpb}x{T}" and g["lds"] == DR.lds_bytes(t, n_used, k, rpb)
                assert (g["LPR"], g["ONE"], g["SW"]) == (f["LPR"], f["ONE"], f["SW"])
                Step(t, T, n_used, n, k).check(qg)


@pytest.mark.parametrize("t", TYPES)
def test_the_forms_the_shape_list_reaches(qg, t):
    """The (LPR, ONE, SW) of the launches above (each asserted there to be its shape's config line): every (LPR, ONE)
    with SW = the largest power of two <= min(n_used, WGS / 64) for the list's n_used."""
    seen = set()
    for k in KQ_K:
        for n_used in N_USED + ((16,) if k >= 4096 else ()):
            f = DR.launch(qg.moe_down_config(3, n_used, 5, k, t))
            seen.add((f["LPR"], f["ONE"], f["SW"]))
    want = {(lpr, one, sw) for lpr, sws in ((4, (1, 2, 4)), (16, (1, 2, 8)), (64, (1, 2, 8, 16))) for sw in sws for one in (0, 1)}
    assert seen == want, (sorted(seen - want), sorted(want - seen))


@pytest.mark.parametrize("t", TYPES)
def test_token_without_a_valid_id_and_many_row_tiles(qg, t):
    """A token whose ids all name no expert is N times the bit pattern 0 whatever its weights hold; more than one
    dispatch of row tiles per token (N = 40 RPB + 3)."""
    n_expert, n_used, T, k = 4, 3, 3, 1024
    ids = np.array([[0, 1, 2, 3], [-1, n_expert, 2 ** 31 - 1, 0], [3, -2 ** 31, 3, 1]], np.int32)
    rpb = DR.launch(qg.moe_down_config(T, n_used, 1, k, t))["RPB"]
    s = Step(t, T, n_used, 40 * rpb + 3, k, n_expert=n_expert, ids=ids)
    assert s.dead_tokens() == [1] and not np.isfinite(s.w_h[1, :n_used]).any()
    c = s.check(qg)
    assert (bits(c[1]) == 0).all() and (c[0] != 0).any() and (c[2] != 0).any()


# ---------------------------------------------------------------------------- 2. against the independent models
@pytest.mark.parametrize("t", TYPES)
def test_against_the_model(qg, t):
    """|c - sum_u w_u D_u| <= sum_u |w_u| tol_u + 2^-23 (2 n_used) sum_u |w_u D_u|: D_u the float64 model of slot u's
    product, tol_u its decode GEMV bound (W = 0); every multiplication and addition of the fold one rounding."""
    R = MR.KR if t == Q4_K else MR.QR
    s = Step(t, 3, 3, 37, 1024)
    c = s.check(qg)
    for tt in range(s.T):
        want, bound, mag = np.zeros(s.n), np.zeros(s.n), np.zeros(s.n)
        for u in range(s.n_used):
            e = int(s.ids_h[tt, u])
            if not 0 <= e < s.n_expert:
                continue
            D, _, m = R.gemm(s.a_h[tt, u].reshape(1, -1, 36), s.b_h[e])
            w = float(s.w_h[tt, u])
            want += w * D[0]
            bound += abs(w) * R.tol(m, s.k, 0)[0]
            mag += np.abs(w * D[0])
        err = np.abs(c[tt].astype(np.float64) - want)
        lim = bound + 2.0 ** -23 * 2 * s.n_used * mag
        assert (err <= lim).all(), float((err / lim).max())


# ---------------------------------------------------------------------------- 3. the ends of the formats
@pytest.mark.parametrize("t", TYPES)
def test_extremes(qg, t):
    """Experts and activation rows from the reference module's extremes(): expert 0 holds the extreme classes, one per
    row; slots (0, 0), (0, 1) and (1, 0) are the extreme activation rows. Finite products, the fold bit for bit."""
    R = MR.KR if t == Q4_K else MR.QR
    n, n_expert, k, T, n_used = 16, 2, 512, 3, 2
    aq, bq = R.extremes(np.random.default_rng([t, 2025]), T * n_used + 2, n * n_expert, k)
    ids = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 1]], np.int32)
    s = Step(t, T, n_used, n, k, n_expert=n_expert, ids=ids, data=(bq.reshape((n_expert, n) + bq.shape[1:]), aq))
    d = s.products(qg)
    assert np.isfinite(d).all()
    print(f"extremes t={t}: |d| up to {np.abs(d).max():.3g}, smallest nonzero |d| {np.abs(d[d != 0]).min():.3g}")
    assert np.isfinite(s.check(qg, what="extremes")).all()


# ---------------------------------------------------------------------------- 4. capture
@pytest.mark.parametrize("t", TYPES)
def test_captured_one_node_follows_the_ids_and_the_weights(qg, t):
    """GEMV, down, GEMV in one graph: the fused call is one kernel node of its own between the two GEMV nodes (without
    it they merge into one; with it the merge counts two GEMV nodes, nothing merged, nothing absorbed), and a replay
    follows the ids and the weights it finds in the buffers."""
    import torch
    qg.set_capture_fusion(1)
    s = Step(t, 3, 3, 33, 1024)
    gk, gn = 4096, 64
    rng = np.random.default_rng(79)
    gw, ga = dev(MR.random_experts(rng, MR.Q4_0, 2, gn, gk)), dev(MR.random_act(rng, 1, gk))
    gout = torch.zeros((2, 1, gn), dtype=torch.float32, device="cuda")
    mout = torch.zeros((s.T, s.n), dtype=torch.float32, device="cuda")
    ids2_h = ((s.ids_h[:, ::-1] + 1) % s.n_expert).astype(np.int32).copy()
    ids2_h[0, 0] = s.n_expert  # an id out of range that was in range on the first replay
    w2_h = (s.w_h[::-1] * np.float32(0.5) + np.float32(0.25)).astype(np.float32).copy()
    w2_h[~np.isfinite(w2_h)] = 0.75  # finite everywhere: ids2 has other slots out of range than the weights' NaN
    w1_h = np.where(np.isfinite(s.w_h), s.w_h, np.float32(-0.5)).astype(np.float32)

    def load(ids_h, w_h):
        s.ids_full.copy_(dev(ids_h))  # in place: the graph holds the pointers
        s.w_full.copy_(dev(w_h))

    def eager(ids_h, w_h):
        load(ids_h, w_h)
        return host(qg.gemm_w4a8_moe_down(s.a, s.b, s.ids, s.w, s.T, s.n_used, s.n, s.k, t)).copy()

    combos = [(i, w) for i in (s.ids_h, ids2_h) for w in (w1_h, w2_h)]
    refs = [eager(i, w) for i, w in combos]
    for x in range(4):
        for y in range(x):
            assert not np.array_equal(bits(refs[x]), bits(refs[y]))

    def step(with_down):
        qg.gemm_w4a8(ga, gw[0], 1, gn, gk, MR.Q4_0, out=gout[0])
        if with_down:
            qg.gemm_w4a8_moe_down(s.a, s.b, s.ids, s.w, s.T, s.n_used, s.n, s.k, t, out=mout)
        qg.gemm_w4a8(ga, gw[1], 1, gn, gk, MR.Q4_0, out=gout[1])

    graphs = {}
    for with_down in (False, True):
        torch.cuda.synchronize()
        s0 = qg.capture_fusion_stats()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step(with_down)
        s1 = qg.capture_fusion_stats()
        graphs[with_down] = (g, (s1[0] - s0[0], s1[1] - s0[1]))
    assert graphs[False][1] == (1, 1)
    assert graphs[True][1] == (0, 2)
    g = graphs[True][0]
    for (ids_h, w_h), ref in zip(combos, refs):
        load(ids_h, w_h)
        mout.fill_(F_SENT)
        g.replay()
        assert np.array_equal(bits(host(mout)), bits(ref))


# ---------------------------------------------------------------------------- 5. pointers
@pytest.mark.parametrize("t", TYPES)
def test_weights_at_the_alignment_classes(qg, t):
    """The experts at the type's smallest offset past a 256-B line, inside a buffer of 0xFF bytes, then of 0x00: the
    checks hold and the surrounding bytes reach no result."""
    off = {Q4_K: 16, Q6_K: 2}[t]
    res = []
    for fill in (0xFF, 0x00):
        s = Step(t, 3, 3, 19, 768, woff=off, fill=fill)
        assert s.b.data_ptr() % 256 == off
        res.append(s.check(qg))
    assert np.array_equal(bits(res[0]), bits(res[1]))


# ---------------------------------------------------------------------------- 6. the C ABI, the view entry, Python
def views(G, s, out, lead=False):
    bb, row = MR.BB[s.t], MR.expert_bytes(s.t, 1, s.k)
    arow = s.k // 32 * 36
    w, a, i, r, o = G.TensorView(), G.TensorView(), G.TensorView(), G.TensorView(), G.TensorView()
    w.data, w.type = s.b.data_ptr(), s.t
    w.ne[:], w.nb[:] = [s.k, s.n, s.n_expert, 1], [bb, row, row * s.n, row * s.n * s.n_expert]
    a.data, a.type = s.a.data_ptr(), G.Q8_1
    a.ne[:], a.nb[:] = [s.k, s.n_used, s.T, 1], [36, arow, arow * s.n_used, arow * s.n_used * s.T]
    i.data, i.type = s.ids.data_ptr(), G.I32
    st = s.ids.stride(0)
    i.ne[:], i.nb[:] = [s.n_used, s.T, 1, 1], [4, 4 * st, 4 * st * s.T, 4 * st * s.T]
    r.data, r.type = s.w.data_ptr(), G.F32
    st = s.w.stride(0)
    if lead:  # ggml's [1, n_used, T]
        r.ne[:], r.nb[:] = [1, s.n_used, s.T, 1], [4, 4, 4 * st, 4 * st * s.T]
    else:
        r.ne[:], r.nb[:] = [s.n_used, s.T, 1, 1], [4, 4 * st, 4 * st * s.T, 4 * st * s.T]
    o.data, o.type = out.data_ptr(), G.F32
    o.ne[:], o.nb[:] = [s.n, s.T, 1, 1], [4, 4 * out.stride(0), 4 * out.stride(0) * s.T, 4 * out.stride(0) * s.T]
    return w, a, i, r, o


@pytest.mark.parametrize("t", TYPES)
def test_c_abi_view_entry_and_python_agree(qg, t):
    import torch
    import quant_gemm._lib as L
    import quant_gemm.ggml as G
    P = ctypes.c_void_p
    s = Step(t, 3, 3, 21, 512, n_expert=16)
    assert s.ids.stride(0) == 16 and s.w.stride(0) == 6 and not s.ids.is_contiguous() and not s.w.is_contiguous()
    py = host(qg.gemm_w4a8_moe_down(s.a, s.b, s.ids, s.w, s.T, s.n_used, s.n, s.k, t)).copy()
    assert py.shape == (s.T, s.n) and np.array_equal(bits(py), bits(s.reference(qg)))
    py_none = host(qg.gemm_w4a8_moe_down(s.a, s.b, s.ids, None, s.T, s.n_used, s.n, s.k, t)).copy()
    assert np.array_equal(bits(py_none), bits(s.reference(qg, weights=False)))
    # the C ABI on raw pointers, ldc > N
    buf = torch.full((s.T, s.n + 3), F_SENT, dtype=torch.float32, device="cuda")
    st = P(torch.cuda.current_stream().cuda_stream)
    call = lambda k=s.k, boff=0, woff=0, ldc=s.n + 3, w_stride=6, ids_stride=16, wt=t, w=True: L.load().qg_gemm_w4a8_moe_down(
        P(s.a.data_ptr()), P(s.b.data_ptr() + boff), s.n_expert, P(s.ids_full.data_ptr()), ids_stride,
        P(s.w_full.data_ptr() + woff) if w else None, w_stride, P(buf.data_ptr()), ldc, s.T, s.n_used, s.n, k, wt, st)
    # refusals on real buffers: the output untouched
    assert call(k=s.k - 32) == -2 and call(boff=1) == -4 and call(woff=2) == -4 and call(ldc=s.n - 1) == -1
    assert call(w_stride=s.n_used - 1) == -1 and call(ids_stride=s.n_used - 1) == -1 and call(wt=MR.Q4_0) == -3
    assert call(k=(160 * 1024 // MR.KQ_REC_BYTES[t] // s.n_used + 1) * 256) == -3
    assert (host(buf) == F_SENT).all()
    assert call() == 0
    got = host(buf)
    assert np.array_equal(bits(got[:, :s.n]), bits(py)) and (got[:, s.n:] == F_SENT).all()
    buf.fill_(F_SENT)
    assert call(w=False, w_stride=0) == 0
    got = host(buf)
    assert np.array_equal(bits(got[:, :s.n]), bits(py_none)) and (got[:, s.n:] == F_SENT).all()
    # the view entry: weights [n_used, T], [1, n_used, T] and none
    out = buf[:, :s.n]
    for lead, want in ((False, py), (True, py), (None, py_none)):
        buf.fill_(F_SENT)
        w, a, i, r, o = views(G, s, out, bool(lead))
        G.mul_mat_id_down_from_ggml(w, a, i, None if lead is None else r, o)
        got = host(buf)
        assert np.array_equal(bits(got[:, :s.n]), bits(want)) and (got[:, s.n:] == F_SENT).all(), lead
    # views the entry cannot express: refused, the output untouched
    buf.fill_(F_SENT)
    arow = s.k // 32 * 36
    for spoil, code in (("act_rows", "unsupported"), ("weights_type", "unsupported"), ("weights_stride", "unsupported"),
                        ("weights_dims", "invalid"), ("expert_stride", "unsupported"), ("ids_type", "unsupported"),
                        ("out_slots", "unsupported"), ("out_tokens", "invalid"), ("row_type", "unsupported")):
        w, a, i, r, o = views(G, s, out)
        if spoil == "act_rows":      # b.ne[1] != n_used: one row per token is the gate / up product's
            a.ne[1], a.nb[2], a.nb[3] = 1, arow, arow * s.T
        elif spoil == "weights_type":
            r.type = G.I32
        elif spoil == "weights_stride":
            r.nb[0] = 8
        elif spoil == "weights_dims":
            r.ne[0] = s.n_used - 1
        elif spoil == "expert_stride":
            w.nb[2] += MR.BB[t]
        elif spoil == "ids_type":
            i.type = G.F32
        elif spoil == "out_slots":   # a row per slot is qg_mul_mat_id_from_view's output
            o.ne[1], o.ne[2] = s.n_used, s.T
        elif spoil == "out_tokens":
            o.ne[1] = s.T - 1
        else:
            w.type = MR.Q8_0
        with pytest.raises(RuntimeError, match=code):
            G.mul_mat_id_down_from_ggml(w, a, i, r, o)
    assert (host(buf) == F_SENT).all()
    with pytest.raises(RuntimeError):
        qg.gemm_w4a8_moe_down(s.a, s.b, s.ids, s.w, s.T, s.n_used, s.n, s.k, MR.Q4_0)
    with pytest.raises(RuntimeError):
        qg.gemm_w4a8_moe_down(s.a, s.b, s.ids, s.w.double(), s.T, s.n_used, s.n, s.k, t)
    with pytest.raises(RuntimeError):
        qg.gemm_w4a8_moe_down(s.a[:, :2], s.b, s.ids, s.w, s.T, s.n_used, s.n, s.k, t)
    assert (host(buf) == F_SENT).all()
