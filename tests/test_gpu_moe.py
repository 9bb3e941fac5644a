"""qg_gemm_w4a8_moe on the GPU: one launch for the T * n_used expert products of a decode step, the ids read on the
device, for all seven weight types.

The reference of every case is the library's own eager single call per slot, qg.gemm_w4a8(row, expert, 1, N, K, t), on
pointers computed on the host, compared as uint32; a slot whose id is outside [0, n_expert) must be N times the bit
pattern 0. One case per type is also held against the NumPy contract / the C oracle (moe_ref.assert_close_to_model,
W = 0), so the module does not rest on the library alone. Outputs go through out= into the interior of a
sentinel-filled [slots + 2, N + pad] buffer (ldc > N, a guard row before and after): the sentinels must survive, and
a second launch must give the same buffer bit for bit.

The ids live in a [T, ids_stride] int32 tensor with ids_stride > n_used whose unused columns hold other valid ids, and
the activations of a_rows = 1 cases in a buffer with n_used spare rows, so a kernel that used n_used for the ids
stride, or u for u % a_rows, would read other but allocated memory and give other bits. The expert offset beyond 4 GiB
is reached in test_expert_beyond_4_gib.
"""
import ctypes
import functools

import numpy as np
import pytest

import moe_ref as MR
from moe_ref import ALL_TYPES, Q4_0, Q4_K, Q6_K, Q8_0, ROW_TYPES

pytestmark = pytest.mark.gpu

F_SENT = -12345.0
KQ_K = (256, 1024, 4096, 2304, 4352)          # LPR 4 / 16 / 64 loop-free, then the unit loop at 16 and 64 lanes
ROW_K = KQ_K + (8192,)                        # the row GEMV: 4096 loop-free, 8192 its loop (Q4_0: two units per lane)
SLOTS = [(1, 1), (1, 8), (3, 2), (8, 8), (9, 8)]  # 72 slots in the last: no cap at 64 items


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def make_ids(rng, T, n_used, n_expert, bad=True):
    """int32 [T, ids_stride], ids_stride = max(n_expert, n_used + 1) > n_used, every column a valid id; ids repeated
    inside a token and across tokens; with `bad`, -1 and n_expert in the middle of the step."""
    stride = max(n_expert, n_used + 1)
    ids = rng.integers(0, n_expert, (T, stride)).astype(np.int32)
    slots = T * n_used
    if bad and slots >= 3:
        for s, v in ((slots // 2, -1), (slots // 2 - 1 if slots < 6 else slots // 3, n_expert)):
            ids[s // n_used, s % n_used] = v
    if n_used >= 2:
        ids[0, 1] = ids[0, 0]                 # (slots 0 and 1 are never the out-of-range ones from 6 slots on)
    if T >= 2:
        ids[T - 1, n_used - 1] = ids[0, 0]    # the last slot never is
    return ids


@functools.lru_cache(maxsize=None)
def operands(t, n_expert, n, k, rows, seed=0):
    """Experts [n_expert, n, ..] and `rows` activation rows of one shape, made once and never modified."""
    rng = np.random.default_rng([t, n_expert, n, k, rows, seed])
    return MR.random_experts(rng, t, n_expert, n, k), MR.random_act(rng, rows, k)


class Step:
    """One decode step on the device. a holds T * a_rows rows followed by n_used spare ones."""

    def __init__(self, t, T, n_used, n_expert, n, k, a_rows, seed=0, woff=None, fill=0, ids=None, bad=True):
        self.t, self.T, self.n_used, self.n_expert, self.n, self.k, self.a_rows = t, T, n_used, n_expert, n, k, a_rows
        self.w_h, a_all = operands(t, n_expert, n, k, T * n_used + n_used, seed)
        self.a_h = a_all[:T * a_rows].reshape(T, a_rows, k // 32, 36)
        self.ids_h = make_ids(np.random.default_rng([seed, T, n_used, n_expert]), T, n_used, n_expert, bad) if ids is None else ids
        self.w = dev(self.w_h) if woff is None else MR.KR.dev_at(self.w_h, woff, fill)
        self.a_all = dev(a_all[:T * a_rows + n_used])
        self.a = self.a_all[:T * a_rows].reshape(T, a_rows, k // 32, 36)
        self.ids_full = dev(self.ids_h)
        self.ids = self.ids_full[:, :n_used]
        self._eager = {}

    def eager_slot(self, qg, row, e):
        """The single call on host-computed pointers, once per (activation row, expert)."""
        if (row, e) not in self._eager:
            a = self.a_all[row:row + 1]
            self._eager[row, e] = host(qg.gemm_w4a8(a, self.w[e], 1, self.n, self.k, self.t))[0].copy()
        return self._eager[row, e]

    def reference(self, qg, ids=None):
        ids = self.ids_h if ids is None else ids
        ref = np.zeros((self.T, self.n_used, self.n), np.float32)
        for tt in range(self.T):
            for u in range(self.n_used):
                e = int(ids[tt, u])
                if 0 <= e < self.n_expert:
                    ref[tt, u] = self.eager_slot(qg, tt * self.a_rows + u % self.a_rows, e)
        return ref

    def launch_guarded(self, qg, pad):
        """(window [T, n_used, N], whole buffer): out= the interior of a sentinel-filled [slots + 2, N + pad] buffer."""
        import torch
        S = self.T * self.n_used
        buf = torch.full((S + 2, self.n + pad), F_SENT, dtype=torch.float32, device="cuda")
        out = buf[1:S + 1, :self.n].unflatten(0, (self.T, self.n_used))
        got = qg.gemm_w4a8_moe(self.a, self.w, self.ids, self.T, self.n_used, self.n, self.k, self.t, a_rows=self.a_rows, out=out)
        assert got.data_ptr() == out.data_ptr()
        whole = host(buf)
        return whole[1:S + 1, :self.n].reshape(self.T, self.n_used, self.n).copy(), whole

    def check(self, qg, pad=None):
        pad = 1 + (3 * self.n + self.T + self.k // 32) % 29 if pad is None else pad
        c, whole = self.launch_guarded(qg, pad)
        outside = np.ones(whole.shape, bool)
        outside[1:-1, :self.n] = False
        assert (whole[outside] == np.float32(F_SENT)).all(), f"wrote outside the slots' rows (ldc = {self.n + pad})"
        ref = self.reference(qg)
        bad = [(tt, u) for tt in range(self.T) for u in range(self.n_used) if not 0 <= self.ids_h[tt, u] < self.n_expert]
        for tt, u in bad:
            assert (bits(c[tt, u]) == 0).all(), (tt, u)  # +0.0f, not -0.0f, not the sentinel
        diff = [(tt, u) for tt in range(self.T) for u in range(self.n_used) if not np.array_equal(bits(c[tt, u]), bits(ref[tt, u]))]
        assert not diff, f"slots {diff[:6]} differ from the eager single call ({qg.moe_config(self.T, self.n_used, self.n, self.k, self.t)})"
        _, again = self.launch_guarded(qg, pad)
        assert np.array_equal(bits(whole), bits(again))
        return c


def rows_per_workgroup(cfg):
    fam, f = MR.cfg_fields(cfg)
    return int(f["WGS"]) // 64 * (64 // int(f["LPR"])) * int(f.get("TPW", 1))


# ---------------------------------------------------------------------------- 1. every type x form x row edge
@pytest.mark.parametrize("t,k", [(t, k) for t in ALL_TYPES for k in (ROW_K if t in ROW_TYPES else KQ_K)])
def test_every_form_and_row_edge(qg, t, k):
    """Each LPR class, loop-free and with the unit loop, at N = 1 and one either side of a workgroup's rows (read from
    qg_moe_config, which names the single call's family and LPR / BPL / ONE(U)); a_rows 1 and n_used in turn."""
    cfg = qg.moe_config(3, 2, 1, k, t)
    assert MR.kernel_choice(cfg) == MR.kernel_choice(qg.debug_config(1, 1, k, t)), cfg
    rpb = rows_per_workgroup(cfg)
    for i, n in enumerate((1, rpb - 1, rpb + 1)):
        assert MR.cfg_fields(qg.moe_config(3, 2, n, k, t))[1]["grid"] == f"{(n + rpb - 1) // rpb}x6"
        Step(t, 3, 2, 4, n, k, a_rows=(1, 2)[i % 2]).check(qg)


def test_full_size_workgroups_and_linear_tile_order(qg):
    """The loop-free row form takes half-size workgroups while N fits one round of full-size ones and full-size ones
    beyond (the threshold read from the device's CU count; of two row tiles, Q8_0 of one); past 512 row tiles every kernel takes the linear tile
    order. Short rows keep the tensors small."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for t, k, rpb_full in [(t, 128, 128) for t in ROW_TYPES] + [(Q4_0, 4096, 32)]:
        n = cus * rpb_full
        half, full = qg.moe_config(2, 2, n, k, t), qg.moe_config(2, 2, n + 1, k, t)
        hf, ff = MR.cfg_fields(half)[1], MR.cfg_fields(full)[1]
        assert int(hf["WGS"]) * 2 == int(ff["WGS"]) and hf["TPW"] == "2" and ff["TPW"] == ("1" if t == Q8_0 else "2"), (half, full)
        assert hf["grid"] == f"{-(-n // rows_per_workgroup(half))}x4" and ff["grid"] == f"{-(-(n + 1) // rows_per_workgroup(full))}x4"
        Step(t, 2, 2, 2, n + 1, k, a_rows=2, bad=False).check(qg)
    for t, k, rpb in ((Q4_0, 128, 128), (Q4_K, 256, 64), (Q6_K, 256, 64)):
        n = 513 * rpb + 1
        assert MR.cfg_fields(qg.moe_config(1, 3, n, k, t))[1]["grid"] == "514x3"
        Step(t, 1, 3, 2, n, k, a_rows=1).check(qg)


# ---------------------------------------------------------------------------- 2. slot counts, ids, activations
@pytest.mark.parametrize("t", ALL_TYPES)
@pytest.mark.parametrize("T,n_used", SLOTS)
def test_slot_counts(qg, t, T, n_used):
    """n_expert 4 and 16, a_rows 1 and n_used, ids_stride > n_used, ids repeated in and across tokens, -1 and
    n_expert in the middle of the step with their neighbours unaffected."""
    for n_expert in (4, 16):
        for a_rows in {1, n_used}:
            Step(t, T, n_used, n_expert, 33, 512, a_rows).check(qg)


# ---------------------------------------------------------------------------- 3. against the models
@pytest.mark.parametrize("t", ALL_TYPES)
def test_against_the_model(qg, O, t):
    s = Step(t, 3, 2, 4, 37, 1024, a_rows=2)
    c = s.check(qg)
    live = 0
    for tt in range(s.T):
        for u in range(s.n_used):
            e = int(s.ids_h[tt, u])
            if 0 <= e < s.n_expert:
                MR.assert_close_to_model(O, c[tt, u], s.a_h[tt, u], s.w_h[e], t)
                live += 1
    assert live >= 4


# ---------------------------------------------------------------------------- 4. what surrounds the expert tensor
@pytest.mark.parametrize("t", ALL_TYPES)
def test_bytes_around_the_experts_reach_no_result(qg, t):
    """The expert tensor inside a buffer of 0xFF bytes, then of 0x00, at the type's smallest offset: the same bits."""
    off = {Q4_K: 16, Q6_K: 2}.get(t, 4)
    res = []
    for fill in (0xFF, 0x00):
        s = Step(t, 3, 2, 4, 19, 768 if t in (Q4_K, Q6_K) else 576, a_rows=1, woff=off, fill=fill)
        assert s.w.data_ptr() % 256 == off
        res.append(s.check(qg))
    assert np.array_equal(bits(res[0]), bits(res[1]))


@pytest.mark.parametrize("n,k", [(5, 768), (3, 256), (7, 4352)])
def test_q6k_experts_of_alternating_parity(qg, n, k):
    """Q6_K experts 2 B off a dword with an odd number of super-blocks per expert: consecutive experts alternate
    between the two parities the kernel realigns."""
    assert (n * k // 256) % 2 == 1 and MR.expert_bytes(Q6_K, n, k) % 4 == 2
    s = Step(Q6_K, 3, 2, 4, n, k, a_rows=2, woff=2, ids=np.array([[0, 1, 2], [3, 2, 1], [1, -1, 3]], np.int32))
    assert s.w.data_ptr() % 4 == 2
    s.check(qg)


# ---------------------------------------------------------------------------- 5. an expert beyond 4 GiB
def test_expert_beyond_4_gib(qg):
    """Q8_0, N = K = 4096, 256 experts of 17 MiB: expert 255 starts 4.5e9 bytes past the base. The tensor is
    torch.empty; only the two selected experts are written."""
    import torch
    t, n, k, n_expert = Q8_0, 4096, 4096, 256
    per = MR.expert_bytes(t, n, k)
    sel = (255, 1)
    assert sel[0] * per > 2 ** 32
    rng = np.random.default_rng(4096)
    w = torch.empty((n_expert, n, k // 32, 34), dtype=torch.uint8, device="cuda")
    w_h = {e: MR.random_experts(rng, t, 1, n, k)[0] for e in sel}
    for e in sel:
        w[e].copy_(dev(w_h[e]))
    a_h = MR.random_act(rng, 1, k)
    a = dev(np.concatenate([a_h, a_h, a_h]))[:1].reshape(1, 1, k // 32, 36)
    ids = torch.tensor([[sel[0], sel[1], 7]], dtype=torch.int32, device="cuda")
    buf = torch.full((4, n + 5), F_SENT, dtype=torch.float32, device="cuda")
    out = buf[1:3, :n].unflatten(0, (1, 2))
    qg.gemm_w4a8_moe(a, w, ids[:, :2], 1, 2, n, k, t, out=out)
    got = host(buf)
    for u, e in enumerate(sel):
        want = host(qg.gemm_w4a8(a[0], w[e], 1, n, k, t))[0]
        assert np.array_equal(bits(got[1 + u, :n]), bits(want)), e
    assert (got[0] == F_SENT).all() and (got[3] == F_SENT).all() and (got[:, n:] == F_SENT).all()
    del w


# ---------------------------------------------------------------------------- 6. capture
@pytest.mark.parametrize("t", [Q4_0, Q4_K, Q6_K])
def test_captured_between_two_gemvs(qg, t):
    """GEMV, MoE, GEMV in one graph: the MoE call is a kernel node of its own, the GEMVs around it do not merge across
    it (without it they do), and a replay follows the ids it finds in the buffer."""
    import torch
    qg.set_capture_fusion(1)
    s = Step(t, 3, 2, 4, 33, 1024, a_rows=1)
    gk, gn = 4096, 64
    rng = np.random.default_rng(77)
    gw, ga = dev(MR.random_experts(rng, Q4_0, 2, gn, gk)), dev(MR.random_act(rng, 1, gk))
    gout = torch.zeros((2, 1, gn), dtype=torch.float32, device="cuda")
    mout = torch.zeros((s.T, s.n_used, s.n), dtype=torch.float32, device="cuda")
    gref = [host(qg.gemm_w4a8(ga, gw[i], 1, gn, gk, Q4_0)) for i in range(2)]
    ids2_h = ((s.ids_h[:, ::-1] + 1) % s.n_expert).astype(np.int32).copy()
    ids2_h[0, 0] = s.n_expert  # and an id out of range that was in range on the first replay
    ref1, ref2 = s.reference(qg), s.reference(qg, ids2_h)
    assert not np.array_equal(bits(ref1), bits(ref2))

    def step(with_moe):
        qg.gemm_w4a8(ga, gw[0], 1, gn, gk, Q4_0, out=gout[0])
        if with_moe:
            qg.gemm_w4a8_moe(s.a, s.w, s.ids, s.T, s.n_used, s.n, s.k, t, a_rows=1, out=mout)
        qg.gemm_w4a8(ga, gw[1], 1, gn, gk, Q4_0, out=gout[1])

    graphs = {}
    for with_moe in (False, True):
        torch.cuda.synchronize()
        s0 = qg.capture_fusion_stats()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step(with_moe)
        s1 = qg.capture_fusion_stats()
        graphs[with_moe] = (g, (s1[0] - s0[0], s1[1] - s0[1]))
    assert graphs[False][1] == (1, 1)  # back to back: one merged node
    assert graphs[True][1] == (0, 2)   # the MoE node between them: two GEMV nodes, nothing merged, nothing absorbed
    g = graphs[True][0]
    for ids_h, ref in ((s.ids_h, ref1), (ids2_h, ref2)):
        s.ids_full.copy_(dev(ids_h))  # in place: the graph holds the pointer
        gout.zero_()
        mout.fill_(F_SENT)
        g.replay()
        assert np.array_equal(bits(host(mout)), bits(ref))
        for i in range(2):
            assert np.array_equal(bits(host(gout[i])), bits(gref[i]))
    assert qg.capture_fusion_stats() == s1


# ---------------------------------------------------------------------------- 7. views and refusals
def views(G, s, out, ids=None):
    ids = s.ids if ids is None else ids
    bb, row = MR.BB[s.t], MR.expert_bytes(s.t, 1, s.k)
    w, a, i, o = G.TensorView(), G.TensorView(), G.TensorView(), G.TensorView()
    w.data, w.type = s.w.data_ptr(), s.t
    w.ne[:], w.nb[:] = [s.k, s.n, s.n_expert, 1], [bb, row, row * s.n, row * s.n * s.n_expert]
    arow = s.k // 32 * 36
    a.data, a.type = s.a.data_ptr(), G.Q8_1
    a.ne[:], a.nb[:] = [s.k, s.a_rows, s.T, 1], [36, arow, arow * s.a_rows, arow * s.a_rows * s.T]
    i.data, i.type = ids.data_ptr(), G.I32
    i.ne[:], i.nb[:] = [s.n_used, s.T, 1, 1], [4, 4 * ids.stride(0), 4 * ids.stride(0) * s.T, 4 * ids.stride(0) * s.T]
    o.data, o.type = out.data_ptr(), G.F32
    o.ne[:], o.nb[:] = [s.n, s.n_used, s.T, 1], [4, 4 * out.stride(1), 4 * out.stride(0), 4 * out.stride(0) * s.T]
    return w, a, i, o


@pytest.mark.parametrize("t", [Q4_0, Q8_0, Q4_K, Q6_K])
def test_view_entry_on_a_strided_ids_view(qg, t):
    import torch
    import quant_gemm.ggml as G
    s = Step(t, 3, 2, 16, 21, 512, a_rows=2)
    assert s.ids.stride(0) == 16 and not s.ids.is_contiguous()
    ref = s.reference(qg)
    buf = torch.full((s.T, s.n_used, s.n + 3), F_SENT, dtype=torch.float32, device="cuda")
    out = buf[:, :, :s.n]
    w, a, i, o = views(G, s, out)
    G.mul_mat_id_from_ggml(w, a, i, o)
    got = host(buf)
    assert np.array_equal(bits(got[:, :, :s.n]), bits(ref)) and (got[:, :, s.n:] == F_SENT).all()
    # views the entry cannot express: refused, the output untouched
    buf.fill_(F_SENT)
    for spoil in ("expert_stride", "ids_bytes", "ne3", "act_rows", "ids_type"):
        w, a, i, o = views(G, s, out)
        if spoil == "expert_stride":
            w.nb[2] += MR.BB[t]
        elif spoil == "ids_bytes":
            i.nb[1] += 2
        elif spoil == "ne3":
            o.ne[3] = 2
        elif spoil == "act_rows":
            a.nb[1] += 36
        else:
            i.type = G.F32
        with pytest.raises(RuntimeError, match="unsupported"):
            G.mul_mat_id_from_ggml(w, a, i, o)
    assert (host(buf) == F_SENT).all()


@pytest.mark.parametrize("t", [Q4_0, Q6_K])
def test_refusals_on_real_buffers(qg, t):
    """Odd K/32 (the row types; for Q6_K a K off its granule) and a weights pointer off the type's alignment: refused
    by the C entry with the output untouched."""
    import torch
    import quant_gemm._lib as L
    P = ctypes.c_void_p
    s = Step(t, 2, 2, 4, 9, 512, a_rows=1)
    out = torch.full((s.T, s.n_used, s.n), F_SENT, dtype=torch.float32, device="cuda")
    st = P(torch.cuda.current_stream().cuda_stream)
    call = lambda k, woff=0, ldc=0: L.load().qg_gemm_w4a8_moe(
        P(s.a.data_ptr()), 1, P(s.w.data_ptr() + woff), s.n_expert, P(s.ids_full.data_ptr()), s.ids_full.stride(0),
        P(out.data_ptr()), ldc, s.T, s.n_used, s.n, k, t, st)
    assert call(512 - 32) == (-3 if t == Q4_0 else -2)
    assert call(512, woff=2 if t == Q4_0 else 1) == -4
    assert call(512, ldc=s.n - 1) == -1
    assert (host(out) == F_SENT).all()
    assert call(512) == 0
    assert np.array_equal(bits(host(out)), bits(s.reference(qg)))


# ---------------------------------------------------------------------------- 8. seeded sweep
def sweep_cases(count=24, seed=1507):
    rng = np.random.default_rng(seed)
    for i in range(count):
        t = ALL_TYPES[i % len(ALL_TYPES)]
        T, n_used = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        g = 256 if t in (Q4_K, Q6_K) else 64
        yield (i, t, T, n_used, int(rng.choice([4, 16])), int(rng.integers(1, 301)), g * int(rng.integers(1, 5120 // g + 1)),
               int(rng.choice([1, n_used])))


def test_seeded_sweep(qg):
    """24 seeded cases over type, T <= 8, n_used <= 8, N <= 300, K <= 5120, each through Step.check."""
    for i, t, T, n_used, n_expert, n, k, a_rows in sweep_cases():
        woff = None if i % 2 else {Q4_K: 48, Q6_K: 18}.get(t, 12)
        Step(t, T, n_used, n_expert, n, k, a_rows, seed=3000 + i, woff=woff, fill=0xFF).check(qg)
