"""qg_gemm_w4a8_moe_batch on the GPU: the slots counting-sorted by expert id on the device, then every expert's rows
through the Q4_K / Q6_K decode GEMV body in tiles of R = 2, 4 or 8 gathered rows.

Every case launches into guarded buffers (out= the interior of a sentinel-filled buffer with ldc > N; the workspace a
window of exactly the size function's bytes, 0xFF before the call, inside 0xFF bytes that must survive; the expert
tensor inside 0xFF bytes) and every output is compared two ways: bit for bit with qg_gemm_w4a8_moe on the same
operands, and against moe_ref.assert_close_to_model, the NumPy contract with the decode GEMV's bound (W = 0). Every
case is launched twice (identical bits).

The operands are those of tests/test_gpu_moe_prefill.py's Case: the ids live in a [T, n_used + 3] tensor whose spare
columns hold other valid ids and the activations are followed by n_used spare rows, so a kernel that took n_used for
the ids stride, or u for u % a_rows, reads other but allocated memory and gives other bits.
"""
import ctypes

import numpy as np
import pytest

import moe_ref as MR
from moe_ref import Q4_K, Q6_K
from test_gpu_moe import F_SENT, bits, dev, host, views
from test_gpu_moe_prefill import Case, guarded_workspace, ids_with_counts

pytestmark = pytest.mark.gpu

TYPES = (Q4_K, Q6_K)
ROWS = (2, 4, 8)
FORM_K = (256, 512, 1024, 1280, 4096, 4352)  # LPR 4 / 16 / 64, each loop-free (ONE) and with the unit loop


def fields(cfg):
    return MR.cfg_fields(cfg)[1]


def rows_of(cfg):
    return int(fields(cfg)["R"])


def rows_per_workgroup(cfg):
    f = fields(cfg)
    return int(f["WGS"]) // 64 * (64 // int(f["LPR"]))


class BatchCase(Case):
    def config(self, qg):
        return qg.moe_batch_config(self.T, self.n_used, self.n_expert, self.n, self.k, self.t)

    def launch_guarded(self, qg, pad):
        """(window [T, n_used, N], whole buffer): out= the interior of a sentinel-filled [slots + 2, N + pad] buffer; the
        workspace a 0xFF-filled window of exactly the size function's bytes inside 0xFF bytes, which must survive."""
        import torch
        S = self.T * self.n_used
        buf = torch.full((S + 2, self.n + pad), F_SENT, dtype=torch.float32, device="cuda")
        out = buf[1:S + 1, :self.n].unflatten(0, (self.T, self.n_used))
        need = qg.moe_batch_workspace_size(self.T, self.n_used, self.n_expert)
        ws, flat, start = guarded_workspace(need)
        got = qg.gemm_w4a8_moe_batch(self.a, self.w, self.ids, self.T, self.n_used, self.n, self.k, self.t,
                                     a_rows=self.a_rows, workspace=ws, out=out)
        assert got.data_ptr() == out.data_ptr()
        whole, flat_h = host(buf), host(flat)
        assert (flat_h[:start] == 0xFF).all() and (flat_h[start + need:] == 0xFF).all(), "wrote outside the workspace"
        return whole[1:S + 1, :self.n].reshape(self.T, self.n_used, self.n).copy(), whole

    def reference(self, qg, ids=None):
        """float32 [T, n_used, N]: qg_gemm_w4a8_moe on the same operands (zeros where the id names no expert)."""
        ids_d = self.ids
        if ids is not None:
            full = host(self.ids_full).copy()
            full[:, :self.n_used] = ids
            ids_d = dev(full)[:, :self.n_used]
        return host(qg.gemm_w4a8_moe(self.a, self.w, ids_d, self.T, self.n_used, self.n, self.k, self.t, a_rows=self.a_rows))

    def assert_close_to_contract(self, c):
        for tt in range(self.T):
            for u in range(self.n_used):
                e = int(self.ids_h[tt, u])
                if 0 <= e < self.n_expert:
                    MR.assert_close_to_model(None, c[tt, u], self.a_all_h[self.row_of(tt, u)], self.w_h[e], self.t)

    def check(self, qg, pad=None, contract=True):
        pad = 1 + (3 * self.n + self.T + self.k // 32) % 29 if pad is None else pad
        c, whole = self.launch_guarded(qg, pad)
        outside = np.ones(whole.shape, bool)
        outside[1:-1, :self.n] = False
        assert (whole[outside] == np.float32(F_SENT)).all(), f"wrote outside the slots' rows (ldc = {self.n + pad})"
        bad = [(tt, u) for tt in range(self.T) for u in range(self.n_used) if not 0 <= self.ids_h[tt, u] < self.n_expert]
        for tt, u in bad:
            assert (bits(c[tt, u]) == 0).all(), (tt, u)  # +0.0f, not -0.0f, not the sentinel
        ref = self.reference(qg)
        diff = [(tt, u) for tt in range(self.T) for u in range(self.n_used) if not np.array_equal(bits(c[tt, u]), bits(ref[tt, u]))]
        assert not diff, f"{len(diff)} slots, first {diff[:6]}, differ from qg_gemm_w4a8_moe ({self.config(qg)})"
        if contract:
            self.assert_close_to_contract(c)
        _, again = self.launch_guarded(qg, pad)
        assert np.array_equal(bits(whole), bits(again))
        return c


def experts_for_rows(qg, t, slots, n_used, r, n, k, at_least):
    """The smallest n_expert >= at_least (the further experts stay empty) at which the config of these slots names R = r."""
    for n_expert in range(at_least, at_least + 64):
        if rows_of(qg.moe_batch_config(slots // n_used, n_used, n_expert, n, k, t)) == r:
            return n_expert
    raise AssertionError(f"no n_expert in [{at_least}, {at_least + 64}) gives R = {r} for {slots} slots at K = {k}")


# ---------------------------------------------------------------------------- 1. every R, the row counts around R
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("k", FORM_K)
def test_every_r_with_row_counts_around_the_tile(qg, t, r, k):
    """Experts with 0, 1, R - 1, R, R + 1 and 2 R + 1 slots in one call, at every (LPR, ONE) form of the body and with N
    one below and one above a workgroup's rows, and N = 1. The n_expert (6 to 8: the further ones empty) at which the
    config names R is searched through qg_moe_batch_config; the test fails where none does."""
    counts = [0, 1, r - 1, r, r + 1, 2 * r + 1]
    T = sum(counts)
    n_expert = experts_for_rows(qg, t, T, 1, r, 17, k, 6)
    assert n_expert <= 8
    counts += [0] * (n_expert - 6)
    cfg = qg.moe_batch_config(T, 1, n_expert, 17, k, t)
    f, single = fields(cfg), fields(qg.moe_config(T, 1, 17, k, t))
    assert cfg.startswith("moeb:" + ("q4k_gemv" if t == Q4_K else "q6k_gemv")) and rows_of(cfg) == r
    assert (f["LPR"], f["WGS"], f["ONE"]) == (single["LPR"], single["WGS"], single["ONE"])
    assert (int(f["LPR"]), int(f["ONE"])) == {256: (4, 1), 512: (4, 0), 1024: (16, 1), 1280: (16, 0), 4096: (64, 1), 4352: (64, 0)}[k]
    rpb = rows_per_workgroup(cfg)
    assert rpb == {4: 64, 16: 32, 64: 16}[int(f["LPR"])]
    ids = ids_with_counts(np.random.default_rng(r), counts)
    for n in (rpb - 1, rpb + 1, 1):
        g = fields(qg.moe_batch_config(T, 1, n_expert, n, k, t))["grid"]
        assert g == f"{-(-n // rpb)}x{T // r + n_expert + 1}", g
        BatchCase(t, ids, n_expert, n, k, a_rows=1, seed=r).check(qg)


# ---------------------------------------------------------------------------- 2. ids and activations
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("a_rows", [1, 3])
def test_repeated_and_invalid_ids(qg, t, a_rows):
    """Ids repeated within a token (a_rows 1: the slots share the token's row; a_rows n_used: a row each), ids of -1,
    n_expert and n_expert + 5 in the middle: bit pattern 0 in exactly those rows, their neighbours unaffected. The ids
    row stride is n_used + 3."""
    rng = np.random.default_rng(7 + a_rows)
    T, n_expert = 14, 4
    ids = rng.integers(0, n_expert, (T, 3)).astype(np.int32)
    ids[:, 1] = ids[:, 0]
    ids[T // 2, 1], ids[T // 2 + 1, 0], ids[T // 3, 2] = -1, n_expert, n_expert + 5
    c = BatchCase(t, ids, n_expert, 21, 1280, a_rows=a_rows)
    assert c.ids.stride(0) == 6 and rows_of(c.config(qg)) == 8
    out = c.check(qg)
    zero = [(tt, u) for tt in range(T) for u in range(3) if (bits(out[tt, u]) == 0).all()]
    assert zero == [(T // 3, 2), (T // 2, 1), (T // 2 + 1, 0)]


@pytest.mark.parametrize("t", TYPES)
def test_every_id_invalid(qg, t):
    ids = np.array([[-1, 5], [7, -3], [2 ** 31 - 1, 5], [-2 ** 31, 6], [5, 5]], np.int32)
    out = BatchCase(t, ids, 5, 33, 512, a_rows=2).check(qg)
    assert (bits(out) == 0).all()


# ---------------------------------------------------------------------------- 3. extreme routing
@pytest.mark.parametrize("t", TYPES)
def test_all_slots_on_one_expert(qg, t):
    ids = np.full((13, 2), 2, np.int32)
    c = BatchCase(t, ids, 4, 33, 1280, a_rows=1)
    assert rows_of(c.config(qg)) == 8  # 26 slots: three tiles of 8 rows, the last of 2
    c.check(qg)


@pytest.mark.parametrize("t", TYPES)
def test_130_experts_most_of_them_empty(qg, t):
    rng = np.random.default_rng(130)
    ids = rng.choice([0, 3, 64, 128, 129], (20, 2)).astype(np.int32)
    c = BatchCase(t, ids, 130, 19, 512, a_rows=2)
    assert rows_of(c.config(qg)) == 2  # 40 slots over 130 experts, eight a piece on the five chosen ones
    c.check(qg)


# ---------------------------------------------------------------------------- 4. position independence
@pytest.mark.parametrize("t", TYPES)
def test_token_order_does_not_reach_the_bits(qg, t):
    """The same slots with the tokens permuted (so every slot lands at another tile position): the same bits per slot."""
    rng = np.random.default_rng(11)
    T, n_used, n_expert, n, k = 19, 2, 3, 23, 1024
    ids = rng.integers(0, n_expert, (T, n_used)).astype(np.int32)
    base = BatchCase(t, ids, n_expert, n, k, a_rows=2)
    c0 = base.check(qg, contract=False)
    perm = rng.permutation(T)
    p = BatchCase(t, ids[perm], n_expert, n, k, a_rows=2)
    rows = (perm[:, None] * 2 + np.arange(2)[None]).reshape(-1)
    p.a_all_h = np.concatenate([base.a_all_h[rows], base.a_all_h[T * 2:]])
    p.a_all = dev(p.a_all_h)
    p.a = p.a_all[:T * 2].reshape(T, 2, k // 32, 36)
    c1, _ = p.launch_guarded(qg, 3)
    assert np.array_equal(bits(c1), bits(c0[perm]))


# ---------------------------------------------------------------------------- 5. Q6_K parity
@pytest.mark.parametrize("n,k", [(5, 768), (3, 256), (7, 2304), (1, 4352)])
def test_q6k_experts_of_alternating_parity(qg, n, k):
    """Q6_K experts 2 B off a dword with an odd number of super-blocks per expert: consecutive experts alternate
    between the two parities the kernel realigns."""
    assert (n * k // 256) % 2 == 1 and MR.expert_bytes(Q6_K, n, k) % 4 == 2
    ids = np.random.default_rng(n).integers(0, 4, (11, 2)).astype(np.int32)
    c = BatchCase(Q6_K, ids, 4, n, k, a_rows=2)
    assert c.w.data_ptr() % 4 == 2
    c.check(qg)


# ---------------------------------------------------------------------------- 6. the LDS cap
@pytest.mark.parametrize("t,k", [(Q4_K, 15616), (Q6_K, 17408)])
def test_rows_per_tile_at_the_lds_cap(qg, t, k):
    """Six slots per expert ask for R = 8; eight rows' records exceed 160 KiB at this K, so the config names R = 4 (and
    R = 8 one super-block below), with more than 64 KiB of dynamic LDS."""
    ids = ids_with_counts(np.random.default_rng(k), [7, 5])
    c = BatchCase(t, ids, 2, 5, k, a_rows=1)
    f = fields(c.config(qg))
    assert int(f["R"]) == 4 and int(f["lds"]) == 4 * (k // 256) * MR.KQ_REC_BYTES[t] > 64 * 1024
    assert rows_of(qg.moe_batch_config(12, 1, 2, 5, k - 256, t)) == 8
    c.check(qg)


# ---------------------------------------------------------------------------- 7. an expert beyond 4 GiB
def test_expert_beyond_4_gib(qg):
    """Q4_K, N = K = 4096, 460 experts of 9 MiB: expert 457 starts 4.3e9 bytes past the base. The tensor is
    torch.empty; only the two selected experts are written."""
    import torch
    t, n, k, n_expert = Q4_K, 4096, 4096, 460
    per = MR.expert_bytes(t, n, k)
    sel = (457, 1)
    assert sel[0] * per > 2 ** 32
    rng = np.random.default_rng(4096)
    w = torch.empty((n_expert, n, k // 256, 144), dtype=torch.uint8, device="cuda")
    w_h = {e: MR.random_experts(rng, t, 1, n, k)[0] for e in sel}
    for e in sel:
        w[e].copy_(dev(w_h[e]))
    ids = np.array([[457, 1], [1, 457], [457, -1]], np.int32)
    c = BatchCase(t, ids, n_expert, n, k, a_rows=1, w=w, w_h=w_h)
    c.check(qg)
    del w, c


# ---------------------------------------------------------------------------- 8. capture
@pytest.mark.parametrize("t", TYPES)
def test_captured_call_follows_the_ids_of_every_replay(qg, t):
    """One captured call; the ids are overwritten between replays with distributions that change every expert's count
    and the number of tiles, one of them with every id invalid."""
    import torch
    T, n_used, n_expert, n, k = 12, 2, 4, 19, 1280
    rng = np.random.default_rng(5)
    dists = [ids_with_counts(rng, c, n_used) for c in ([6, 6, 6, 6], [1, 3, 11, 9], [20, 0, 3, 1])]
    dists.append(np.full((T, n_used), -1, np.int32))
    dists.append(ids_with_counts(rng, [5, 9, 0, 10], n_used))
    c = BatchCase(t, dists[0], n_expert, n, k, a_rows=2)
    r = rows_of(c.config(qg))
    tiles = [sum(-(-int(x) // r) for x in np.bincount(np.where(d < 0, n_expert, d).reshape(-1), minlength=n_expert + 1)) for d in dists]
    assert len(set(tiles)) >= 3, tiles
    refs = [c.reference(qg, d) for d in dists]
    out = torch.zeros((T, n_used, n), dtype=torch.float32, device="cuda")
    ws = torch.full((qg.moe_batch_workspace_size(T, n_used, n_expert),), 0xFF, dtype=torch.uint8, device="cuda")
    call = lambda: qg.gemm_w4a8_moe_batch(c.a, c.w, c.ids, T, n_used, n, k, t, a_rows=2, workspace=ws, out=out)
    call()  # (warm: module load outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for d, ref in zip(dists, refs):
        c.ids_full[:, :n_used].copy_(dev(d))  # in place: the graph holds the pointer
        out.fill_(F_SENT)
        g.replay()
        assert np.array_equal(bits(host(out)), bits(ref))
    assert (bits(refs[3]) == 0).all()


# ---------------------------------------------------------------------------- 9. refusals on real buffers
@pytest.mark.parametrize("t", TYPES)
def test_refusals_on_real_buffers(qg, t):
    """Refused by the C entry with the output and the workspace untouched: a K off the granule, a row type, weights
    and a workspace off their alignment, a workspace one byte short (the prefill's size is), an ldc below N, too many
    experts; then the call itself."""
    import torch
    import quant_gemm._lib as L
    P = ctypes.c_void_p
    ids = np.random.default_rng(9).integers(0, 4, (12, 2)).astype(np.int32)
    s = BatchCase(t, ids, 4, 9, 512, a_rows=1)
    out = torch.full((s.T, s.n_used, s.n), F_SENT, dtype=torch.float32, device="cuda")
    need = qg.moe_batch_workspace_size(s.T, s.n_used, 4)
    assert qg.moe_prefill_workspace_size(s.T, s.n_used, 4) < need
    ws = torch.full((need + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    st = P(torch.cuda.current_stream().cuda_stream)
    call = lambda k=512, woff=0, ldc=0, wt=t, wsoff=0, wsb=need, ne=4: L.load().qg_gemm_w4a8_moe_batch(
        P(s.a.data_ptr()), 1, P(s.w.data_ptr() + woff), ne, P(s.ids_full.data_ptr()), s.ids_full.stride(0),
        P(out.data_ptr()), ldc, s.T, s.n_used, s.n, k, wt, P(ws.data_ptr() + wsoff), wsb, st)
    assert call(512 - 32) == -2
    assert call(wt=MR.Q4_0) == -3 and call(wt=MR.Q8_0) == -3
    assert call(woff=1 if t == Q6_K else 8) == -4
    assert call(ldc=s.n - 1) == -1
    assert call(wsoff=4) == -4 and call(wsoff=8) == -4
    assert call(wsb=need - 1) == -1 and call(wsb=qg.moe_prefill_workspace_size(s.T, s.n_used, 4)) == -1
    assert call(ne=4097, wsb=1 << 30) == -3
    assert (host(out) == F_SENT).all() and (host(ws) == 0xFF).all()
    assert call() == 0
    assert np.array_equal(bits(host(out)), bits(s.reference(qg)))
    assert (host(ws)[need:] == 0xFF).all()


# ---------------------------------------------------------------------------- 10. the view entry
@pytest.mark.parametrize("t", TYPES)
def test_view_entry_on_a_strided_ids_view(qg, t):
    import torch
    import quant_gemm.ggml as G
    ids = np.random.default_rng(3).integers(0, 16, (24, 2)).astype(np.int32)
    s = BatchCase(t, ids, 16, 21, 512, a_rows=2)
    assert s.ids.stride(0) == 5 and not s.ids.is_contiguous()
    ref = s.reference(qg)
    buf = torch.full((s.T, s.n_used, s.n + 3), F_SENT, dtype=torch.float32, device="cuda")
    out = buf[:, :, :s.n]  # nb[1] = 4 (N + 3)
    ws = torch.full((qg.moe_batch_workspace_size(s.T, s.n_used, 16),), 0xFF, dtype=torch.uint8, device="cuda")
    w, a, i, o = views(G, s, out)
    assert o.nb[1] > 4 * s.n
    G.mul_mat_id_from_ggml_batch(w, a, i, o, ws)
    got = host(buf)
    assert np.array_equal(bits(got[:, :, :s.n]), bits(ref)) and (got[:, :, s.n:] == F_SENT).all()
    # the refusals of qg_mul_mat_id_from_view, the output and the workspace untouched
    buf.fill_(F_SENT)
    ws.fill_(0xFF)
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
            G.mul_mat_id_from_ggml_batch(w, a, i, o, ws)
    with pytest.raises(RuntimeError, match="invalid argument"):
        G.mul_mat_id_from_ggml_batch(*views(G, s, out), ws[:-1])
    assert (host(buf) == F_SENT).all() and (host(ws) == 0xFF).all()


# ---------------------------------------------------------------------------- 11. seeded sweep
def sweep_cases(count=24, seed=2240):  # (a seed at which both types meet every R three times or more)
    rng = np.random.default_rng(seed)
    for i in range(count):
        t = TYPES[i % 2]
        n_expert = int(rng.choice([1, 3, 8, 17, 40, 140]))
        n_used = int(rng.integers(1, 5))
        T = int(rng.integers(1, 71))
        yield (i, t, T, n_used, n_expert, int(rng.integers(1, 201)), 256 * int(rng.integers(1, 21)), int(rng.choice([1, n_used])))


def test_seeded_sweep(qg):
    """24 seeded cases over type, T <= 70, n_used <= 4, 1 .. 140 experts, N <= 200, K <= 5120, ids from -1 to n_expert,
    each through BatchCase.check."""
    seen = set()
    for i, t, T, n_used, n_expert, n, k, a_rows in sweep_cases():
        ids = np.random.default_rng(i).integers(-1 if i % 3 == 0 else 0, n_expert + (i % 3 == 0), (T, n_used)).astype(np.int32)
        c = BatchCase(t, ids, n_expert, n, k, a_rows, seed=6000 + i)
        seen.add(rows_of(c.config(qg)))
        c.check(qg)
    assert seen == set(ROWS), seen
