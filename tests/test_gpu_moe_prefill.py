"""qg_gemm_w4a8_moe_prefill on the GPU: the slots counting-sorted by expert id on the device, then every expert's rows
through the Q4_K / Q6_K MFMA prefill body in tiles of 16 TT rows.

Reference of every case: per expert, the slots' activation rows gathered on the host and the library's eager product
forced to the MFMA family -- in chunks of at most 32 rows (always RG = 1 / KS = 8) where qg_moe_prefill_config names
RG = 1, and at a row count whose qg_debug_config names RG = 4 where it names RG = 4 -- compared as uint32: an
output's arithmetic depends on its activation row, its weight row and KS alone. Every case is also held against the
NumPy contract with the MFMA bound of the type's own tests (KR.tol(mag, K, 16) for Q4_K, QR.tol(mag, K, 8) for Q6_K),
launched twice (identical bits), and written through out= into the interior of a sentinel-filled buffer with
ldc > N. The expert tensor and the workspace sit inside 0xFF bytes, and the workspace itself is 0xFF before the call.

The ids live in a [T, n_used + 3] tensor whose spare columns hold other valid ids and the activations are followed by
n_used spare rows, so a kernel that took n_used for the ids stride, or u for u % a_rows, reads other but allocated
memory and gives other bits.
"""
import ctypes
import functools

import numpy as np
import pytest

import moe_ref as MR
from moe_ref import Q4_K, Q6_K
from test_gpu_moe import F_SENT, bits, dev, host, views

pytestmark = pytest.mark.gpu

TYPES = (Q4_K, Q6_K)
FORMS = ((1, 1), (2, 1), (4, 1), (4, 4))
ALGO_MFMA = 2
W_MMQ = {Q4_K: 16, Q6_K: 8}  # the MFMA families' extra partial sums (kquant_ref.tol)
WOFF = {Q4_K: 16, Q6_K: 2}   # the smallest offset past a 256-B boundary the type's kernels take


def ref_mod(t):
    return MR.KR if t == Q4_K else MR.QR


def form_of(cfg):
    f = MR.cfg_fields(cfg)[1]
    return int(f["TT"]), int(f["RG"])


@functools.lru_cache(maxsize=None)
def operands(t, n_expert, n, k, rows, seed=0):
    """Experts [n_expert, n, ..] and `rows` activation rows of one shape, made once and never modified."""
    rng = np.random.default_rng([t, n_expert, n, k, rows, seed])
    return MR.random_experts(rng, t, n_expert, n, k), MR.random_act(rng, rows, k)


def ids_with_counts(rng, counts, n_used=1):
    """[T, n_used] ids in which expert e appears counts[e] times, shuffled (sum(counts) a multiple of n_used)."""
    flat = np.repeat(np.arange(len(counts), dtype=np.int32), counts)
    rng.shuffle(flat)
    return flat.reshape(-1, n_used)


def guarded_workspace(nbytes, fill=0xFF):
    """(16-B aligned window of nbytes, the whole flat buffer, the window's start) inside `fill` bytes."""
    import torch
    flat = torch.full((nbytes + 512,), fill, dtype=torch.uint8, device="cuda")
    start = (-flat.data_ptr()) % 256 + 16
    return flat[start:start + nbytes], flat, start


class Case:
    """One call on the device. a_all holds T * a_rows rows followed by n_used spare ones."""

    def __init__(self, t, ids_h, n_expert, n, k, a_rows, seed=0, w=None, w_h=None):
        ids_h = np.ascontiguousarray(ids_h, np.int32)
        self.t, self.n_expert, self.n, self.k, self.a_rows = t, n_expert, n, k, a_rows
        self.T, self.n_used = ids_h.shape
        self.ids_h = ids_h
        T, n_used = self.T, self.n_used
        if w is None:
            self.w_h, a_all = operands(t, n_expert, n, k, T * a_rows + n_used, seed)
            self.w = MR.KR.dev_at(self.w_h, WOFF[t], 0xFF)
        else:
            self.w_h, self.w = w_h, w
            a_all = MR.random_act(np.random.default_rng([seed, k]), T * a_rows + n_used, k)
        self.a_all_h = a_all
        self.a_all = dev(a_all)
        self.a = self.a_all[:T * a_rows].reshape(T, a_rows, k // 32, 36)
        full = np.random.default_rng([seed, T, n_used]).integers(0, n_expert, (T, n_used + 3)).astype(np.int32)
        full[:, :n_used] = ids_h
        self.ids_full = dev(full)
        self.ids = self.ids_full[:, :n_used]

    # -- the call
    def config(self, qg):
        return qg.moe_prefill_config(self.T, self.n_used, self.n_expert, self.n, self.k, self.t)

    def launch_guarded(self, qg, pad):
        """(window [T, n_used, N], whole buffer): out= the interior of a sentinel-filled [slots + 2, N + pad] buffer; the
        workspace a 0xFF-filled window of exactly the size function's bytes inside 0xFF bytes, which must survive."""
        import torch
        S = self.T * self.n_used
        buf = torch.full((S + 2, self.n + pad), F_SENT, dtype=torch.float32, device="cuda")
        out = buf[1:S + 1, :self.n].unflatten(0, (self.T, self.n_used))
        need = qg.moe_prefill_workspace_size(self.T, self.n_used, self.n_expert)
        ws, flat, start = guarded_workspace(need)
        got = qg.gemm_w4a8_moe_prefill(self.a, self.w, self.ids, self.T, self.n_used, self.n, self.k, self.t,
                                       a_rows=self.a_rows, workspace=ws, out=out)
        assert got.data_ptr() == out.data_ptr()
        whole, flat_h = host(buf), host(flat)
        assert (flat_h[:start] == 0xFF).all() and (flat_h[start + need:] == 0xFF).all(), "wrote outside the workspace"
        return whole[1:S + 1, :self.n].reshape(self.T, self.n_used, self.n).copy(), whole

    # -- the references
    def slots_of(self, e, ids=None):
        ids = self.ids_h if ids is None else ids
        return [(tt, u) for tt in range(self.T) for u in range(self.n_used) if ids[tt, u] == e]

    def row_of(self, tt, u):
        return tt * self.a_rows + u % self.a_rows

    def eager(self, qg, rows, e, rg):
        """The eager MFMA product of activation rows `rows` with expert e, at the given RG."""
        out = np.empty((len(rows), self.n), np.float32)
        if rg == 1:
            for i in range(0, len(rows), 32):
                a = self.a_all_h[rows[i:i + 32]]
                assert "RG=1 KS=8" in qg.debug_config(len(a), self.n, self.k, self.t, ALGO_MFMA)
                out[i:i + 32] = host(qg.gemm_w4a8(dev(a), self.w[e], len(a), self.n, self.k, self.t, algo=ALGO_MFMA))
            return out
        import torch
        m4 = 65  # the eager rule is ceil(N / 64) ceil(M / 64) >= CUs: at N <= 64 that takes 64 (CUs - 1) + 1 rows
        while "RG=4" not in qg.debug_config(m4, self.n, self.k, self.t, ALGO_MFMA):
            m4 += 64
            assert m4 <= 65 + 64 * 1024, "no RG = 4 eager shape at this N on this device"
        for i in range(0, len(rows), m4):
            r = list(rows[i:i + m4])
            idx = torch.tensor(r + [r[-1]] * (m4 - len(r)), device="cuda")  # (padded with the last row, on the device)
            out[i:i + m4] = host(qg.gemm_w4a8(self.a_all[idx], self.w[e], m4, self.n, self.k, self.t, algo=ALGO_MFMA)[:len(r)])
        return out

    def reference(self, qg, ids=None, rg=None):
        """float32 [T, n_used, N]: the eager family's bits; zeros where the id names no expert."""
        ids = self.ids_h if ids is None else ids
        rg = form_of(self.config(qg))[1] if rg is None else rg
        ref = np.zeros((self.T, self.n_used, self.n), np.float32)
        for e in np.unique(ids):
            if 0 <= e < self.n_expert:
                sl = self.slots_of(e, ids)
                got = self.eager(qg, [self.row_of(tt, u) for tt, u in sl], int(e), rg)
                for (tt, u), row in zip(sl, got):
                    ref[tt, u] = row
        return ref

    def assert_close_to_contract(self, c):
        R = ref_mod(self.t)
        for e in np.unique(self.ids_h):
            if 0 <= e < self.n_expert:
                sl = self.slots_of(e)
                a = self.a_all_h[[self.row_of(tt, u) for tt, u in sl]]
                c64, _, mag = R.gemm(a, self.w_h[e])
                tol = R.tol(mag, self.k, W_MMQ[self.t])
                got = np.stack([c[tt, u] for tt, u in sl]).astype(np.float64)
                err = np.abs(got - c64)
                assert (err <= tol).all(), (int(e), float((err / tol).max()))

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
        assert not diff, f"{len(diff)} slots, first {diff[:6]}, differ from the eager MFMA product ({self.config(qg)})"
        if contract:
            self.assert_close_to_contract(c)
        _, again = self.launch_guarded(qg, pad)
        assert np.array_equal(bits(whole), bits(again))
        return c


def rg4_n(qg, t, T, n_used, n_expert, k):
    """The smallest ragged N = 64 j + 1 at which the prefill config of these slots names RG = 4."""
    n = 65
    while form_of(qg.moe_prefill_config(T, n_used, n_expert, n, k, t)) != (4, 4):
        n += 64 * 8
        assert n <= 65 + 64 * 512, "the (4, 4) form is unreachable on this device"
    while n > 65 and form_of(qg.moe_prefill_config(T, n_used, n_expert, n - 64, k, t)) == (4, 4):
        n -= 64
    return n


# ---------------------------------------------------------------------------- 1. every form, the row counts around R
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("form", FORMS)
def test_every_form_with_row_counts_around_the_tile(qg, t, form):
    """Six experts with 0, 1, R - 1, R, R + 1 and 2 R + 1 slots in one call (R = 16 TT): 5 R + 2 slots over 6 experts
    is the form's own range of slots / n_expert. RG = 4 at K = 768: the second K slice idles in the last step; the
    RG = 1 forms at K = 1280 (five of the eight slices busy; Q6_K takes them only beyond K = 1024).
    The form is searched through qg_moe_prefill_config, the test fails where it is not reached."""
    tt, rg = form
    R, k = 16 * tt, 768 if rg == 4 else 1280
    counts = [0, 1, R - 1, R, R + 1, 2 * R + 1]
    T = sum(counts)
    n = rg4_n(qg, Q4_K, T, 1, 6, k) if rg == 4 else 17  # (the N of the rule both types share)
    cfg = qg.moe_prefill_config(T, 1, 6, n, k, t)
    assert form_of(cfg) == form and f"KS={8 // rg} R={R}" in cfg, cfg
    assert MR.cfg_fields(cfg)[1]["grid"] == f"{-(-n // (16 * rg))}x{T // R + 7}", cfg
    ids = ids_with_counts(np.random.default_rng(R), counts)
    Case(t, ids, 6, n, k, a_rows=1, seed=tt + rg).check(qg)


# ---------------------------------------------------------------------------- 2. K and N edges
@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("k,n", [(256, 1), (256, 65), (768, 15), (2304, 17), (2304, 1)])
def test_k_and_n_edges(qg, t, k, n):
    """K = 256: one super-block, seven idle slices; K = 2304: a second pass of the eight slices; N = 1, 15, 17, 65
    around the 16-row group. Two used experts per token, a row per slot, in the (1, 1) and the (4, 1) form; Q6_K at
    K <= 1024 takes (4, 4) for any slots (K = 256: one slice of the two idle throughout)."""
    rng = np.random.default_rng([k, n])
    for T, n_expert, want in ((9, 3, (1, 1)), (50, 2, (4, 1))):
        ids = rng.integers(0, n_expert, (T, 2)).astype(np.int32)
        c = Case(t, ids, n_expert, n, k, a_rows=2, seed=k + n)
        assert form_of(c.config(qg)) == ((4, 4) if t == Q6_K and k <= 1024 else want)
        c.check(qg)


# ---------------------------------------------------------------------------- 3. ids
@pytest.mark.parametrize("t", TYPES)
def test_all_slots_on_one_expert(qg, t):
    ids = np.full((35, 2), 2, np.int32)
    c = Case(t, ids, 4, 33, 1280, a_rows=1)
    assert form_of(c.config(qg)) == (2, 1)  # 70 slots: three tiles of 32 rows, the last of 6
    c.check(qg)


@pytest.mark.parametrize("t", TYPES)
def test_130_experts_most_of_them_empty(qg, t):
    rng = np.random.default_rng(130)
    ids = rng.choice([0, 3, 64, 128, 129], (20, 2)).astype(np.int32)
    c = Case(t, ids, 130, 19, 512, a_rows=2)
    c.check(qg)
    counts, _ = qg.debug_moe_prefill_plan(c.ids, 130, 19, 512, t, a_rows=2)
    assert (host(counts) == 0).sum() == 131 - 5


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("a_rows", [1, 3])
def test_repeated_and_invalid_ids(qg, t, a_rows):
    """Ids repeated within a token (a_rows 1: the slots share the token's row; a_rows n_used: a row each), ids of -1
    and n_expert in the middle: bit pattern 0 in exactly those rows, their neighbours unaffected."""
    rng = np.random.default_rng(7 + a_rows)
    T, n_expert = 30, 4
    ids = rng.integers(0, n_expert, (T, 3)).astype(np.int32)
    ids[:, 1] = ids[:, 0]
    ids[T // 2, 1], ids[T // 2 + 1, 0], ids[T // 3, 2] = -1, n_expert, 2 ** 31 - 1
    c = Case(t, ids, n_expert, 21, 1280, a_rows=a_rows)
    assert form_of(c.config(qg)) == (2, 1)
    out = c.check(qg)
    zero = [(tt, u) for tt in range(T) for u in range(3) if (bits(out[tt, u]) == 0).all()]
    assert zero == [(T // 3, 2), (T // 2, 1), (T // 2 + 1, 0)]


@pytest.mark.parametrize("n,k", [(5, 768), (3, 256), (7, 2304)])
def test_q6k_experts_of_alternating_parity(qg, n, k):
    """Q6_K experts 2 B off a dword with an odd number of super-blocks per expert: consecutive experts alternate
    between the two parities the kernel realigns."""
    assert (n * k // 256) % 2 == 1 and MR.expert_bytes(Q6_K, n, k) % 4 == 2
    ids = np.random.default_rng(n).integers(0, 4, (40, 2)).astype(np.int32)
    c = Case(Q6_K, ids, 4, n, k, a_rows=2)
    assert c.w.data_ptr() % 4 == 2
    c.check(qg)


# ---------------------------------------------------------------------------- 4. position independence
@pytest.mark.parametrize("t", TYPES)
def test_token_order_does_not_reach_the_bits(qg, t):
    """The same slots with the tokens permuted (so every slot lands at another tile position): the same bits per slot."""
    rng = np.random.default_rng(11)
    T, n_used, n_expert, n, k = 45, 2, 3, 23, 1024
    ids = rng.integers(0, n_expert, (T, n_used)).astype(np.int32)
    base = Case(t, ids, n_expert, n, k, a_rows=2)
    c0 = base.check(qg, contract=False)
    perm = rng.permutation(T)
    p = Case(t, ids[perm], n_expert, n, k, a_rows=2)
    rows = (perm[:, None] * 2 + np.arange(2)[None]).reshape(-1)
    p.a_all_h = np.concatenate([base.a_all_h[rows], base.a_all_h[T * 2:]])
    p.a_all = dev(p.a_all_h)
    p.a = p.a_all[:T * 2].reshape(T, 2, k // 32, 36)
    c1, _ = p.launch_guarded(qg, 3)
    assert np.array_equal(bits(c1), bits(c0[perm]))


# ---------------------------------------------------------------------------- 5. the plan
@pytest.mark.parametrize("n_expert,T,n_used", [(1, 5, 1), (8, 64, 2), (130, 33, 3), (1024, 300, 4)])
def test_plan_counts_and_sorted_list(qg, n_expert, T, n_used):
    rng = np.random.default_rng([n_expert, T])
    ids = rng.integers(-2, n_expert + 2, (T, n_used + 2)).astype(np.int32)
    ids_d = dev(ids)[:, :n_used]
    ids = ids[:, :n_used]
    ws, flat, start = guarded_workspace(qg.moe_prefill_workspace_size(T, n_used, n_expert))
    counts, order = qg.debug_moe_prefill_plan(ids_d, n_expert, 32, 512, Q4_K, workspace=ws)
    counts, order = host(counts), host(order)
    flat_ids = ids.reshape(-1)
    valid = (flat_ids >= 0) & (flat_ids < n_expert)
    want = np.bincount(np.where(valid, flat_ids, n_expert), minlength=n_expert + 1)
    assert np.array_equal(counts, want)
    assert np.array_equal(np.sort(order), np.arange(T * n_used))  # a permutation of all the slots
    nv = int(valid.sum())
    head = order[:nv]
    assert valid[head].all() and not valid[order[nv:]].any()
    assert (np.diff(flat_ids[head]) >= 0).all()  # grouped by expert, in expert order
    f = host(flat)
    assert (f[:start] == 0xFF).all() and (f[start + ws.numel():] == 0xFF).all()


# ---------------------------------------------------------------------------- 6. an expert beyond 4 GiB
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
    c = Case(t, ids, n_expert, n, k, a_rows=1, w=w, w_h=w_h)
    c.check(qg)
    del w, c


# ---------------------------------------------------------------------------- 7. capture
@pytest.mark.parametrize("t", TYPES)
def test_captured_call_follows_the_ids_of_every_replay(qg, t):
    """One captured call; the ids are overwritten between replays with distributions that change every expert's count
    and the number of tiles, one of them with every id invalid."""
    import torch
    T, n_used, n_expert, n, k = 40, 2, 4, 19, 1280
    rng = np.random.default_rng(5)
    dists = [ids_with_counts(rng, c, n_used) for c in ([20, 20, 20, 20], [1, 3, 40, 36], [70, 0, 9, 1])]
    dists.append(np.full((T, n_used), -1, np.int32))
    dists.append(ids_with_counts(rng, [17, 33, 0, 30], n_used))
    c = Case(t, dists[0], n_expert, n, k, a_rows=2)
    assert form_of(c.config(qg)) == (2, 1)
    tiles = [sum(-(-int(x) // 32) for x in np.bincount(np.where(d < 0, n_expert, d).reshape(-1), minlength=n_expert + 1)) for d in dists]
    assert len(set(tiles)) >= 3, tiles
    refs = [c.reference(qg, d) for d in dists]
    out = torch.zeros((T, n_used, n), dtype=torch.float32, device="cuda")
    ws = torch.full((qg.moe_prefill_workspace_size(T, n_used, n_expert),), 0xFF, dtype=torch.uint8, device="cuda")
    call = lambda: qg.gemm_w4a8_moe_prefill(c.a, c.w, c.ids, T, n_used, n, k, t, a_rows=2, workspace=ws, out=out)
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


# ---------------------------------------------------------------------------- 8. the view entry and the refusals
@pytest.mark.parametrize("t", TYPES)
def test_view_entry_on_a_strided_ids_view(qg, t):
    import torch
    import quant_gemm.ggml as G
    ids = np.random.default_rng(3).integers(0, 16, (24, 2)).astype(np.int32)
    s = Case(t, ids, 16, 21, 512, a_rows=2)
    assert s.ids.stride(0) == 5 and not s.ids.is_contiguous()
    ref = s.reference(qg)
    buf = torch.full((s.T, s.n_used, s.n + 3), F_SENT, dtype=torch.float32, device="cuda")
    out = buf[:, :, :s.n]
    ws = torch.full((qg.moe_prefill_workspace_size(s.T, s.n_used, 16),), 0xFF, dtype=torch.uint8, device="cuda")
    w, a, i, o = views(G, s, out)
    G.mul_mat_id_from_ggml_ws(w, a, i, o, ws)
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
            G.mul_mat_id_from_ggml_ws(w, a, i, o, ws)
    with pytest.raises(RuntimeError, match="invalid argument"):
        G.mul_mat_id_from_ggml_ws(*views(G, s, out), ws[:-1])
    assert (host(buf) == F_SENT).all() and (host(ws) == 0xFF).all()


@pytest.mark.parametrize("t", TYPES)
def test_refusals_on_real_buffers(qg, t):
    """Refused by the C entry with the output and the workspace untouched: a K off the granule, a row type, weights
    and a workspace off their alignment, a workspace one byte short, an ldc below N; then the call itself."""
    import torch
    import quant_gemm._lib as L
    P = ctypes.c_void_p
    ids = np.random.default_rng(9).integers(0, 4, (12, 2)).astype(np.int32)
    s = Case(t, ids, 4, 9, 512, a_rows=1)
    out = torch.full((s.T, s.n_used, s.n), F_SENT, dtype=torch.float32, device="cuda")
    need = qg.moe_prefill_workspace_size(s.T, s.n_used, 4)
    ws = torch.full((need + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    st = P(torch.cuda.current_stream().cuda_stream)
    call = lambda k=512, woff=0, ldc=0, wt=t, wsoff=0, wsb=need: L.load().qg_gemm_w4a8_moe_prefill(
        P(s.a.data_ptr()), 1, P(s.w.data_ptr() + woff), 4, P(s.ids_full.data_ptr()), s.ids_full.stride(0),
        P(out.data_ptr()), ldc, s.T, s.n_used, s.n, k, wt, P(ws.data_ptr() + wsoff), wsb, st)
    assert call(512 - 32) == -2
    assert call(wt=MR.Q4_0) == -3 and call(wt=MR.Q8_0) == -3
    assert call(woff=1 if t == Q6_K else 8) == -4
    assert call(ldc=s.n - 1) == -1
    assert call(wsoff=4) == -4 and call(wsoff=8) == -4
    assert call(wsb=need - 1) == -1
    assert (host(out) == F_SENT).all() and (host(ws) == 0xFF).all()
    assert call() == 0
    assert np.array_equal(bits(host(out)), bits(s.reference(qg)))
    assert (host(ws)[need:] == 0xFF).all()


# ---------------------------------------------------------------------------- 9. seeded sweep
def sweep_cases(count=24, seed=2107):
    rng = np.random.default_rng(seed)
    for i in range(count):
        t = TYPES[i % 2]
        n_expert = int(rng.choice([1, 3, 8, 130]))
        n_used = int(rng.integers(1, 5))
        T = int(rng.integers(1, 41))
        yield (i, t, T, n_used, n_expert, int(rng.integers(1, 151)), 256 * int(rng.integers(1, 10)), int(rng.choice([1, n_used])))


def test_seeded_sweep(qg):
    """24 seeded cases over type, T <= 40, n_used <= 4, 1 .. 130 experts, N <= 150, K <= 2304, ids from -1 to n_expert,
    each through Case.check."""
    seen = set()
    for i, t, T, n_used, n_expert, n, k, a_rows in sweep_cases():
        ids = np.random.default_rng(i).integers(-1 if i % 3 == 0 else 0, n_expert + (i % 3 == 0), (T, n_used)).astype(np.int32)
        c = Case(t, ids, n_expert, n, k, a_rows, seed=5000 + i)
        seen.add(form_of(c.config(qg)))
        c.check(qg)
    assert len(seen) >= 3, seen
