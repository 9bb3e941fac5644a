"""qg_gemm_w4a8_moe_prefill_bias on the GPU: the expert-grouped MFMA prefill with MXFP4 experts ("moe:mxfp4_mmq") and a
per-expert bias added to the finished product, Q4_K / Q6_K beside it.

The harness is tests/test_gpu_moe_prefill.py's (its Case, imported): ids in a [T, n_used + 3] tensor, spare activation
rows, the output in the interior of a sentinel-filled buffer with ldc > N, the workspace 0xFF-filled and guarded, every
case launched twice with identical bits. The reference of the product is that module's: per expert the gathered rows
through the eager qg_gemm_w4a8 forced to the MFMA family at the RG the config names, as uint32; then
np.float32(product) + np.float32(bias). Every case is also held against the type's NumPy model with the prefill's own
bound plus 2^-24 |product + bias| for the add (moe_id_bias_ref.biased_tol).

The bias sits in a [n_expert + 2, stride > N] buffer, the experts in rows 1 .. n_expert; rows 0 and n_expert + 1 and the
padding columns hold NaN: an id clamped into the buffer or a wrong stride shows as NaN in the output.
"""
import ctypes
import functools

import numpy as np
import pytest

import moe_id_bias_ref as BR
import moe_ref as MR
from moe_id_bias_ref import MXFP4, Q4_K, Q6_K
from test_gpu_moe import F_SENT, bits, dev, host
from test_gpu_moe_prefill import Case, form_of, guarded_workspace, ids_with_counts

pytestmark = pytest.mark.gpu

FORMS = ((1, 1), (2, 1), (4, 1), (4, 4))
WOFF = {Q4_K: 16, Q6_K: 2}  # (MXFP4: any byte, given per case)


@functools.lru_cache(maxsize=None)
def experts(t, n_expert, n, k, seed=0):
    """Experts [n_expert, n, ..] of one shape, made once and never modified."""
    return BR.random_experts(np.random.default_rng([t, n_expert, n, k, seed]), t, n_expert, n, k)


class BiasCase(Case):
    """One call of the biased entry. bias: True (a guarded buffer of stride N + 3), or None (the null bias)."""

    def __init__(self, t, ids_h, n_expert, n, k, a_rows, seed=0, woff=None, bias=True):
        w_h = experts(t, n_expert, n, k, seed)
        woff = WOFF.get(t, seed % 4) if woff is None else woff
        super().__init__(t, ids_h, n_expert, n, k, a_rows, seed=seed, w=MR.KR.dev_at(w_h, woff, 0xFF), w_h=w_h)
        self.bias_all_h = self.bias_all = self.bias_h = self.bias = None
        if bias:
            self.bias_all_h = BR.random_bias(np.random.default_rng([seed, n, n_expert]), n_expert, n, n + 3)
            self.bias_all = dev(self.bias_all_h)
            self.bias_h, self.bias = self.bias_all_h[1:-1, :n], self.bias_all[1:-1, :n]

    def config(self, qg):
        return qg.moe_prefill_bias_config(self.T, self.n_used, self.n_expert, self.n, self.k, self.t)

    def launch_guarded(self, qg, pad):
        import torch
        S = self.T * self.n_used
        buf = torch.full((S + 2, self.n + pad), F_SENT, dtype=torch.float32, device="cuda")
        out = buf[1:S + 1, :self.n].unflatten(0, (self.T, self.n_used))
        need = qg.moe_prefill_workspace_size(self.T, self.n_used, self.n_expert)
        ws, flat, start = guarded_workspace(need)
        got = qg.gemm_w4a8_moe_prefill_bias(self.a, self.w, self.bias, self.ids, self.T, self.n_used, self.n, self.k, self.t,
                                            a_rows=self.a_rows, workspace=ws, out=out)
        assert got.data_ptr() == out.data_ptr()
        whole, flat_h = host(buf), host(flat)
        assert (flat_h[:start] == 0xFF).all() and (flat_h[start + need:] == 0xFF).all(), "wrote outside the workspace"
        return whole[1:S + 1, :self.n].reshape(self.T, self.n_used, self.n).copy(), whole

    def biased_reference(self, qg, ids=None):
        """The eager MFMA product at the config's RG, then the float32 bias add."""
        ids = self.ids_h if ids is None else ids
        return BR.add_bias(self.reference(qg, ids), self.bias_h, ids, self.n_expert)

    def assert_close_to_contract(self, c):
        R = BR.ref_mod(self.t)
        for e in np.unique(self.ids_h):
            if 0 <= e < self.n_expert:
                sl = self.slots_of(e)
                a = self.a_all_h[[self.row_of(tt, u) for tt, u in sl]]
                c64, _, mag = R.gemm(a, self.w_h[e])
                ref, tol = BR.biased_tol(self.t, c64, mag, None if self.bias_h is None else self.bias_h[e], self.k)
                err = np.abs(np.stack([c[tt, u] for tt, u in sl]).astype(np.float64) - ref)
                assert (err <= tol).all(), (int(e), float((err / tol).max()))

    def check(self, qg, pad=None, contract=True):
        pad = 1 + (3 * self.n + self.T + self.k // 32) % 29 if pad is None else pad
        c, whole = self.launch_guarded(qg, pad)
        outside = np.ones(whole.shape, bool)
        outside[1:-1, :self.n] = False
        assert (whole[outside] == np.float32(F_SENT)).all(), f"wrote outside the slots' rows (ldc = {self.n + pad})"
        assert not np.isnan(c).any(), "a bias row or column outside the experts' was read"
        bad = [(tt, u) for tt in range(self.T) for u in range(self.n_used) if not 0 <= self.ids_h[tt, u] < self.n_expert]
        for tt, u in bad:
            assert (bits(c[tt, u]) == 0).all(), (tt, u)  # +0.0f: no bias, not -0.0f, not the sentinel
        ref = self.biased_reference(qg)
        diff = [(tt, u) for tt in range(self.T) for u in range(self.n_used) if not np.array_equal(bits(c[tt, u]), bits(ref[tt, u]))]
        assert not diff, f"{len(diff)} slots, first {diff[:6]}, differ from eager MFMA product + bias ({self.config(qg)})"
        if contract:
            self.assert_close_to_contract(c)
        _, again = self.launch_guarded(qg, pad)
        assert np.array_equal(bits(whole), bits(again))
        return c


def rg4_n(qg, t, T, n_used, n_expert, k):
    """The smallest ragged N = 64 j + 1 at which the biased prefill config of these slots names RG = 4."""
    cfg = lambda n: form_of(qg.moe_prefill_bias_config(T, n_used, n_expert, n, k, t))
    n = 65
    while cfg(n) != (4, 4):
        n += 64 * 8
        assert n <= 65 + 64 * 512, "the (4, 4) form is unreachable on this device"
    while n > 65 and cfg(n - 64) == (4, 4):
        n -= 64
    return n


def views(G, s, out, bias):
    """The ggml views of a case: experts, bias (or None), activations, ids, out."""
    bb, row = BR.BB[s.t], BR.expert_bytes(s.t, 1, s.k)
    w, b, a, i, o = G.TensorView(), G.TensorView(), G.TensorView(), G.TensorView(), G.TensorView()
    w.data, w.type = s.w.data_ptr(), s.t
    w.ne[:], w.nb[:] = [s.k, s.n, s.n_expert, 1], [bb, row, row * s.n, row * s.n * s.n_expert]
    arow = s.k // 32 * 36
    a.data, a.type = s.a.data_ptr(), G.Q8_1
    a.ne[:], a.nb[:] = [s.k, s.a_rows, s.T, 1], [36, arow, arow * s.a_rows, arow * s.a_rows * s.T]
    i.data, i.type = s.ids.data_ptr(), G.I32
    i.ne[:], i.nb[:] = [s.n_used, s.T, 1, 1], [4, 4 * s.ids.stride(0), 4 * s.ids.stride(0) * s.T, 4 * s.ids.stride(0) * s.T]
    o.data, o.type = out.data_ptr(), G.F32
    o.ne[:], o.nb[:] = [s.n, s.n_used, s.T, 1], [4, 4 * out.stride(1), 4 * out.stride(0), 4 * out.stride(0) * s.T]
    if bias is None:
        return w, None, a, i, o
    b.data, b.type = bias.data_ptr(), G.F32
    b.ne[:], b.nb[:] = [s.n, s.n_expert, 1, 1], [4, 4 * bias.stride(0), 4 * bias.stride(0) * s.n_expert, 4 * bias.stride(0) * s.n_expert]
    return w, b, a, i, o


# ---------------------------------------------------------------------------- 1. every form, the row counts around R
@pytest.mark.parametrize("form", FORMS)
def test_every_form_with_row_counts_around_the_tile(qg, form):
    """Six experts with 0, 1, R - 1, R, R + 1 and 2 R + 1 slots in one call (R = 16 TT). The RG = 1 forms at N = 17,
    K = 2912: 91 blocks are 12 groups, the last of 3 blocks, and a second pass of the eight slices with 4 busy; the expert
    stride 17 * 91 * 17 is odd, so the experts sit at all four byte offsets. RG = 4 at K = 352: two groups over KS = 2,
    the second of 3 blocks. The form is searched through the config, the test fails where it is not reached."""
    tt, rg = form
    R, k = 16 * tt, 352 if rg == 4 else 2912
    counts = [0, 1, R - 1, R, R + 1, 2 * R + 1]
    T = sum(counts)
    n = rg4_n(qg, MXFP4, T, 1, 6, k) if rg == 4 else 17
    cfg = qg.moe_prefill_bias_config(T, 1, 6, n, k, MXFP4)
    assert cfg.startswith("moe:mxfp4_mmq ") and form_of(cfg) == form and f"KS={8 // rg} R={R}" in cfg, cfg
    assert MR.cfg_fields(cfg)[1]["grid"] == f"{-(-n // (16 * rg))}x{T // R + 7}", cfg
    if rg == 1:
        assert BR.expert_bytes(MXFP4, n, k) % 2 == 1
    ids = ids_with_counts(np.random.default_rng(R), counts)
    BiasCase(MXFP4, ids, 6, n, k, a_rows=1, seed=tt + rg, woff=0).check(qg)


# ---------------------------------------------------------------------------- 2. K and N edges
@pytest.mark.parametrize("k", [32, 96, 256, 288, 2912])
@pytest.mark.parametrize("n", [1, 15, 17, 65])
def test_k_and_n_edges(qg, k, n):
    """K = 32: one block, seven idle slices; 96: a partial only group; 256: one whole group; 288: a whole group and one
    of a single block; 2912: a second pass. N around the 16-row group. The weight base at byte offsets 0 .. 3. Two used
    experts per token, a row per slot, in the (1, 1) and the (4, 1) form."""
    rng = np.random.default_rng([k, n])
    for j, (T, n_expert, want) in enumerate(((9, 3, (1, 1)), (50, 2, (4, 1)))):
        ids = rng.integers(0, n_expert, (T, 2)).astype(np.int32)
        c = BiasCase(MXFP4, ids, n_expert, n, k, a_rows=2, seed=k + n, woff=(k // 32 + n + 2 * j) % 4)
        assert form_of(c.config(qg)) == want
        c.check(qg)


def test_every_weight_offset_is_reached_by_the_edge_cases():
    assert {(k // 32 + n + 2 * j) % 4 for k in (32, 96, 256, 288, 2912) for n in (1, 15, 17, 65) for j in (0, 1)} == {0, 1, 2, 3}


# ---------------------------------------------------------------------------- 3. ids
def test_all_slots_on_one_expert(qg):
    ids = np.full((35, 2), 2, np.int32)
    c = BiasCase(MXFP4, ids, 4, 33, 1312, a_rows=1, woff=3)
    assert form_of(c.config(qg)) == (2, 1)  # 70 slots: three tiles of 32 rows, the last of 6
    c.check(qg)


def test_130_experts_most_of_them_empty(qg):
    rng = np.random.default_rng(130)
    ids = rng.choice([0, 3, 64, 128, 129], (20, 2)).astype(np.int32)
    BiasCase(MXFP4, ids, 130, 19, 544, a_rows=2, woff=1).check(qg)


@pytest.mark.parametrize("a_rows", [1, 3])
def test_repeated_and_invalid_ids(qg, a_rows):
    """Ids repeated within a token (a_rows 1: the slots share the token's row; a_rows n_used: a row each), ids of -1,
    n_expert and INT32_MIN in the middle: bit pattern 0 in exactly those rows (no bias), their neighbours unaffected."""
    rng = np.random.default_rng(7 + a_rows)
    T, n_expert = 30, 4
    ids = rng.integers(0, n_expert, (T, 3)).astype(np.int32)
    ids[:, 1] = ids[:, 0]
    ids[T // 2, 1], ids[T // 2 + 1, 0], ids[T // 3, 2] = -1, n_expert, -2 ** 31
    c = BiasCase(MXFP4, ids, n_expert, 21, 1312, a_rows=a_rows, woff=2)
    assert form_of(c.config(qg)) == (2, 1)
    out = c.check(qg)
    zero = [(tt, u) for tt in range(T) for u in range(3) if (bits(out[tt, u]) == 0).all()]
    assert zero == [(T // 3, 2), (T // 2, 1), (T // 2 + 1, 0)]


# ---------------------------------------------------------------------------- 4. null bias, and the K-quants
def test_mxfp4_null_bias_is_the_eager_product(qg):
    rng = np.random.default_rng(4)
    ids = rng.integers(0, 3, (21, 2)).astype(np.int32)
    c = BiasCase(MXFP4, ids, 3, 19, 416, a_rows=2, woff=1, bias=None)
    out = c.check(qg)
    assert np.array_equal(bits(out), bits(c.reference(qg)))


@pytest.mark.parametrize("t,T,want", [(Q4_K, 21, (1, 1)), (Q6_K, 21, (4, 4)), (Q4_K, 40, (2, 1))])
def test_kquants_are_the_old_entry_then_the_add(qg, t, T, want):
    """Null bias: bit-equal to qg_gemm_w4a8_moe_prefill on the same operands. With a bias: float32(old + bias)."""
    rng = np.random.default_rng([t, T])
    ids = rng.integers(-1, 3, (T, 2)).astype(np.int32)
    c = BiasCase(t, ids, 3, 19, 768, a_rows=2)
    assert form_of(c.config(qg)) == want and c.config(qg) == qg.moe_prefill_config(T, 2, 3, 19, 768, t)
    old = host(qg.gemm_w4a8_moe_prefill(c.a, c.w, c.ids, T, 2, 19, 768, t, a_rows=2))
    none = host(qg.gemm_w4a8_moe_prefill_bias(c.a, c.w, None, c.ids, T, 2, 19, 768, t, a_rows=2))
    assert np.array_equal(bits(none), bits(old))
    got = c.check(qg)
    assert np.array_equal(bits(got), bits(BR.add_bias(old, c.bias_h, ids, 3)))


# ---------------------------------------------------------------------------- 5. further behaviour
def test_token_order_does_not_reach_the_bits(qg):
    """The same slots with the tokens permuted (so every slot lands at another tile position): the same bits per slot."""
    rng = np.random.default_rng(11)
    T, n_used, n_expert, n, k = 45, 2, 3, 23, 1056
    ids = rng.integers(0, n_expert, (T, n_used)).astype(np.int32)
    base = BiasCase(MXFP4, ids, n_expert, n, k, a_rows=2, woff=3)
    c0 = base.check(qg, contract=False)
    perm = rng.permutation(T)
    p = BiasCase(MXFP4, ids[perm], n_expert, n, k, a_rows=2, woff=3)
    rows = (perm[:, None] * 2 + np.arange(2)[None]).reshape(-1)
    p.a_all_h = np.concatenate([base.a_all_h[rows], base.a_all_h[T * 2:]])
    p.a_all = dev(p.a_all_h)
    p.a = p.a_all[:T * 2].reshape(T, 2, k // 32, 36)
    c1, _ = p.launch_guarded(qg, 3)
    assert np.array_equal(bits(c1), bits(c0[perm]))


def test_captured_call_follows_the_ids_of_every_replay(qg):
    """One captured call; the ids are overwritten between replays with distributions that change every expert's count
    and the number of tiles, one of them with every id invalid."""
    import torch
    T, n_used, n_expert, n, k = 40, 2, 4, 19, 1312
    rng = np.random.default_rng(5)
    dists = [ids_with_counts(rng, c, n_used) for c in ([20, 20, 20, 20], [1, 3, 40, 36], [70, 0, 9, 1])]
    dists.append(np.full((T, n_used), -1, np.int32))
    dists.append(ids_with_counts(rng, [17, 33, 0, 30], n_used))
    c = BiasCase(MXFP4, dists[0], n_expert, n, k, a_rows=2, woff=1)
    assert form_of(c.config(qg)) == (2, 1)
    refs = [c.biased_reference(qg, d) for d in dists]
    out = torch.zeros((T, n_used, n), dtype=torch.float32, device="cuda")
    ws = torch.full((qg.moe_prefill_workspace_size(T, n_used, n_expert),), 0xFF, dtype=torch.uint8, device="cuda")
    call = lambda: qg.gemm_w4a8_moe_prefill_bias(c.a, c.w, c.bias, c.ids, T, n_used, n, k, MXFP4, a_rows=2, workspace=ws, out=out)
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


@pytest.mark.parametrize("with_bias", [True, False])
def test_view_entry_on_strided_ids_and_bias_views(qg, with_bias):
    import torch
    import quant_gemm.ggml as G
    ids = np.random.default_rng(3).integers(0, 16, (24, 2)).astype(np.int32)
    s = BiasCase(MXFP4, ids, 16, 21, 544, a_rows=2, woff=3, bias=with_bias or None)
    assert s.ids.stride(0) == 5 and not s.ids.is_contiguous()
    assert s.bias is None or (s.bias.stride(0) == 24 and not s.bias.is_contiguous())
    ref = s.biased_reference(qg)
    buf = torch.full((s.T, s.n_used, s.n + 3), F_SENT, dtype=torch.float32, device="cuda")
    out = buf[:, :, :s.n]
    ws = torch.full((qg.moe_prefill_workspace_size(s.T, s.n_used, 16),), 0xFF, dtype=torch.uint8, device="cuda")
    G.mul_mat_id_bias_from_ggml_ws(*views(G, s, out, s.bias), ws)
    got = host(buf)
    assert np.array_equal(bits(got[:, :, :s.n]), bits(ref)) and (got[:, :, s.n:] == F_SENT).all()
    if not with_bias:
        return
    # the refusals of the bias view, the output and the workspace untouched
    buf.fill_(F_SENT)
    ws.fill_(0xFF)
    for spoil, msg in (("type", "unsupported"), ("nb0", "unsupported"), ("nb1", "unsupported"), ("short", "unsupported"),
                       ("ne0", "invalid argument"), ("ne1", "invalid argument"), ("null", "invalid argument")):
        w, b, a, i, o = views(G, s, out, s.bias)
        if spoil == "type":
            b.type = G.I32
        elif spoil == "nb0":
            b.nb[0] = 8
        elif spoil == "nb1":
            b.nb[1] += 2
        elif spoil == "short":
            b.nb[1] = 4 * (s.n - 1)
        elif spoil == "ne0":
            b.ne[0] = s.n + 1
        elif spoil == "ne1":
            b.ne[1] = 15
        else:
            b.data = None
        with pytest.raises(RuntimeError, match=msg):
            G.mul_mat_id_bias_from_ggml_ws(w, b, a, i, o, ws)
    assert (host(buf) == F_SENT).all() and (host(ws) == 0xFF).all()


def test_refusals_on_real_buffers(qg):
    """Refused by the C entry with the output and the workspace untouched: a K off the granule, a row type, a bias off
    4 B, a bias stride below N, a workspace off its alignment or one byte short, an ldc below N; then the call itself,
    with the weights at an odd byte."""
    import torch
    import quant_gemm._lib as L
    P = ctypes.c_void_p
    ids = np.random.default_rng(9).integers(0, 4, (12, 2)).astype(np.int32)
    s = BiasCase(MXFP4, ids, 4, 9, 544, a_rows=1, woff=1)
    out = torch.full((s.T, s.n_used, s.n), F_SENT, dtype=torch.float32, device="cuda")
    need = qg.moe_prefill_workspace_size(s.T, s.n_used, 4)
    ws = torch.full((need + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    st = P(torch.cuda.current_stream().cuda_stream)
    call = lambda k=544, boff=0, bs=s.n + 3, ldc=0, wt=MXFP4, wsoff=0, wsb=need: L.load().qg_gemm_w4a8_moe_prefill_bias(
        P(s.a.data_ptr()), 1, P(s.w.data_ptr()), P(s.bias.data_ptr() + boff), bs, 4, P(s.ids_full.data_ptr()),
        s.ids_full.stride(0), P(out.data_ptr()), ldc, s.T, s.n_used, s.n, k, wt, P(ws.data_ptr() + wsoff), wsb, st)
    assert call(544 - 16) == -2
    assert call(wt=MR.Q4_0) == -3 and call(wt=MR.Q8_0) == -3 and call(wt=Q4_K) == -2
    assert call(boff=2) == -4 and call(boff=1, bs=1) == -4
    assert call(bs=s.n - 1) == -1 and call(bs=-1) == -1
    assert call(ldc=s.n - 1) == -1
    assert call(wsoff=4) == -4 and call(wsoff=8) == -4
    assert call(wsb=need - 1) == -1
    assert (host(out) == F_SENT).all() and (host(ws) == 0xFF).all()
    assert call() == 0
    assert np.array_equal(bits(host(out)), bits(s.biased_reference(qg)))
    assert (host(ws)[need:] == 0xFF).all()


# ---------------------------------------------------------------------------- 6. seeded sweep
def sweep_cases(count=16, seed=3916):
    rng = np.random.default_rng(seed)
    for i in range(count):
        n_used = int(rng.integers(1, 5))
        yield (i, int(rng.integers(1, 81)), n_used, int(rng.choice([1, 2, 3, 4, 6, 11, 25, 40])), int(rng.integers(1, 131)),
               32 * int(rng.integers(1, 97)), int(rng.choice([1, n_used])), i % 4, i % 3 != 2)


def test_seeded_sweep(qg):
    """16 seeded cases: T <= 80, n_used <= 4, 1 .. 40 experts (drawn from eight counts, so that the rows per expert
    reach three forms), N <= 130, K = 32 (1 .. 96), every weight offset, a null bias in about a third, ids from -1 to n_expert in a third, each through BiasCase.check."""
    seen, offs, nulls = set(), set(), 0
    for i, T, n_used, n_expert, n, k, a_rows, woff, bias in sweep_cases():
        ids = np.random.default_rng(i).integers(-1 if i % 3 == 0 else 0, n_expert + (i % 3 == 0), (T, n_used)).astype(np.int32)
        c = BiasCase(MXFP4, ids, n_expert, n, k, a_rows, seed=7000 + i, woff=woff, bias=bias or None)
        seen.add(form_of(c.config(qg)))
        offs.add(woff)
        nulls += not bias
        c.check(qg)
    assert len(seen) >= 3 and offs == {0, 1, 2, 3} and 4 <= nulls <= 6, (seen, offs, nulls)
