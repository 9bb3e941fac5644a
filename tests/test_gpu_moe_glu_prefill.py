"""qg_gemm_w4a8_moe_glu_prefill on the GPU against g and u from qg.gemm_w4a8_moe_prefill on the gate and the up experts
(one RG in both config lines): ReGLU bit for bit, SwiGLU within moe_glu_ref.assert_swiglu. Launches write through out=
into a sentinel-filled buffer, the workspace a guarded 0xFF window of the size function's bytes; a second launch agrees."""
import ctypes

import numpy as np
import pytest

import moe_glu_ref as GR
import moe_ref as MR
from moe_glu_ref import REGLU, SWIGLU
from moe_ref import Q4_K, Q6_K
from test_gpu_moe import F_SENT, bits, dev, host
from test_gpu_moe_glu import views
from test_gpu_moe_prefill import TYPES, W_MMQ, WOFF, Case, guarded_workspace, ids_with_counts, operands, ref_mod, rg4_n

pytestmark = pytest.mark.gpu
OPS = (REGLU, SWIGLU)


class Pair(Case):
    """A Case (a row per token, ids with spare columns) as the gate tensor, and an up tensor; both WOFF[t] past a 256-B line."""

    def __init__(self, t, ids_h, n_expert, n, k, seed=0, fill=0xFF):
        super().__init__(t, ids_h, n_expert, n, k, a_rows=1, seed=seed)
        self.gate_h, self.up_h = self.w_h, operands(t, n_expert, n, k, 1, seed + 1000)[0]
        self.gate, self.up = (MR.KR.dev_at(w, WOFF[t], fill) for w in (self.gate_h, self.up_h))
        self.a = self.a.reshape(self.T, k // 32, 36)
        self.args = (self.T, self.n_used, n, k, t)

    def rg(self, qg):
        new, old = (MR.cfg_fields(f(self.T, self.n_used, self.n_expert, self.n, self.k, self.t))[1]
                    for f in (qg.moe_glu_prefill_config, qg.moe_prefill_config))
        assert new["RG"] == old["RG"] and new["KS"] == old["KS"], (new, old)
        return int(new["RG"]), int(new["R"])

    def products(self, qg, gate=None, up=None):
        return tuple(host(qg.gemm_w4a8_moe_prefill(self.a, w, self.ids, *self.args)).copy()
                     for w in (self.gate if gate is None else gate, self.up if up is None else up))

    def launch(self, qg, op, pad=3, gate=None, up=None):
        import torch
        S = self.T * self.n_used
        buf = torch.full((S + 2, self.n + pad), F_SENT, dtype=torch.float32, device="cuda")
        out = buf[1:S + 1, :self.n].unflatten(0, (self.T, self.n_used))
        need = qg.moe_prefill_workspace_size(self.T, self.n_used, self.n_expert)
        ws, flat, start = guarded_workspace(need)
        got = qg.gemm_w4a8_moe_glu_prefill(self.a, self.gate if gate is None else gate, self.up if up is None else up,
                                           self.ids, *self.args, op, workspace=ws, out=out)
        assert got.data_ptr() == out.data_ptr()
        whole, flat_h = host(buf), host(flat)
        assert (flat_h[:start] == 0xFF).all() and (flat_h[start + need:] == 0xFF).all(), "wrote outside the workspace"
        assert (whole[[0, -1]] == F_SENT).all() and (whole[:, self.n:] == F_SENT).all(), "wrote outside the slots' rows"
        return whole[1:S + 1, :self.n].reshape(self.T, self.n_used, self.n).copy(), whole

    def check(self, qg, ops=OPS, gate=None, up=None):
        self.rg(qg)
        g, u = self.products(qg, gate, up)
        res = []
        for op in ops:
            c, whole = self.launch(qg, op, gate=gate, up=up)
            bad = ~((self.ids_h >= 0) & (self.ids_h < self.n_expert))
            assert (bits(c[bad]) == 0).all() and (bits(g[bad]) == 0).all()  # +0.0f, not -0.0f, not the sentinel
            if op == REGLU:
                assert np.array_equal(bits(c), bits(GR.reglu(g, u)))
            else:
                GR.assert_swiglu(c, g, u, f"t={self.t} N={self.n} K={self.k}")
            assert np.array_equal(bits(whole), bits(self.launch(qg, op, gate=gate, up=up)[1]))
            res.append(c)
        return res


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("rg", [1, 4])
def test_every_form_with_row_counts_around_the_tile(qg, t, rg):
    """Six experts with 0, 1, R - 1, R, R + 1 and 2 R + 1 slots, R from the new config line. The fused tile is R = 16
    in every form, and 82 slots over six experts stay below the 32 per expert from which Q4_K's rule names RG = 4: there
    a seventh expert takes 8 R + 15 more, the six counts as they are. The test fails where the form is not reached."""
    k = 768 if rg == 4 else 1280
    R = int(MR.cfg_fields(qg.moe_glu_prefill_config(64, 1, 6, 17, k, t))[1]["R"])
    counts = [0, 1, R - 1, R, R + 1, 2 * R + 1] + ([8 * R + 15] if rg == 4 else [])
    n = rg4_n(qg, Q4_K, sum(counts), 1, len(counts), k) if rg == 4 else 17  # (the N of the rule both types share)
    p = Pair(t, ids_with_counts(np.random.default_rng(R), counts), len(counts), n, k, seed=rg)
    assert p.rg(qg) == (rg, R)
    p.check(qg)


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("k,n", [(256, 1), (256, 65), (768, 15), (2304, 17)])
def test_k_and_n_edges(qg, t, k, n):
    """One super-block and a second pass of the slices, N around the row group; ids a view with spare columns of valid ids."""
    rng = np.random.default_rng([k, n])
    for T, n_expert in ((9, 3), (50, 2)):
        p = Pair(t, rng.integers(0, n_expert, (T, 2)).astype(np.int32), n_expert, n, k, seed=k + n)
        assert p.ids.stride(0) == 5
        p.check(qg)


@pytest.mark.parametrize("t", TYPES)
def test_ids_and_operands(qg, t):
    """Repeated ids with -1 and n_expert mid-step (bit pattern 0); one expert for all; gate and up swapped; B_up is B_gate."""
    rng, T, n_expert = np.random.default_rng(7), 30, 4
    ids = rng.integers(0, n_expert, (T, 3)).astype(np.int32)
    ids[:, 1] = ids[:, 0]
    ids[T // 2, 1], ids[T // 2 + 1, 0] = -1, n_expert
    p = Pair(t, ids, n_expert, 21, 1280)
    c = p.check(qg)[0]
    assert [(tt, u) for tt in range(T) for u in range(3) if (bits(c[tt, u]) == 0).all()] == [(T // 2, 1), (T // 2 + 1, 0)]
    assert not np.array_equal(bits(c), bits(p.check(qg, gate=p.up, up=p.gate)[0]))
    g = p.products(qg)[0]
    assert np.array_equal(bits(p.check(qg, up=p.gate)[0]), bits(GR.reglu(g, g)))
    Pair(t, np.full((35, 2), 2, np.int32), 4, 33, 1280).check(qg)


@pytest.mark.parametrize("t", TYPES)
def test_reglu_against_the_model(qg, t):
    """test_gpu_moe_glu.test_reglu_against_the_model's bound at the MFMA tolerances; G, U the float64 NumPy contract."""
    R = ref_mod(t)
    p = Pair(t, np.random.default_rng(20).integers(-1, 4, (20, 2)).astype(np.int32), 3, 37, 1024)
    c = p.launch(qg, REGLU)[0]
    live = [(tt, u, int(p.ids_h[tt, u])) for tt in range(p.T) for u in range(p.n_used) if 0 <= p.ids_h[tt, u] < p.n_expert]
    assert len(live) >= 4
    for tt, u, e in live:
        row = p.a_all_h[tt].reshape(1, -1, 36)
        (G, _, mg), (U, _, mu) = R.gemm(row, p.gate_h[e]), R.gemm(row, p.up_h[e])
        tg, tu = R.tol(mg, p.k, W_MMQ[t]), R.tol(mu, p.k, W_MMQ[t])
        bound = tg * np.abs(U) + tu * np.abs(G) + tg * tu + 2.0 ** -23 * np.abs(G * U)
        err = np.abs(c[tt, u].astype(np.float64) - (np.maximum(G, 0.0) * U)[0])
        assert (err <= bound[0]).all(), float((err / bound[0]).max())


@pytest.mark.parametrize("t", TYPES)
def test_weights_at_the_alignment_classes(qg, t):
    """Both tensors at the type's offset past a 256-B line inside 0xFF bytes, then 0x00: the same bits."""
    ids, res = np.random.default_rng(5).integers(0, 3, (12, 2)).astype(np.int32), []
    for fill in (0xFF, 0x00):
        p = Pair(t, ids, 3, 19, 768, fill=fill)
        assert p.gate.data_ptr() % 256 == WOFF[t] and p.up.data_ptr() % 256 == WOFF[t]
        res.append(p.check(qg))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(*res))


@pytest.mark.parametrize("t", TYPES)
def test_captured_call_follows_the_ids_of_every_replay(qg, t):
    import torch
    T, n_used, n_expert, rng = 40, 2, 4, np.random.default_rng(5)
    dists = [ids_with_counts(rng, c, n_used) for c in ([1, 3, 40, 36], [70, 0, 9, 1])]
    dists[1][T // 2, 1] = n_expert  # an id out of range that was in range on the first replay
    p = Pair(t, dists[0], n_expert, 19, 1280)
    out = torch.zeros((T, n_used, p.n), dtype=torch.float32, device="cuda")
    ws = torch.full((qg.moe_prefill_workspace_size(T, n_used, n_expert),), 0xFF, dtype=torch.uint8, device="cuda")
    call = lambda: qg.gemm_w4a8_moe_glu_prefill(p.a, p.gate, p.up, p.ids, *p.args, SWIGLU, workspace=ws, out=out)
    refs = [None, None]
    for i in (1, 0):  # (eager, and warm: the module is loaded outside the capture)
        p.ids_full[:, :n_used].copy_(dev(dists[i]))
        refs[i] = host(call()).copy()
    assert not np.array_equal(bits(refs[0]), bits(refs[1])) and (bits(refs[1][T // 2, 1]) == 0).all()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for d, ref in list(zip(dists, refs)) * 2:
        p.ids_full[:, :n_used].copy_(dev(d))  # in place: the graph holds the pointer
        out.fill_(F_SENT)
        g.replay()
        assert np.array_equal(bits(host(out)), bits(ref))


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("op", OPS)
def test_c_abi_view_entry_and_python_agree(qg, t, op):
    import torch
    import quant_gemm._lib as L
    import quant_gemm.ggml as G
    P = ctypes.c_void_p
    s = Pair(t, np.random.default_rng(9).integers(0, 4, (12, 2)).astype(np.int32), 4, 21, 512)
    py = s.check(qg, (op,))[0]
    buf = torch.full((s.T, s.n_used, s.n + 3), F_SENT, dtype=torch.float32, device="cuda")
    need = qg.moe_prefill_workspace_size(s.T, s.n_used, 4)
    ws = torch.full((need + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    st = P(torch.cuda.current_stream().cuda_stream)
    call = lambda k=s.k, uoff=0, ldc=s.n + 3, glu_op=op, wsb=need: L.load().qg_gemm_w4a8_moe_glu_prefill(
        P(s.a.data_ptr()), P(s.gate.data_ptr()), P(s.up.data_ptr() + uoff), 4, P(s.ids_full.data_ptr()),
        s.ids_full.stride(0), P(buf.data_ptr()), ldc, s.T, s.n_used, s.n, k, t, glu_op, P(ws.data_ptr()), wsb, st)
    assert (call(k=s.k - 32), call(uoff=1 if t == Q6_K else 8), call(ldc=s.n - 1), call(glu_op=1), call(wsb=need - 1)) == (-2, -4, -1, -3, -1)
    assert (host(buf) == F_SENT).all() and (host(ws) == 0xFF).all()
    assert call() == 0  # the C ABI on raw pointers, ldc > N
    same = lambda got: np.array_equal(bits(got[:, :, :s.n]), bits(py)) and (got[:, :, s.n:] == F_SENT).all()
    assert same(host(buf)) and (host(ws)[need:] == 0xFF).all()
    buf.fill_(F_SENT)
    G.mul_mat_id_glu_from_ggml_ws(*views(G, s, buf[:, :, :s.n]), op, ws)
    assert same(host(buf))
    with pytest.raises(RuntimeError, match="unsupported"):
        G.mul_mat_id_glu_from_ggml_ws(*views(G, s, buf[:, :, :s.n]), 1, ws)
