"""qg_gemm_w4a8_moe_batch_bias on the GPU: the expert-grouped decode GEMV with MXFP4 experts ("moeb:mxfp4_gemv") and a
per-expert bias added to the finished product, Q4_K / Q6_K beside it.

The harness is tests/test_gpu_moe_batch.py's on the operands of tests/test_gpu_moe_prefill_bias.py's BiasCase: guarded
output, workspace and expert tensor, the bias inside NaN rows and columns, every case launched twice (identical bits).
The reference is qg_gemm_w4a8_moe on the same operands, bit for bit, then the float32 bias add; every case is also held
against the type's NumPy model with the decode GEMV's bound (W = 0) plus 2^-24 |product + bias| for the add.
"""
import numpy as np
import pytest

import moe_id_bias_ref as BR
import moe_ref as MR
from moe_id_bias_ref import MXFP4, Q4_K, Q6_K
from test_gpu_moe import F_SENT, bits, dev, host
from test_gpu_moe_batch import fields, rows_of, rows_per_workgroup
from test_gpu_moe_prefill import guarded_workspace, ids_with_counts
from test_gpu_moe_prefill_bias import BiasCase, views

pytestmark = pytest.mark.gpu

ROWS = (2, 4, 8)
FORM_K = (96, 544, 2912)  # the three rungs of kq_gemv_form_units: LPR 4 (ONE), LPR 16 (17 units: the loop), LPR 64 (the loop)


class BatchBiasCase(BiasCase):
    def config(self, qg):
        return qg.moe_batch_bias_config(self.T, self.n_used, self.n_expert, self.n, self.k, self.t)

    def launch_guarded(self, qg, pad):
        import torch
        S = self.T * self.n_used
        buf = torch.full((S + 2, self.n + pad), F_SENT, dtype=torch.float32, device="cuda")
        out = buf[1:S + 1, :self.n].unflatten(0, (self.T, self.n_used))
        need = qg.moe_batch_workspace_size(self.T, self.n_used, self.n_expert)
        ws, flat, start = guarded_workspace(need)
        got = qg.gemm_w4a8_moe_batch_bias(self.a, self.w, self.bias, self.ids, self.T, self.n_used, self.n, self.k, self.t,
                                          a_rows=self.a_rows, workspace=ws, out=out)
        assert got.data_ptr() == out.data_ptr()
        whole, flat_h = host(buf), host(flat)
        assert (flat_h[:start] == 0xFF).all() and (flat_h[start + need:] == 0xFF).all(), "wrote outside the workspace"
        return whole[1:S + 1, :self.n].reshape(self.T, self.n_used, self.n).copy(), whole

    def reference(self, qg, ids=None, rg=None):
        """float32 [T, n_used, N]: qg_gemm_w4a8_moe on the same operands (zeros where the id names no expert)."""
        ids_d = self.ids
        if ids is not None:
            full = host(self.ids_full).copy()
            full[:, :self.n_used] = ids
            ids_d = dev(full)[:, :self.n_used]
        return host(qg.gemm_w4a8_moe(self.a, self.w, ids_d, self.T, self.n_used, self.n, self.k, self.t, a_rows=self.a_rows))

    def assert_close_to_contract(self, c):
        R = BR.ref_mod(self.t)
        for e in np.unique(self.ids_h):
            if 0 <= e < self.n_expert:
                sl = self.slots_of(e)
                a = self.a_all_h[[self.row_of(tt, u) for tt, u in sl]]
                c64, _, mag = R.gemm(a, self.w_h[e])
                ref = c64 if self.bias_h is None else c64 + self.bias_h[e].astype(np.float64)[None]
                tol = R.tol(mag, self.k, 0) + (0.0 if self.bias_h is None else 2.0 ** -24 * np.abs(ref))
                err = np.abs(np.stack([c[tt, u] for tt, u in sl]).astype(np.float64) - ref)
                assert (err <= tol).all(), (int(e), float((err / tol).max()))


def experts_for_rows(qg, slots, n_used, r, n, k, at_least):
    """The smallest n_expert >= at_least (the further experts stay empty) at which the config of these slots names R = r."""
    for n_expert in range(at_least, at_least + 64):
        if rows_of(qg.moe_batch_bias_config(slots // n_used, n_used, n_expert, n, k, MXFP4)) == r:
            return n_expert
    raise AssertionError(f"no n_expert in [{at_least}, {at_least + 64}) gives R = {r} for {slots} slots at K = {k}")


# ---------------------------------------------------------------------------- 1. every R, the row counts around R
@pytest.mark.parametrize("r", ROWS)
@pytest.mark.parametrize("k", FORM_K)
def test_every_r_with_row_counts_around_the_tile(qg, r, k):
    """Experts with 0, 1, R - 1, R, R + 1 and 2 R + 1 slots in one call, at each rung of the body's ladder, with N one
    below and one above a workgroup's rows, and N = 1: N * K/32 * 17 is odd for odd N and odd K/32, so the experts sit
    at all four byte offsets. The n_expert (6 to 8) at which the config names R is searched through the config."""
    counts = [0, 1, r - 1, r, r + 1, 2 * r + 1]
    T = sum(counts)
    n_expert = experts_for_rows(qg, T, 1, r, 17, k, 6)
    assert n_expert <= 8
    counts += [0] * (n_expert - 6)
    cfg = qg.moe_batch_bias_config(T, 1, n_expert, 17, k, MXFP4)
    f, single = fields(cfg), fields(qg.moe_config(T, 1, 17, k, MXFP4))
    assert cfg.startswith("moeb:mxfp4_gemv ") and rows_of(cfg) == r
    assert (f["LPR"], f["WGS"], f["ONE"]) == (single["LPR"], single["WGS"], single["ONE"])
    assert (int(f["LPR"]), int(f["WGS"]), int(f["ONE"])) == BR.mxfp4_form(k) == {96: (4, 256, 1), 544: (16, 512, 0), 2912: (64, 1024, 0)}[k]
    rpb = rows_per_workgroup(cfg)
    ids = ids_with_counts(np.random.default_rng(r), counts)
    for j, n in enumerate((rpb - 1, rpb + 1, 1)):
        g = fields(qg.moe_batch_bias_config(T, 1, n_expert, n, k, MXFP4))
        assert g["grid"] == f"{-(-n // rpb)}x{T // r + n_expert + 1}" and int(g["lds"]) == r * (k // 32) * 48, g
        assert BR.expert_bytes(MXFP4, n, k) % 2 == 1
        BatchBiasCase(MXFP4, ids, n_expert, n, k, a_rows=1, seed=r, woff=(r + j) % 4).check(qg)


def test_loop_free_form_at_16_and_64_lanes(qg):
    """K = 512 and 2048: ONE at LPR 16 and 64, which the three rungs above reach only with the unit loop."""
    for k, lpr in ((512, 16), (2048, 64)):
        ids = np.random.default_rng(k).integers(0, 3, (11, 2)).astype(np.int32)
        c = BatchBiasCase(MXFP4, ids, 3, 37, k, a_rows=2, woff=1)
        f = fields(c.config(qg))
        assert (int(f["LPR"]), int(f["ONE"]), int(f["R"])) == (lpr, 1, 8)
        c.check(qg)


# ---------------------------------------------------------------------------- 2. ids
@pytest.mark.parametrize("a_rows", [1, 3])
def test_repeated_and_invalid_ids(qg, a_rows):
    rng = np.random.default_rng(7 + a_rows)
    T, n_expert = 14, 4
    ids = rng.integers(0, n_expert, (T, 3)).astype(np.int32)
    ids[:, 1] = ids[:, 0]
    ids[T // 2, 1], ids[T // 2 + 1, 0], ids[T // 3, 2] = -1, n_expert, -2 ** 31
    c = BatchBiasCase(MXFP4, ids, n_expert, 21, 1312, a_rows=a_rows, woff=3)
    assert c.ids.stride(0) == 6 and rows_of(c.config(qg)) == 8
    out = c.check(qg)
    zero = [(tt, u) for tt in range(T) for u in range(3) if (bits(out[tt, u]) == 0).all()]
    assert zero == [(T // 3, 2), (T // 2, 1), (T // 2 + 1, 0)]


def test_every_id_invalid(qg):
    ids = np.array([[-1, 5], [7, -3], [2 ** 31 - 1, 5], [-2 ** 31, 6], [5, 5]], np.int32)
    out = BatchBiasCase(MXFP4, ids, 5, 33, 544, a_rows=2, woff=2).check(qg)
    assert (bits(out) == 0).all()


def test_130_experts_most_of_them_empty(qg):
    rng = np.random.default_rng(130)
    ids = rng.choice([0, 3, 64, 128, 129], (20, 2)).astype(np.int32)
    c = BatchBiasCase(MXFP4, ids, 130, 19, 544, a_rows=2, woff=1)
    assert rows_of(c.config(qg)) == 2
    c.check(qg)


# ---------------------------------------------------------------------------- 3. null bias, and the K-quants
def test_mxfp4_null_bias_is_qg_gemm_w4a8_moe(qg):
    ids = np.random.default_rng(4).integers(-1, 3, (9, 2)).astype(np.int32)
    c = BatchBiasCase(MXFP4, ids, 3, 19, 416, a_rows=2, woff=1, bias=None)
    out = c.check(qg)
    assert np.array_equal(bits(out), bits(c.reference(qg)))


@pytest.mark.parametrize("t", [Q4_K, Q6_K])
def test_kquants_are_the_old_entry_then_the_add(qg, t):
    """Null bias: bit-equal to qg_gemm_w4a8_moe_batch on the same operands. With a bias: float32(old + bias)."""
    T, k = 9, 1280
    ids = np.random.default_rng([t, T]).integers(-1, 3, (T, 2)).astype(np.int32)
    c = BatchBiasCase(t, ids, 3, 35, k, a_rows=2)
    assert c.config(qg) == qg.moe_batch_config(T, 2, 3, 35, k, t) and rows_of(c.config(qg)) == 8
    old = host(qg.gemm_w4a8_moe_batch(c.a, c.w, c.ids, T, 2, 35, k, t, a_rows=2))
    none = host(qg.gemm_w4a8_moe_batch_bias(c.a, c.w, None, c.ids, T, 2, 35, k, t, a_rows=2))
    assert np.array_equal(bits(none), bits(old))
    got = c.check(qg)
    assert np.array_equal(bits(got), bits(BR.add_bias(old, c.bias_h, ids, 3)))


# ---------------------------------------------------------------------------- 4. capture, views
def test_captured_call_follows_the_ids_of_every_replay(qg):
    import torch
    T, n_used, n_expert, n, k = 12, 2, 4, 19, 1312
    rng = np.random.default_rng(5)
    dists = [ids_with_counts(rng, c, n_used) for c in ([6, 6, 6, 6], [1, 3, 12, 8], [20, 0, 3, 1])]
    dists.append(np.full((T, n_used), -1, np.int32))
    dists.append(ids_with_counts(rng, [5, 9, 0, 10], n_used))
    c = BatchBiasCase(MXFP4, dists[0], n_expert, n, k, a_rows=2, woff=1)
    assert rows_of(c.config(qg)) == 8
    refs = [c.biased_reference(qg, d) for d in dists]
    out = torch.zeros((T, n_used, n), dtype=torch.float32, device="cuda")
    ws = torch.full((qg.moe_batch_workspace_size(T, n_used, n_expert),), 0xFF, dtype=torch.uint8, device="cuda")
    call = lambda: qg.gemm_w4a8_moe_batch_bias(c.a, c.w, c.bias, c.ids, T, n_used, n, k, MXFP4, a_rows=2, workspace=ws, out=out)
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


def test_view_entry_on_strided_ids_and_bias_views(qg):
    import torch
    import quant_gemm.ggml as G
    ids = np.random.default_rng(3).integers(0, 16, (8, 2)).astype(np.int32)
    s = BatchBiasCase(MXFP4, ids, 16, 21, 544, a_rows=2, woff=3)
    assert s.ids.stride(0) == 5 and s.bias.stride(0) == 24
    ref = s.biased_reference(qg)
    buf = torch.full((s.T, s.n_used, s.n + 3), F_SENT, dtype=torch.float32, device="cuda")
    out = buf[:, :, :s.n]
    ws = torch.full((qg.moe_batch_workspace_size(s.T, s.n_used, 16),), 0xFF, dtype=torch.uint8, device="cuda")
    G.mul_mat_id_bias_from_ggml_batch(*views(G, s, out, s.bias), ws)
    got = host(buf)
    assert np.array_equal(bits(got[:, :, :s.n]), bits(ref)) and (got[:, :, s.n:] == F_SENT).all()
    buf.fill_(F_SENT)
    G.mul_mat_id_bias_from_ggml_batch(*views(G, s, out, None), ws)
    assert np.array_equal(bits(host(buf)[:, :, :s.n]), bits(s.reference(qg)))
    buf.fill_(F_SENT)
    with pytest.raises(RuntimeError, match="invalid argument"):
        G.mul_mat_id_bias_from_ggml_batch(*views(G, s, out, s.bias), ws[:-1])
    w, b, a, i, o = views(G, s, out, s.bias)
    b.nb[1] = 4 * (s.n - 1)
    with pytest.raises(RuntimeError, match="unsupported"):
        G.mul_mat_id_bias_from_ggml_batch(w, b, a, i, o, ws)
    assert (host(buf) == F_SENT).all()


# ---------------------------------------------------------------------------- 5. seeded sweep
def sweep_cases(count=12, seed=4220):
    rng = np.random.default_rng(seed)
    for i in range(count):
        n_used = int(rng.integers(1, 5))
        yield (i, int(rng.integers(1, 33)), n_used, int(rng.choice([1, 3, 8, 40])), int(rng.integers(1, 131)),
               32 * int(rng.integers(1, 97)), int(rng.choice([1, n_used])), i % 4, i % 3 != 2)


def test_seeded_sweep(qg):
    """12 seeded cases: T <= 32, n_used <= 4, 1 .. 40 experts, N <= 130, K = 32 (1 .. 96), every weight offset, a null
    bias in a third, ids from -1 to n_expert in a third, each through BatchBiasCase.check."""
    seen = set()
    for i, T, n_used, n_expert, n, k, a_rows, woff, bias in sweep_cases():
        ids = np.random.default_rng(i).integers(-1 if i % 3 == 0 else 0, n_expert + (i % 3 == 0), (T, n_used)).astype(np.int32)
        c = BatchBiasCase(MXFP4, ids, n_expert, n, k, a_rows, seed=8000 + i, woff=woff, bias=bias or None)
        seen.add(rows_of(c.config(qg)))
        c.check(qg)
    assert seen == {2, 4, 8}, seen
