"""qg_gemm_w4a8_moe_glu_batch on the GPU ("moeb_glu:q4k_gemv", "moeb_glu:q6k_gemv", "moeb_glu:mxfp4_gemv"). The reference
operands are g and u of two qg_gemm_w4a8_moe calls: ReGLU equals moe_ffn_bias_ref.glu_model on them bit for bit, SwiGLU and
gpt-oss's op stay inside moe_glu_ref.assert_swiglu / moe_ffn_bias_ref.assert_oai of the float64 evaluation, and every op
equals qg_gemm_w4a8_moe_glu_bias bit for bit. Every call writes into the interior of a sentinel-filled buffer with a
workspace of exactly the size function's bytes inside 0xFF bytes, twice."""
import functools

import numpy as np
import pytest

import moe_ffn_bias_ref as FR
import moe_glu_ref as GR
import mxfp4_ref as XR
from moe_ffn_bias_ref import MXFP4, REGLU, SWIGLU, SWIGLU_OAI, bits
from moe_ref import Q4_K, Q6_K, random_act
from test_gpu_moe import F_SENT, dev, host
from test_gpu_moe_batch import fields, rows_of, rows_per_workgroup
from test_gpu_moe_prefill import guarded_workspace, ids_with_counts

pytestmark = pytest.mark.gpu

KQ_K = (256, 512, 1024, 1280, 4096, 4352)  # LPR 4 / 16 / 64, each loop-free and looped (tests/test_gpu_moe_batch.py)
MX_K = (32, 160, 512, 544, 2048, 2912)     # the same six forms by K / 32 units: one block; 5, 17 and 91 are odd
assert len({FR.mxfp4_form(k) for k in MX_K}) == 6
OPS = ((REGLU, 1.702, 7.0), (SWIGLU, 1.702, 7.0), (SWIGLU_OAI, 1.702, 7.0), (SWIGLU_OAI, 1.0, 0.5))
N_USED = 2


@functools.lru_cache(maxsize=4)
def operands(t, n_expert, T, n, k):
    """Host arrays, never modified: gate and up experts [2][n_expert, n, blocks, bytes] (g and u fall on both sides of
    the OAI clamps), one activation row per token, the two biases [2][n_expert, n + 5]."""
    rng = np.random.default_rng([t, n_expert, T, n, k])
    w = np.stack([FR.small_experts(rng, t, n_expert, n, k) for _ in range(2)])
    bias = rng.uniform(-10.0, 10.0, (2, n_expert, n + 5)).astype(np.float32)
    bias[:, :, n:] = np.nan  # the gap is never read
    return w, random_act(rng, T, k), bias


class Call:
    """One shape on the device. ids rows are N_USED + 3 apart, bias rows N + 5, C rows N + 3; MXFP4 experts start 1 and
    3 bytes past a 256-B line (with an odd expert stride the experts then sit at every byte offset)."""

    def __init__(self, qg, t, ids_h, n_expert, n, k):
        self.qg, self.t, self.n_expert, self.n, self.k = qg, t, n_expert, n, k
        self.T = ids_h.shape[0]
        w, a, bias = operands(t, n_expert, self.T, n, k)
        put = (lambda x, o: XR.dev_at(x, o)) if t == MXFP4 else (lambda x, o: dev(x))
        self.gate, self.up, self.a = put(w[0], 1), put(w[1], 3), dev(a)
        self.bias_h = bias
        self.bias_full = dev(bias)
        self.bg, self.bu = self.bias_full[0][:, :n], self.bias_full[1][:, :n]
        full = np.full((self.T, N_USED + 3), 12345, np.int32)  # the columns past n_used are never read
        self.ids_full = dev(full)
        self.ids = self.ids_full[:, :N_USED]
        self.set_ids(ids_h)

    def set_ids(self, ids_h):
        self.ids_h = np.ascontiguousarray(ids_h, np.int32)
        self.ids.copy_(dev(self.ids_h))  # in place: a captured graph holds the pointer
        self.ok = (self.ids_h >= 0) & (self.ids_h < self.n_expert)

    def shape(self):
        return self.ids, self.T, N_USED, self.n, self.k, self.t

    def ups(self, up):
        return self.up if up is None else up

    def products(self, up=None):
        return tuple(host(self.qg.gemm_w4a8_moe(self.a, w, *self.shape())).copy() for w in (self.gate, self.ups(up)))

    def decode(self, op, alpha, limit, bg, bu, up=None):
        return host(self.qg.gemm_w4a8_moe_glu_bias(self.a, self.gate, self.ups(up), bg, bu, *self.shape(), op, alpha, limit))

    def launch(self, op, alpha, limit, bg, bu, up=None):
        """Two guarded launches with identical bits -> the [T, n_used, N] window."""
        import torch
        S, n, outs = self.T * N_USED, self.n, []
        need = self.qg.moe_batch_workspace_size(self.T, N_USED, self.n_expert)
        for _ in range(2):
            buf = torch.full((S + 2, n + 3), F_SENT, dtype=torch.float32, device="cuda")
            ws, flat, start = guarded_workspace(need)
            self.qg.gemm_w4a8_moe_glu_batch(self.a, self.gate, self.ups(up), *self.shape(), op, bg, bu, alpha, limit,
                                            workspace=ws, out=buf[1:S + 1, :n].unflatten(0, (self.T, N_USED)))
            whole, flat_h = host(buf), host(flat)
            assert (flat_h[:start] == 0xFF).all() and (flat_h[start + need:] == 0xFF).all(), "wrote outside the workspace"
            assert (whole[0] == F_SENT).all() and (whole[-1] == F_SENT).all() and (whole[:, n:] == F_SENT).all()
            outs.append(whole[1:S + 1, :n].reshape(self.T, N_USED, n).copy())
        assert np.array_equal(bits(outs[0]), bits(outs[1])), "two launches differ"
        return outs[0]

    def check(self, g, u, bg=True, bu=True, up=None, ops=OPS):
        """Every op of `ops` against the model on (g, u) and against the decode entry."""
        dbg, dbu = self.bg if bg else None, self.bu if bu else None
        hbg, hbu = self.bias_h[0] if bg else None, self.bias_h[1] if bu else None
        want, gb, ub = FR.glu_model(g, u, hbg, hbu, self.ids_h, self.n_expert)
        ok = self.ok
        for op, alpha, limit in ops:
            got = self.launch(op, alpha, limit, dbg, dbu, up)
            assert (bits(got[~ok]) == 0).all(), "an invalid slot is not +0.0f"
            if op == REGLU:
                assert np.array_equal(bits(got), bits(want))
            elif op == SWIGLU:
                GR.assert_swiglu(got[ok], gb[ok], ub[ok], "moe_glu_batch")
            else:
                FR.assert_oai(got[ok], gb[ok], ub[ok], alpha, limit, "moe_glu_batch")
            assert np.array_equal(bits(got), bits(self.decode(op, alpha, limit, dbg, dbu, up))), op
        return got


def ids_around_the_tile(rng, r, n_expert):
    """Experts with 0, 1, R - 1, R, R + 1 and 2 R + 1 slots, one id of -1 and one of n_expert, shuffled: 5 R + 4 slots."""
    flat = np.concatenate([ids_with_counts(rng, [0, 1, r - 1, r, r + 1, 2 * r + 1]).ravel(), np.int32([-1, n_expert])])
    return rng.permutation(flat).reshape(-1, N_USED)


@pytest.mark.parametrize("r", (2, 4, 8))
@pytest.mark.parametrize("t,k", [(t, k) for t in (Q4_K, Q6_K) for k in KQ_K] + [(MXFP4, k) for k in MX_K])
def test_every_form_and_tile_size(qg, t, k, r):
    """Each type x (LPR, ONE) form x R with the row counts around the tile, at N = 17 and one either side of a
    workgroup's rows; the config line's fields are the batch entry's."""
    T = (5 * r + 4) // N_USED  # the smallest n_expert >= 6 (the further experts stay empty) at which the config names R = r
    n_expert = next(e for e in range(6, 40) if rows_of(qg.moe_glu_batch_config(T, N_USED, e, 17, k, t)) == r)
    cfg = qg.moe_glu_batch_config(T, N_USED, n_expert, 17, k, t)
    assert cfg.startswith("moeb_glu:") and fields(cfg) == fields(qg.moe_batch_bias_config(T, N_USED, n_expert, 17, k, t))
    if t == MXFP4:
        assert (int(fields(cfg)["LPR"]), int(fields(cfg)["WGS"]), int(fields(cfg)["ONE"])) == FR.mxfp4_form(k)
    rpb = rows_per_workgroup(cfg)
    ids = ids_around_the_tile(np.random.default_rng([r, k]), r, n_expert)
    for n in (17, rpb - 1, rpb + 1):
        c = Call(qg, t, ids, n_expert, n, k)
        c.check(*c.products())


@pytest.mark.parametrize("bg,bu,alias", [(False, False, False), (True, False, False), (False, True, False), (True, True, True)])
@pytest.mark.parametrize("t,k", [(Q4_K, 1280), (Q6_K, 4352), (MXFP4, 2912)])
def test_null_biases_and_aliased_experts(qg, t, k, bg, bu, alias):
    """A null bias is no add (ReGLU of g <= 0 and u < 0 keeps its -0.0f), each bias null on its own, B_up = B_gate."""
    ids = ids_around_the_tile(np.random.default_rng(k), 4, 6)
    c = Call(qg, t, ids, 6, 19, k)
    up = c.gate if alias else None
    got = c.check(*c.products(up), bg=bg, bu=bu, up=up, ops=OPS[:1] + OPS[2:3])
    if not (bg or bu):
        assert (bits(c.launch(REGLU, 0.0, 0.0, None, None)) == 0x80000000).any()


def test_captured_call_follows_the_ids_of_every_replay(qg):
    """Capture once, replay, overwrite the ids on the device with a distribution that changes the rows per expert,
    replay again: each replay equals the eager call on the ids it found. Two nodes in a line, no parallel branch."""
    import torch
    T, n_expert, n, k = 12, 4, 19, 2912
    rng = np.random.default_rng(5)
    dists = [ids_with_counts(rng, cnt, N_USED) for cnt in ([6, 6, 6, 6], [1, 3, 12, 8], [20, 0, 3, 1])]
    dists.append(np.full((T, N_USED), -1, np.int32))
    c = Call(qg, MXFP4, dists[0], n_expert, n, k)
    assert rows_of(qg.moe_glu_batch_config(T, N_USED, n_expert, n, k, MXFP4)) == 8
    out = torch.zeros((T, N_USED, n), dtype=torch.float32, device="cuda")
    ws = torch.full((qg.moe_batch_workspace_size(T, N_USED, n_expert),), 0xFF, dtype=torch.uint8, device="cuda")
    call = lambda o: qg.gemm_w4a8_moe_glu_batch(c.a, c.gate, c.up, *c.shape(), SWIGLU_OAI, c.bg, c.bu, workspace=ws, out=o)
    call(out)  # (warm: module load outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(out)
    for d in dists + dists[:1]:
        c.set_ids(d)
        out.fill_(F_SENT)
        g.replay()
        assert np.array_equal(bits(host(out)), bits(host(call(None))))
