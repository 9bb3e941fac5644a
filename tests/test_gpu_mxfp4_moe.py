"""qg_gemm_w4a8_moe with MXFP4 experts (family "moe:mxfp4_gemv") on the GPU: every slot bit-identical to the eager M = 1
qg_gemm_w4a8 on its activation row and expert, ids read on the device, experts at any byte offset.

The expert stride is N * K/32 * 17 bytes: with N = 67 and K = 2912 (or 96) it is odd, so consecutive experts sit at all
four byte offsets in a dword; the experts tensor itself starts 0..3 bytes past a 256-B boundary.
"""
import ctypes
import functools

import numpy as np
import pytest

import mxfp4_ref as MR

pytestmark = pytest.mark.gpu

MXFP4 = 39
F_SENT = -7.5  # fills an output before a call that must not touch it
SLOTS = ((4, 2, 1), (8, 4, 3), (32, 4, 8))  # (n_expert, n_used, T)


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


@functools.lru_cache(maxsize=None)
def operands(n_expert, n_used, T, n, k, a_rows):
    """Experts, activations and ids of one step (host arrays, shared, never modified). The ids cover -1 and n_expert
    once there are four slots; the ids rows are n_used + 3 apart."""
    rng = np.random.default_rng([n_expert, n_used, T, n, k, a_rows])
    w = MR.random_mxfp4(rng, n_expert * n, k).reshape(n_expert, n, k // 32, 17)
    a = MR.random_q8_1(rng, T * a_rows, k).reshape(T, a_rows, k // 32, 36)
    ids = np.full((T, n_used + 3), 12345, np.int32)  # the columns past n_used are never read
    ids[:, :n_used] = rng.integers(0, n_expert, (T, n_used))
    if T * n_used >= 4:
        ids[0, 1], ids[T - 1, 0] = -1, n_expert
    return w, a, ids


def reference(qg, w_d, a_d, ids_h, n_expert, n_used, T, n, k, a_rows):
    """Slot (t, u): the eager M = 1 product on the slot's own operands (device views of the very buffers), zeros for
    an id that names no expert."""
    out = np.zeros((T, n_used, n), np.float32)
    for t in range(T):
        for u in range(n_used):
            e = int(ids_h[t, u])
            if 0 <= e < n_expert:
                out[t, u] = host(qg.gemm_w4a8(a_d[t, u % a_rows], w_d[e], 1, n, k, MXFP4))[0]
    return out


@pytest.mark.parametrize("a_rows_is_n_used", [False, True])
@pytest.mark.parametrize("n,k", [(67, 96), (200, 96), (67, 2880), (200, 2880), (67, 2912), (200, 2912)])
@pytest.mark.parametrize("n_expert,n_used,T", SLOTS)
def test_slots_are_the_eager_products(qg, n_expert, n_used, T, n, k, a_rows_is_n_used):
    import torch
    a_rows = n_used if a_rows_is_n_used else 1
    w, a, ids_h = operands(n_expert, n_used, T, n, k, a_rows)
    woff = (n + k // 32 + T) % 4
    w_d, a_d = MR.dev_at(w, woff), dev(a)
    if n == 67 and k in (96, 2912):
        assert {(w_d[e].data_ptr()) % 4 for e in range(4)} == {0, 1, 2, 3}
    ids_full = dev(ids_h)
    ids = ids_full[:, :n_used]
    assert ids.stride(0) == n_used + 3
    cfg = qg.moe_config(T, n_used, n, k, MXFP4)
    assert cfg.startswith("moe:mxfp4_gemv ") and f"x{T * n_used} " in cfg, cfg
    out = torch.full((T, n_used, n), F_SENT, dtype=torch.float32, device="cuda")
    qg.gemm_w4a8_moe(a_d, w_d, ids, T, n_used, n, k, MXFP4, a_rows=a_rows, out=out)
    got = host(out)
    want = reference(qg, w_d, a_d, ids_h, n_expert, n_used, T, n, k, a_rows)
    assert np.array_equal(bits(got), bits(want))
    if T * n_used >= 4:
        assert (bits(got[0, 1]) == 0).all() and (bits(got[T - 1, 0]) == 0).all()  # +0.0f, not -0.0f
    # against the model too, so that "identical" is not "identically wrong"
    t, u = T - 1, n_used - 1
    c64, _, mag = MR.gemm(a[t, u % a_rows][None], w[int(ids_h[t, u])])
    assert (np.abs(got[t, u].astype(np.float64) - c64[0]) <= MR.tol(mag[0], k, 0)).all()


def test_captured_once_replayed_with_changed_ids(qg):
    import torch
    n_expert, n_used, T, n, k = 8, 4, 3, 67, 2912
    w, a, ids_h = operands(n_expert, n_used, T, n, k, 1)
    w_d, a_d = MR.dev_at(w, 3), dev(a)
    ids_full = dev(ids_h)
    ids = ids_full[:, :n_used]
    ids2_h = ids_h.copy()
    ids2_h[:, :n_used] = (ids_h[:, :n_used][:, ::-1] + 1) % n_expert
    ids2_h[1, 2] = n_expert  # an id out of range that was in range on the first replay
    ref1 = reference(qg, w_d, a_d, ids_h, n_expert, n_used, T, n, k, 1)
    ref2 = reference(qg, w_d, a_d, ids2_h, n_expert, n_used, T, n, k, 1)
    assert not np.array_equal(bits(ref1), bits(ref2))
    out = torch.zeros((T, n_used, n), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        qg.gemm_w4a8_moe(a_d, w_d, ids, T, n_used, n, k, MXFP4, a_rows=1, out=out)
    for h, ref in ((ids_h, ref1), (ids2_h, ref2)):
        ids_full.copy_(dev(h))  # in place: the graph holds the pointer
        out.fill_(F_SENT)
        g.replay()
        assert np.array_equal(bits(host(out)), bits(ref))


def test_view_entry_equals_the_plain_one(qg):
    import torch
    import quant_gemm.ggml as G
    n_expert, n_used, T, n, k = 8, 4, 3, 67, 2912
    for a_rows in (1, n_used):
        w, a, ids_h = operands(n_expert, n_used, T, n, k, a_rows)
        w_d, a_d = MR.dev_at(w, 1), dev(a)
        ids_full = dev(ids_h)
        ids = ids_full[:, :n_used]
        plain = host(qg.gemm_w4a8_moe(a_d, w_d, ids, T, n_used, n, k, MXFP4, a_rows=a_rows))
        buf = torch.full((T, n_used, n + 3), F_SENT, dtype=torch.float32, device="cuda")
        out = buf[:, :, :n]
        row = k // 32 * 17
        arow = k // 32 * 36
        wv, av, iv, ov = G.TensorView(), G.TensorView(), G.TensorView(), G.TensorView()
        wv.data, wv.type = w_d.data_ptr(), G.MXFP4
        wv.ne[:], wv.nb[:] = [k, n, n_expert, 1], [17, row, row * n, row * n * n_expert]
        av.data, av.type = a_d.data_ptr(), G.Q8_1
        av.ne[:], av.nb[:] = [k, a_rows, T, 1], [36, arow, arow * a_rows, arow * a_rows * T]
        iv.data, iv.type = ids.data_ptr(), G.I32
        iv.ne[:], iv.nb[:] = [n_used, T, 1, 1], [4, 4 * ids.stride(0), 4 * ids.stride(0) * T, 4 * ids.stride(0) * T]
        ov.data, ov.type = out.data_ptr(), G.F32
        ov.ne[:], ov.nb[:] = [n, n_used, T, 1], [4, 4 * out.stride(1), 4 * out.stride(0), 4 * out.stride(0) * T]
        G.mul_mat_id_from_ggml(wv, av, iv, ov)
        got = host(buf)
        assert np.array_equal(bits(got[:, :, :n]), bits(plain)) and (got[:, :, n:] == F_SENT).all()
        wv.nb[2] += 1  # experts a byte further apart than dense: not expressible
        buf.fill_(F_SENT)
        with pytest.raises(RuntimeError, match="unsupported"):
            G.mul_mat_id_from_ggml(wv, av, iv, ov)
        assert (host(buf) == F_SENT).all()


def test_the_other_expert_entries_refuse_mxfp4_on_real_buffers(qg):
    """Prefill, batch, GLU and down: -3 for type 39 with real operands, C untouched."""
    import torch
    import quant_gemm._lib as L
    P = ctypes.c_void_p
    so = L.load()
    n_expert, n_used, T, n, k = 8, 4, 3, 64, 512
    w, a, ids_h = operands(n_expert, n_used, T, n, k, n_used)
    w_d, a_d, ids = dev(w), dev(a), dev(np.ascontiguousarray(ids_h[:, :n_used]))
    out = torch.full((T, n_used, n), F_SENT, dtype=torch.float32, device="cuda")
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    st = P(torch.cuda.current_stream().cuda_stream)
    p = lambda t: P(t.data_ptr())
    assert so.qg_gemm_w4a8_moe_prefill(p(a_d), n_used, p(w_d), n_expert, p(ids), n_used, p(out), 0, T, n_used, n, k, MXFP4,
                                       p(ws), ws.numel(), st) == -3
    assert so.qg_gemm_w4a8_moe_batch(p(a_d), n_used, p(w_d), n_expert, p(ids), n_used, p(out), 0, T, n_used, n, k, MXFP4,
                                     p(ws), ws.numel(), st) == -3
    assert so.qg_gemm_w4a8_moe_glu(p(a_d), p(w_d), p(w_d), n_expert, p(ids), n_used, p(out), 0, T, n_used, n, k, MXFP4, 2,
                                   st) == -3
    assert so.qg_gemm_w4a8_moe_down(p(a_d), p(w_d), n_expert, p(ids), n_used, None, n_used, p(out), 0, T, n_used, n, k,
                                    MXFP4, st) == -3
    assert (host(out) == F_SENT).all()
    # and the served entry on the same operands, so that the buffers are shown to be good ones
    got = host(qg.gemm_w4a8_moe(a_d, w_d, ids, T, n_used, n, k, MXFP4, a_rows=n_used))
    assert np.array_equal(bits(got), bits(reference(qg, w_d, a_d, ids_h, n_expert, n_used, T, n, k, n_used)))
