"""Capture-time merge of back-to-back GEMVs (csrc/qg_capture_fuse.hip capture_gemv; qg.h at qg_gemm_w4a8).

Under stream capture, consecutive independent qg_gemm_w4a8 GEMVs of one M, K and weight type become ONE
grouped kernel node. Bar: every output of the graph replay equals the eager calls on the same inputs bit for
bit (torch.equal on the int32 view), and the library's counters (qg_capture_fusion_stats: calls merged into
an existing node, nodes started) say exactly which calls merged: independent ones do — calls - ceil(calls/64)
of them — and nothing that carries a dependency (same output, output read as the next activations, a kernel
in between), differs in M, K or weight type, or runs with the merge switched off.

Shapes: K = 256 (4-lane rows, 64-row workgroups) and 4096 (one wave per row); N = 40 and 48 (ragged last
tile, half-filled two-tile workgroup) and 4096 (the grid's full width); M = 1, 2, 4; Q4_0, Q5_1, Q8_0.
"""
import math

import pytest

pytestmark = pytest.mark.gpu

BB = {2: 18, 3: 20, 6: 22, 7: 24, 8: 34}


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


@pytest.fixture(autouse=True)
def _fusion_on(qg):
    qg.set_capture_fusion(1)
    yield
    qg.set_capture_fusion(1)


def _f16_field(torch, gen, shape, lo, hi):
    x = (torch.rand(shape, generator=gen, device="cuda") * (hi - lo) + lo).to(torch.float16)
    return x.view(torch.uint8).reshape(shape + (2,))


def acts(torch, gen, m, k):
    """Random Q8_1 rows [m, k/32, 36] with finite scales (as test_gpu_product.random_blocks)."""
    a = torch.randint(0, 256, (m, k // 32, 36), dtype=torch.uint8, device="cuda", generator=gen)
    a[..., 0:2] = _f16_field(torch, gen, (m, k // 32), 1e-3, 2e-2)
    a[..., 2:4] = _f16_field(torch, gen, (m, k // 32), -5.0, 5.0)
    return a


def weights(torch, gen, count, n, k, t):
    """`count` distinct random weight matrices [count, n, k/32, block bytes] with finite scales."""
    w = torch.randint(0, 256, (count, n, k // 32, BB[t]), dtype=torch.uint8, device="cuda", generator=gen)
    w[..., 0:2] = _f16_field(torch, gen, (count, n, k // 32), -0.1, 0.1)
    if t in (3, 7):
        w[..., 2:4] = _f16_field(torch, gen, (count, n, k // 32), -0.5, 0.5)
    return w


def gen_(torch, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def bits_equal(torch, a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def captured(torch, qg, fn, replays=2, before_replay=None):
    """Capture fn() into a graph, replay it; returns (merged, nodes) the capture added to the counters."""
    torch.cuda.synchronize()
    s0 = qg.capture_fusion_stats()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    s1 = qg.capture_fusion_stats()
    for _ in range(replays):
        if before_replay is not None:
            before_replay()
        g.replay()
    torch.cuda.synchronize()
    assert qg.capture_fusion_stats() == s1  # replays do not count
    return s1[0] - s0[0], s1[1] - s0[1]


def eager(torch, qg, fn):
    """fn() outside capture: never merged, the counters stay."""
    s0 = qg.capture_fusion_stats()
    r = fn()
    torch.cuda.synchronize()
    assert qg.capture_fusion_stats() == s0
    return r


CALLS = [2, 3, 64, 65, 130]
INDEPENDENT = [(CALLS[i % len(CALLS)], t, m, n, k) for i, (t, m, k, n) in enumerate(
    (t, m, k, n) for t in (2, 7, 8) for m in (1, 2, 4) for k in (256, 4096) for n in (40, 48, 4096))]
# every call count at the headline shape class as well (one wave per row, full grid)
INDEPENDENT += [(c, 2, 1, 4096, 4096) for c in CALLS]


@pytest.mark.parametrize("calls,t,m,n,k", INDEPENDENT)
def test_independent_gemvs_merge(torch_, qg, calls, t, m, n, k):
    torch = torch_
    gen = gen_(torch, calls * 1000 + t * 100 + m * 10 + n + k)
    a = acts(torch, gen, m, k)
    w = weights(torch, gen, calls, n, k, t)
    ref = eager(torch, qg, lambda: torch.stack([qg.gemm_w4a8(a, w[i], m, n, k, t) for i in range(calls)]))
    out = torch.full((calls, m, n), float("nan"), dtype=torch.float32, device="cuda")

    def step():
        for i in range(calls):
            qg.gemm_w4a8(a, w[i], m, n, k, t, out=out[i])
    first = []
    merged, nodes = captured(torch, qg, step, replays=2,
                             before_replay=lambda: (first.append(out.clone()), out.fill_(float("nan"))))
    assert merged == calls - math.ceil(calls / 64) and nodes == math.ceil(calls / 64)
    assert bits_equal(torch, out, ref)       # the second replay
    assert bits_equal(torch, first[1], ref)  # the first replay (cloned before the second)


@pytest.mark.parametrize("m,k,t,merges", [(1, 8192, 2, True), (1, 8192, 8, True), (1, 3072, 2, True),
                                          (2, 8192, 2, False), (4, 8192, 7, False), (2, 3072, 2, False),
                                          (4, 2048, 2, True)])
def test_gate_by_shape_class(torch_, qg, m, k, t, merges):
    """The unit-loop form (more units per row than its lanes: K > 4096, K = 3072) merges at M = 1 only — M >= 2
    measured slower merged (csrc/qg_capture_fuse.hip fuse_class_enabled) — and with the gate lifted (mode 2) everything
    merges; the bits are the eager calls' in all three graphs."""
    torch = torch_
    n, calls = 48, 3
    gen = gen_(torch, 900 + m * 10 + t + k)
    a = acts(torch, gen, m, k)
    w = weights(torch, gen, calls, n, k, t)
    ref = eager(torch, qg, lambda: torch.stack([qg.gemm_w4a8(a, w[i], m, n, k, t) for i in range(calls)]))
    out = torch.zeros((calls, m, n), dtype=torch.float32, device="cuda")

    def step():
        for i in range(calls):
            qg.gemm_w4a8(a, w[i], m, n, k, t, out=out[i])
    for mode, want in ((1, calls - 1 if merges else 0), (2, calls - 1), (0, 0)):
        qg.set_capture_fusion(mode)
        merged, nodes = captured(torch, qg, step, before_replay=out.zero_)
        assert (merged, nodes) == (want, calls - want), mode
        assert bits_equal(torch, out, ref), mode


def test_strided_outputs_one_row_merge_more_rows_conservative(torch_, qg):
    """Column slices of one wide buffer: with M = 1 the outputs are disjoint and merge; with M = 2 each item's
    single conservative C span ((M-1) * ldc + N floats) covers its neighbours' first rows, so they stay
    separate nodes. Correct either way, and nothing is written outside the slices."""
    torch = torch_
    n, k, t, cnt = 48, 4096, 2, 3
    for m, want in ((1, cnt - 1), (2, 0)):
        gen = gen_(torch, 77 + m)
        a = acts(torch, gen, m, k)
        w = weights(torch, gen, cnt, n, k, t)
        ref = eager(torch, qg, lambda: [qg.gemm_w4a8(a, w[i], m, n, k, t) for i in range(cnt)])
        wide = torch.full((m, cnt * n + 5), float("nan"), dtype=torch.float32, device="cuda")

        def step():
            for i in range(cnt):
                qg.gemm_w4a8(a, w[i], m, n, k, t, out=wide[:, i * n:(i + 1) * n])
        merged, nodes = captured(torch, qg, step)
        assert (merged, nodes) == (want, cnt - want)
        for i in range(cnt):
            assert bits_equal(torch, wide[:, i * n:(i + 1) * n], ref[i])
        assert torch.isnan(wide[:, cnt * n:]).all()


def test_write_after_write_not_merged(torch_, qg):
    torch = torch_
    m, n, k, t = 1, 4096, 4096, 2
    gen = gen_(torch, 1)
    a = acts(torch, gen, m, k)
    w = weights(torch, gen, 2, n, k, t)
    ref = eager(torch, qg, lambda: qg.gemm_w4a8(a, w[1], m, n, k, t))
    out = torch.zeros((m, n), dtype=torch.float32, device="cuda")

    def step():
        qg.gemm_w4a8(a, w[0], m, n, k, t, out=out)
        qg.gemm_w4a8(a, w[1], m, n, k, t, out=out)
    merged, nodes = captured(torch, qg, step, before_replay=out.zero_)
    assert (merged, nodes) == (0, 2)
    assert bits_equal(torch, out, ref)  # the second one's


def test_read_after_write_by_aliasing_not_merged(torch_, qg):
    """The first GEMV's output buffer (4096 floats) IS the second's activation pointer (its first 4608 bytes
    read as 128 Q8_1 blocks)."""
    torch = torch_
    m, n, k, t = 1, 4096, 4096, 2
    gen = gen_(torch, 2)
    a = acts(torch, gen, m, k)
    w = weights(torch, gen, 2, n, k, t)

    def chain(out1, out2):
        qg.gemm_w4a8(a, w[0], m, n, k, t, out=out1)
        a2 = out1.view(torch.uint8)[:, :(k // 32) * 36].view(m, k // 32, 36)
        assert a2.data_ptr() == out1.data_ptr()
        qg.gemm_w4a8(a2, w[1], m, n, k, t, out=out2)
    r1, r2 = (torch.zeros((m, n), dtype=torch.float32, device="cuda") for _ in range(2))
    eager(torch, qg, lambda: chain(r1, r2))
    o1, o2 = (torch.zeros((m, n), dtype=torch.float32, device="cuda") for _ in range(2))
    merged, nodes = captured(torch, qg, lambda: chain(o1, o2), before_replay=lambda: (o1.zero_(), o2.zero_()))
    assert (merged, nodes) == (0, 2)
    assert bits_equal(torch, o1, r1) and bits_equal(torch, o2, r2)


def test_intervening_kernel_not_merged(torch_, qg):
    """GEMV -> quantize_q8_1 of its output -> GEMV: the second GEMV's capture dependency is the quantizer."""
    torch = torch_
    m, n, k, t = 1, 4096, 4096, 2
    gen = gen_(torch, 3)
    a = acts(torch, gen, m, k)
    w = weights(torch, gen, 2, n, k, t)

    def chain(out1, out2):
        qg.gemm_w4a8(a, w[0], m, n, k, t, out=out1)
        qg.gemm_w4a8(qg.quantize_q8_1(out1), w[1], m, n, k, t, out=out2)
    r1, r2 = (torch.zeros((m, n), dtype=torch.float32, device="cuda") for _ in range(2))
    eager(torch, qg, lambda: chain(r1, r2))
    o1, o2 = (torch.zeros((m, n), dtype=torch.float32, device="cuda") for _ in range(2))
    merged, nodes = captured(torch, qg, lambda: chain(o1, o2), before_replay=lambda: (o1.zero_(), o2.zero_()))
    assert (merged, nodes) == (0, 2)
    assert bits_equal(torch, o1, r1) and bits_equal(torch, o2, r2)


def test_mixed_m_k_wtype_not_merged(torch_, qg):
    torch = torch_
    n = 48
    seq = [(1, 4096, 2), (2, 4096, 2), (2, 256, 2), (2, 256, 8), (1, 256, 8), (1, 4096, 8), (1, 4096, 7), (1, 4096, 2)]
    gen = gen_(torch, 4)
    ins = [(acts(torch, gen, m, k), weights(torch, gen, 1, n, k, t)[0]) for m, k, t in seq]
    ref = eager(torch, qg, lambda: [qg.gemm_w4a8(a, w, m, n, k, t) for (a, w), (m, k, t) in zip(ins, seq)])
    outs = [torch.zeros((m, n), dtype=torch.float32, device="cuda") for m, _, _ in seq]

    def step():
        for (a, w), (m, k, t), o in zip(ins, seq, outs):
            qg.gemm_w4a8(a, w, m, n, k, t, out=o)
    merged, nodes = captured(torch, qg, step)
    assert (merged, nodes) == (0, len(seq))
    for o, r in zip(outs, ref):
        assert bits_equal(torch, o, r)


def test_forked_stream_reads_first_output(torch_, qg):
    """A side stream forked after the first GEMV reads its output while the capturing stream goes on with two
    more GEMVs (merged into the first one's node: the side stream's kernel then waits for all three), then joins."""
    torch = torch_
    m, n, k, t = 1, 4096, 4096, 2
    gen = gen_(torch, 5)
    a = acts(torch, gen, m, k)
    w = weights(torch, gen, 3, n, k, t)
    ref = eager(torch, qg, lambda: torch.stack([qg.gemm_w4a8(a, w[i], m, n, k, t) for i in range(3)]))
    out = torch.zeros((3, m, n), dtype=torch.float32, device="cuda")
    doubled = torch.zeros((m, n), dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()

    def step():
        main = torch.cuda.current_stream()
        qg.gemm_w4a8(a, w[0], m, n, k, t, out=out[0])
        side.wait_stream(main)
        with torch.cuda.stream(side):
            torch.mul(out[0], 2.0, out=doubled)
        qg.gemm_w4a8(a, w[1], m, n, k, t, out=out[1])
        qg.gemm_w4a8(a, w[2], m, n, k, t, out=out[2])
        main.wait_stream(side)
    merged, nodes = captured(torch, qg, step, before_replay=lambda: (out.zero_(), doubled.zero_()))
    assert (merged, nodes) == (2, 1)
    assert bits_equal(torch, out, ref)
    assert bits_equal(torch, doubled, ref[0] * 2.0)


@pytest.mark.parametrize("calls", [3, 65])
def test_opt_out(torch_, qg, calls):
    torch = torch_
    m, n, k, t = 1, 48, 4096, 2
    gen = gen_(torch, 6)
    a = acts(torch, gen, m, k)
    w = weights(torch, gen, calls, n, k, t)
    ref = eager(torch, qg, lambda: torch.stack([qg.gemm_w4a8(a, w[i], m, n, k, t) for i in range(calls)]))
    out = torch.zeros((calls, m, n), dtype=torch.float32, device="cuda")

    def step():
        for i in range(calls):
            qg.gemm_w4a8(a, w[i], m, n, k, t, out=out[i])
    qg.set_capture_fusion(0)
    merged, nodes = captured(torch, qg, step, before_replay=out.zero_)
    assert (merged, nodes) == (0, calls)
    assert bits_equal(torch, out, ref)
    qg.set_capture_fusion(1)  # and back on: the same calls merge again
    merged, nodes = captured(torch, qg, step, before_replay=out.zero_)
    assert (merged, nodes) == (calls - math.ceil(calls / 64), math.ceil(calls / 64))
    assert bits_equal(torch, out, ref)


def test_lone_gemv_and_eager_calls(torch_, qg):
    torch = torch_
    m, n, k, t = 1, 4096, 4096, 2
    gen = gen_(torch, 7)
    a = acts(torch, gen, m, k)
    w = weights(torch, gen, 2, n, k, t)
    ref = eager(torch, qg, lambda: [qg.gemm_w4a8(a, w[i], m, n, k, t) for i in range(2)])  # counters stay
    out = torch.zeros((m, n), dtype=torch.float32, device="cuda")
    merged, nodes = captured(torch, qg, lambda: qg.gemm_w4a8(a, w[0], m, n, k, t, out=out), before_replay=out.zero_)
    assert (merged, nodes) == (0, 1)
    assert bits_equal(torch, out, ref[0])
    # a record left by one capture never matches the next capture (capture ids are unique)
    out2 = torch.zeros((m, n), dtype=torch.float32, device="cuda")
    merged, nodes = captured(torch, qg, lambda: qg.gemm_w4a8(a, w[1], m, n, k, t, out=out2), before_replay=out2.zero_)
    assert (merged, nodes) == (0, 1)
    assert bits_equal(torch, out2, ref[1]) and bits_equal(torch, out, ref[0])
