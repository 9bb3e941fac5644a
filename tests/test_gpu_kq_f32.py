"""qg_gemm_w4a8_f32_kq on the GPU: the Q4_K / Q6_K decode GEMV that quantizes its FP32 rows in the prologue.

Every shape is held to two bars: the bits of gemm_w4a8(quantize_q8_1(x), b) from the same library, and the float64 contract
(tests/kquant_ref.py, tests/q6k_ref.py) on the oracle's CPU quantization of x, |C - C64| <= 2 (K/32 + 2) 2^-24 mag (W = 0:
the decode GEMV's lane-serial sum). A relaunch is identical and nothing is written outside C. The grid reaches every
(MT, LPR, ONE) form; K = 256 at M = 1 is one wave's worth of blocks in a 256-thread workgroup, M = 8 at K = 4352 is 1088
blocks against 128 per round (a partial last round), N = 67 leaves partial row tiles.
"""
import ctypes
import functools

import numpy as np
import pytest

import kquant_ref as KR
import q6k_ref as QR

pytestmark = pytest.mark.gpu

Q4_K, Q6_K = 12, 14
REF = {Q4_K: (KR, KR.random_q4k), Q6_K: (QR, QR.random_q6k)}
MS, NS, KS = (1, 2, 3, 5, 8), (1, 67), (256, 512, 1024, 2304, 4096, 4352)
SENT, GUARD = -7.25, 64


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def corner_rows(m, k):
    """FP32 rows whose blocks hold, in turn: zeros (d = 0, id = 0); an amax that gives a subnormal f16 d; amax =
    127 * 65504 / 2 (d = 32752, elements in cancelling pairs so that s stays finite in f16); all negative; x * id on .5
    ties (amax = 127, so d = id = 1). Block (row, b) is of kind (row + b) % 5."""
    rng = np.random.default_rng([m, k])
    x = np.zeros((m, k // 32, 32), np.float32)
    half = np.arange(16, dtype=np.float32)
    for r in range(m):
        for b in range(k // 32):
            kind = (r + b) % 5
            if kind == 1:
                x[r, b] = rng.uniform(-1, 1, 32) * (127 * 3e-6)
                x[r, b, 5] = 127 * 3e-6
            elif kind == 2:
                x[r, b, 0::2] = (127 * 65504 / 2) / (1 + half)
                x[r, b, 1::2] = -x[r, b, 0::2]
            elif kind == 3:
                x[r, b] = rng.uniform(-2.0, -0.5, 32)
            elif kind == 4:
                x[r, b] = (rng.integers(-100, 100, 32) + 0.5) * rng.choice([-1.0, 1.0], 32)
                x[r, b, 31] = -127.0
    return x.reshape(m, k)


@functools.lru_cache(maxsize=None)
def operands(t, m, n, k, corners=False):
    """(x, b, C64, mag): computed once, shared, never modified. C64 is the contract on the oracle's quantization of x."""
    import oracle as O
    rng = np.random.default_rng([t, m, n, k])
    x = corner_rows(m, k) if corners else rng.uniform(-1, 1, (m, k)).astype(np.float32)
    b = REF[t][1](rng, n, k)
    c64, _, mag = REF[t][0].gemm(O.quantize(x, O.Q8_1).reshape(m, k // 32, 36), b)
    return x, b, c64, mag


def device(t, x, b, odd):
    """x 16 B past a 256-B boundary and Q6_K weights 2 B past one on odd cases; C between two guards of a flat buffer."""
    import torch
    xd = KR.dev_at(x.view(np.uint8), 16 * odd).view(torch.float32)
    bd = KR.dev_at(b, 2 * odd if t == Q6_K else 0)
    flat = torch.full((2 * GUARD + x.shape[0] * b.shape[0],), SENT, dtype=torch.float32, device="cuda")
    return xd, bd, flat, flat[GUARD:-GUARD].view(x.shape[0], b.shape[0])


def check(qg, t, m, n, k, corners=False):
    x, b, c64, mag = operands(t, m, n, k, corners)
    xd, bd, flat, out = device(t, x, b, (m + n + k // 256) % 2)
    qg.gemm_w4a8_f32_kq(xd, bd, t, out=out)
    first = host(flat).copy()
    c = first[GUARD:-GUARD].reshape(m, n)
    two_calls = host(qg.gemm_w4a8(qg.quantize_q8_1(xd), bd, m, n, k, t))
    err, tol = np.abs(c.astype(np.float64) - c64), KR.tol(mag, k, 0)
    print(f"{qg.f32_kq_config(m, n, k, t)}: max err/tol = {(err / tol).max():.3f}")
    assert np.array_equal(bits(c), bits(two_calls))
    assert (err <= tol).all()
    assert (first[:GUARD] == SENT).all() and (first[-GUARD:] == SENT).all()
    flat.fill_(SENT)
    qg.gemm_w4a8_f32_kq(xd, bd, t, out=out)
    assert np.array_equal(bits(host(flat)), bits(first))  # relaunch


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("t", (Q4_K, Q6_K))
def test_against_two_calls_and_contract(qg, t, m, n, k):
    check(qg, t, m, n, k)


@pytest.mark.parametrize("t", (Q4_K, Q6_K))
def test_quantizer_corners_through_the_product(qg, t):
    check(qg, t, 4, 67, 512, corners=True)


@pytest.mark.parametrize("t", (Q4_K, Q6_K))
def test_captured_call_is_one_kernel_node(qg, t):
    """One captured call is one kernel node; replays after X was overwritten in place give the eager result on the new X."""
    import torch
    m, n, k = 2, 67, 1024
    x, b, _, _ = operands(t, m, n, k)
    xd, bd, flat, out = device(t, x, b, 1)
    qg.gemm_w4a8_f32_kq(xd, bd, t, out=out)  # (warm: module load outside the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        qg.gemm_w4a8_f32_kq(xd, bd, t, out=out)
    hip, count = qg._lib.load(), ctypes.c_size_t(0)
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    assert hip.hipGraphGetNodes(graph.raw_cuda_graph(), None, ctypes.byref(count)) == 0 and count.value == 1
    graph.instantiate()
    for seed in (5, 6, 7):
        xd.copy_(torch.from_numpy(np.random.default_rng(seed).uniform(-1, 1, (m, k)).astype(np.float32)))
        flat.fill_(SENT)
        graph.replay()
        assert np.array_equal(bits(host(out)), bits(host(qg.gemm_w4a8_f32_kq(xd, bd, t))))
        assert (host(flat)[:GUARD] == SENT).all() and (host(flat)[-GUARD:] == SENT).all()
