"""Q6_K x Q8_1 on the GPU: the decode GEMV (q6k_gemv, M <= 8) and the MFMA prefill (q6k_mmq, M >= 9) against the
NumPy contract (tests/q6k_ref.py).

isum (qg_debug_sumi) must be bit-equal; every fp32 output must satisfy |c - C64| <= 2 (K/32 + W + 2) 2^-24 mag with
W = 0 for q6k_gemv and 8 for q6k_mmq (QR.tol); two launches must give identical bits.

Shapes and what they reach (qg.debug_config; tests/test_q6k_cpu.py::test_every_instantiation_has_a_shape checks the
list): K = 256 puts every odd row 2 B off a dword, K = 768 alternates the parity along and between rows, K = 512 keeps
row starts aligned with odd super-blocks shifted; N = 1 / 15 / 17 / 33 leave partial row tiles.
  q6k_gemv MT = 1, 2, 4 (M = 3, 4), 8 (M = 5, 8) with
    LPR=4 ONE=1    K = 256            LPR=4 ONE=0    K = 768
    LPR=16 ONE=1   K = 1024           LPR=16 ONE=0   K = 1280
    LPR=64 ONE=1   K = 4096           LPR=64 ONE=0   K = 4352;   M = 8, K = 6912: LDS records above 64 KiB
  q6k_mmq  TT=1 RG=1 M = 9, 16 (and the forced M = 8)   TT=2 RG=1 M = 17   TT=4 RG=1 M = 33, 64
           TT=4 RG=4 M = 65, N = 8200 (130 x 2 tiles of 64 x 64 fill 256 CUs)
  tests/test_gpu_q6k_paths.py: RG=4 with data in both K slices, the prefetch loops, gridDim.y > 1, grids past 512
    workgroups, the LDS classes at 160 KiB, M inside a tile x every form, outputs inside guards, the bytes around the tensors
"""
import functools

import numpy as np
import pytest

import q6k_ref as QR

pytestmark = pytest.mark.gpu

Q6_K = 14
GEMV_SHAPES = [(m, n, k) for m in (1, 2, 3, 4, 5, 8) for n, k in ((1, 256), (17, 256), (33, 768), (20, 4096))]
# the lanes-per-row forms the list above does not reach, one per M tile; and LDS records above 64 KiB
GEMV_MORE = [(m, n, k) for m in (1, 2, 4, 8) for n, k in ((20, 1024), (9, 1280), (5, 4352))] + [(8, 3, 6912)]
MMQ_SHAPES = [(m, n, k) for m in (9, 16, 17, 33, 64) for n, k in ((1, 512), (15, 256), (17, 768), (70, 1024))]
MMQ_MORE = [(65, 8200, 256)]  # enough 64 x 64 tiles to fill 256 CUs: the 4-row-group form


def all_product_shapes():
    return GEMV_SHAPES + GEMV_MORE + MMQ_SHAPES + MMQ_MORE


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(m, n, k, seed=0):
    """Inputs and the float64 reference of one shape, computed once and shared (never modified)."""
    rng = np.random.default_rng([m, n, k, seed])
    bq, aq = QR.random_q6k(rng, n, k), QR.random_q8_1(rng, m, k)
    return (aq, bq) + QR.gemm(aq, bq)


WORST = {"q6k_gemv": 0.0, "q6k_mmq": 0.0}


def check(qg, aq, bq, ref, fam, algo=0, a=None, b=None):
    """config names `fam` and equals its sumi twin; isum bit-equal; output within tolerance; relaunch identical."""
    c64, isum, mag = ref
    (m, nb), n = aq.shape[:2], bq.shape[0]
    k = 32 * nb
    cfg = qg.debug_config(m, n, k, Q6_K, algo=algo)
    assert cfg.startswith(fam + " "), cfg
    assert cfg == qg.debug_config(m, n, k, Q6_K, algo=algo, sumi=True)
    a = dev(aq) if a is None else a
    b = dev(bq) if b is None else b
    s = host(qg.debug_sumi(a, b, m, n, k, Q6_K, algo))
    assert np.array_equal(s, isum)
    c = host(qg.gemm_w4a8(a, b, m, n, k, Q6_K, algo))
    tol = QR.tol(mag, k, 0 if fam == "q6k_gemv" else 8)
    err = np.abs(c.astype(np.float64) - c64)
    ratio = float((err / tol).max())
    WORST[fam] = max(WORST[fam], ratio)
    print(f"{cfg} M={m} N={n} K={k}: max err/tol = {ratio:.3f}")
    assert (err <= tol).all(), ratio
    c2 = host(qg.gemm_w4a8(a, b, m, n, k, Q6_K, algo))
    assert np.array_equal(c.view(np.uint32), c2.view(np.uint32))
    return c, s


@pytest.mark.parametrize("m,n,k", GEMV_SHAPES + GEMV_MORE)
def test_gemv_shapes(qg, m, n, k):
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "q6k_gemv")


@pytest.mark.parametrize("m,n,k", MMQ_SHAPES + MMQ_MORE)
def test_mmq_shapes(qg, m, n, k):
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "q6k_mmq")


def test_forced_families_at_the_threshold(qg):
    """algo 1 and algo 2 at M = 8 are both served, each within its tolerance, with identical isum."""
    aq, bq, *ref = case(8, 33, 768)
    _, s1 = check(qg, aq, bq, ref, "q6k_gemv", algo=1)
    _, s2 = check(qg, aq, bq, ref, "q6k_mmq", algo=2)
    assert np.array_equal(s1, s2)


@pytest.mark.parametrize("m,n,k", [(3, 33, 768), (17, 17, 768)])
@pytest.mark.parametrize("woff,aoff", [(2, 4), (18, 8), (2, 12), (18, 4)])
def test_pointer_offsets(qg, m, n, k, woff, aoff):
    """Weights 2 and 18 bytes past a 256-B boundary (every super-block's parity flipped), activations at 4 / 8 / 12."""
    aq, bq, *ref = case(m, n, k)
    a, b = QR.dev_at(aq, aoff), QR.dev_at(bq, woff)
    assert b.data_ptr() % 4 == 2 and a.data_ptr() % 16 == aoff
    check(qg, aq, bq, ref, "q6k_gemv" if m <= 8 else "q6k_mmq", a=a, b=b)


@pytest.mark.parametrize("m", [3, 12])
def test_extremes(qg, m):
    """QR.extremes: d at f16 subnormals / the smallest normal / +-65504, scales -128 / 127 / 0, all codes 0 and all 63,
    activations at their f16 ends and qs = -128 (|isum| = 2^24), each class on a weight row of its own."""
    n, k = 16, 512
    aq, bq = QR.extremes(np.random.default_rng([7, m]), m, n, k)
    ref = QR.gemm(aq, bq)
    assert np.abs(ref[1]).max() == 2 ** 24
    c, _ = check(qg, aq, bq, ref, "q6k_gemv" if m <= 8 else "q6k_mmq")
    assert np.isfinite(c).all() and (c[:, 7] == 0).all()


def test_captured_gemvs_stay_plain_nodes(qg):
    """Three Q6_K GEMVs captured on one stream replay to the eager bits, and the capture-time merge never sees them."""
    import torch
    m, n, k = 2, 17, 768
    aq, bq, *_ = case(m, n, k)
    a = dev(aq)
    ws = [dev(np.roll(bq, i, axis=0)) for i in range(3)]
    eager = [host(qg.gemm_w4a8(a, w, m, n, k, Q6_K)) for w in ws]
    outs = [torch.zeros((m, n), dtype=torch.float32, device="cuda") for _ in ws]
    torch.cuda.synchronize()
    s0 = qg.capture_fusion_stats()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for w, o in zip(ws, outs):
            qg.gemm_w4a8(a, w, m, n, k, Q6_K, out=o)
    assert qg.capture_fusion_stats() == s0
    g.replay()
    torch.cuda.synchronize()
    assert qg.capture_fusion_stats() == s0
    for e, o in zip(eager, outs):
        assert np.array_equal(e.view(np.uint32), host(o).view(np.uint32))


def test_dequantize_bit_exact(qg):
    """All 64 codes x scales {-128, -1, 0, 1, 127} (and random d), then random blocks."""
    rng = np.random.default_rng(11)
    scs = np.array([-128, -1, 0, 1, 127])
    q = np.tile(np.repeat(np.arange(64) - 32, 4), (5, 1))            # [5, 256]: each code 4 times
    q = np.stack([np.roll(q, 16 * i, axis=1) for i in range(4)], 1)  # every code in every nibble / bit-pair position
    sc = np.broadcast_to(scs[:, None, None], (5, 4, 16))
    b = QR.build(rng.uniform(-0.01, 0.01, (5, 4)), sc, q)
    b = np.concatenate([b, QR.random_q6k(rng, 3, 1024)])
    y = host(qg.dequantize(dev(b), Q6_K))
    assert y.shape == (8, 1024)
    assert np.array_equal(y.view(np.uint32), QR.dequant(b).view(np.uint32))


@pytest.mark.parametrize("m", [2, 12])
def test_f32_activations_through_workspace(qg, m):
    n, k = 33, 512
    rng = np.random.default_rng(13)
    x = dev(rng.uniform(-1, 1, (m, k)).astype(np.float32))
    b = dev(QR.random_q6k(rng, n, k))
    fused = host(qg.gemm_w4a8_f32(x, b, Q6_K))
    two = host(qg.gemm_w4a8(qg.quantize_q8_1(x), b, m, n, k, Q6_K))
    assert np.array_equal(fused.view(np.uint32), two.view(np.uint32))
    with pytest.raises(RuntimeError):
        qg.gemm_w4a8_f32(x, b, Q6_K, workspace=False)


def test_from_ggml_view(qg):
    import torch
    from quant_gemm import ggml as G
    m, n, k = 2, 17, 768
    aq, bq, *_ = case(m, n, k)
    a, w = dev(aq), dev(bq)
    out = torch.empty((m, n), dtype=torch.float32, device="cuda")
    wv = G.view_of(w, G.Q6_K, k)
    assert list(wv.nb[:2]) == [210, 630] and list(wv.ne[:2]) == [k, n]
    G.gemm_w4a8_from_ggml(G.view_of(a, G.Q8_1, k), wv, G.view_of(out, G.F32, n))
    direct = host(qg.gemm_w4a8(a, w, m, n, k, Q6_K))
    assert np.array_equal(host(out).view(np.uint32), direct.view(np.uint32))


def test_nmse_against_fp32(qg):
    """U[-1, 1] inputs, weights through the test-side min/max quantizer: NMSE against the float64 product under the
    project's 5e-3 bar."""
    m, n, k = 4, 64, 1024
    rng = np.random.default_rng(0)
    a = rng.uniform(-1, 1, (m, k)).astype(np.float32)
    w = rng.uniform(-1, 1, (n, k)).astype(np.float32)
    bq = QR.quantize(w)
    aq = qg.quantize_q8_1(dev(a))
    c = host(qg.gemm_w4a8(aq, dev(bq), m, n, k, Q6_K)).astype(np.float64)
    ref = a.astype(np.float64) @ w.astype(np.float64).T
    nmse = ((c - ref) ** 2).sum() / (ref ** 2).sum()
    print(f"Q6_K NMSE vs FP32 = {nmse:.3e}")
    assert nmse <= 5e-3, nmse


def test_seeded_sweep(qg):
    """16 seeded cases (QR.fuzz_cases): M from the product sweep's list, N in 1..200, K = 256 * (1..12), weights 2 / 18
    and activations 4 / 8 / 12 bytes past a 256-B boundary. None is skipped; the largest error / bound ratio is printed."""
    worst = 0.0
    for i, m, n, k, woff, aoff in QR.fuzz_cases():
        aq, bq, *ref = case(m, n, k, seed=1000 + i)
        fam = "q6k_gemv" if m <= 8 else "q6k_mmq"
        before = WORST[fam]
        WORST[fam] = 0.0
        check(qg, aq, bq, ref, fam, a=QR.dev_at(aq, aoff), b=QR.dev_at(bq, woff))
        worst = max(worst, WORST[fam])
        WORST[fam] = max(before, WORST[fam])
    print(f"Q6_K sweep: largest err/tol = {worst:.3f}; whole module so far: {WORST}")
    assert worst <= 1.0
