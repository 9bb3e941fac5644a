"""MXFP4 x Q8_1 on the GPU: the decode GEMV (mxfp4_gemv, M <= 8) and the MFMA prefill (mxfp4_mmq, M >= 9) against the
NumPy contract (tests/mxfp4_ref.py).

sumi (qg_debug_sumi) must be bit-equal; every fp32 output must satisfy |c - C64| <= 2 (K/32 + W + 2) 2^-24 mag with
W = 0 for mxfp4_gemv and W = MR.MMQ_W = 8 for mxfp4_mmq (MR.tol); two launches must give identical bits.

Shapes and what they reach (qg.debug_config, asserted in test_gemv_shapes_reach_every_form):
  mxfp4_gemv MT = 1, 2, 4, 8 with LPR=4 ONE=1 (K = 32, 96), LPR=16 ONE=1 (K = 512), LPR=64 ONE=0 (K = 2880, 2912, 4096,
    8192), and LPR=4 / 16 ONE=0 and LPR=64 ONE=1 from GEMV_MORE (K = 160, 1504, 2048). K = 96 (51-B rows) and K = 2912
    (1547-B rows) put consecutive rows at all four byte offsets in a dword; every case also starts its weights 0..3
    bytes past a 256-B boundary. N = 1 and 67 leave partial row tiles, N = 200 takes more than one workgroup.
  mxfp4_mmq TT=1 (M = 9, 16) TT=2 (17) TT=4 (33, 65, 130), RG=1; RG=4 at M = 65 and the smallest N that fills the CUs;
    K = 32 and 96 are one partial group of blocks, K = 2912 is 11 whole groups and one of 3 blocks over the 8 K slices.
"""
import functools

import numpy as np
import pytest

import mxfp4_ref as MR

pytestmark = pytest.mark.gpu

MXFP4 = 39
GEMV_K = (32, 96, 512, 2880, 2912, 4096, 8192)
GEMV_SHAPES = [(m, n, k) for m in range(1, 9) for n in (1, 67, 200) for k in GEMV_K]
GEMV_MORE = [(m, 67, k) for m in (1, 2, 4, 8) for k in (160, 1504, 2048)]  # LPR=4 loop, LPR=16 loop, LPR=64 one unit
MMQ_SHAPES = [(m, n, k) for m in (9, 16, 17, 33, 65, 130) for n in (1, 17, 200) for k in (32, 96, 2912)]


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
    bq, aq = MR.random_mxfp4(rng, n, k), MR.random_q8_1(rng, m, k)
    return (aq, bq) + MR.gemm(aq, bq)


WORST = {"mxfp4_gemv": 0.0, "mxfp4_mmq": 0.0}


def check(qg, aq, bq, ref, fam, algo=0, woff=0, aoff=0, bound=None):
    """config names `fam` and equals its sumi twin; sumi bit-equal; output within tolerance; relaunch identical. The
    weights start woff bytes past a 256-B boundary, the activations aoff."""
    c64, sumi, mag = ref
    (m, nb), n = aq.shape[:2], bq.shape[0]
    k = 32 * nb
    cfg = qg.debug_config(m, n, k, MXFP4, algo=algo)
    assert cfg.startswith(fam + " "), cfg
    assert cfg == qg.debug_config(m, n, k, MXFP4, algo=algo, sumi=True)
    a, b = MR.dev_at(aq, aoff), MR.dev_at(bq, woff)
    assert b.data_ptr() % 4 == woff % 4 and a.data_ptr() % 16 == aoff
    s = host(qg.debug_sumi(a, b, m, n, k, MXFP4, algo))
    assert np.array_equal(s, sumi)
    c = host(qg.gemm_w4a8(a, b, m, n, k, MXFP4, algo))
    tol = MR.tol(mag, k, 0 if fam == "mxfp4_gemv" else MR.MMQ_W) if bound is None else bound
    err = np.abs(c.astype(np.float64) - c64)
    ratio = float((err[tol > 0] / tol[tol > 0]).max())  # (a floor-free bound is 0 where every term is)
    WORST[fam] = max(WORST[fam], ratio)
    print(f"{cfg} M={m} N={n} K={k} woff={woff}: max err/tol = {ratio:.3f}")
    assert (err <= tol).all(), ratio
    c2 = host(qg.gemm_w4a8(a, b, m, n, k, MXFP4, algo))
    assert np.array_equal(c.view(np.uint32), c2.view(np.uint32))
    return c, s


def test_gemv_shapes_reach_every_form(qg):
    seen = set()
    for m, n, k in GEMV_SHAPES + GEMV_MORE:
        cfg = qg.debug_config(m, n, k, MXFP4)
        seen.add(" ".join(w for w in cfg.split() if w.split("=")[0] in ("mxfp4_gemv", "MT", "LPR", "ONE")))
    want = {f"mxfp4_gemv MT={mt} LPR={lpr} ONE={one}" for mt in (1, 2, 4, 8) for lpr in (4, 16, 64) for one in (1, 0)}
    assert len(want) == 24 and want <= seen, sorted(want - seen)
    assert any(qg.debug_config(m, 200, k, MXFP4).split()[5] != "grid=1" for m, _, k in GEMV_SHAPES)
    mmq = {" ".join(qg.debug_config(m, n, k, MXFP4).split()[:3]) for m, n, k in MMQ_SHAPES}
    assert mmq == {f"mxfp4_mmq TT={tt} RG=1" for tt in (1, 2, 4)}, mmq


@pytest.mark.parametrize("m,n,k", GEMV_SHAPES + GEMV_MORE)
def test_gemv_shapes(qg, m, n, k):
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "mxfp4_gemv", woff=(m + n + k // 32) % 4)


@pytest.mark.parametrize("m,n,k", MMQ_SHAPES)
def test_mmq_shapes(qg, m, n, k):
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "mxfp4_mmq", woff=(m + n + k // 32) % 4)


@pytest.mark.parametrize("woff", [0, 1, 2, 3])
@pytest.mark.parametrize("m,n,k,algo", [(1, 67, 2912, 0), (5, 67, 2912, 0), (8, 5, 96, 0), (17, 67, 2912, 0), (9, 5, 96, 0),
                                        (1, 67, 2912, 2), (8, 67, 2912, 1)])
def test_every_weight_offset(qg, m, n, k, algo, woff):
    """Weights 0, 1, 2 and 3 bytes past a 256-B boundary, for both families, the forced MFMA kernel at M = 1 and the
    forced GEMV at M = 8; rows of 1547 and 51 bytes put the rows themselves at every offset too."""
    aq, bq, *ref = case(m, n, k)
    fam = "mxfp4_mmq" if algo == 2 or (algo == 0 and m > 8) else "mxfp4_gemv"
    check(qg, aq, bq, ref, fam, algo=algo, woff=woff, aoff=4 * (woff & 1))


def test_forced_families_at_the_threshold(qg):
    """algo 1 and algo 2 at M = 8 are both served, each within its tolerance, with identical sumi."""
    aq, bq, *ref = case(8, 67, 2912)
    _, s1 = check(qg, aq, bq, ref, "mxfp4_gemv", algo=1, woff=3)
    _, s2 = check(qg, aq, bq, ref, "mxfp4_mmq", algo=2, woff=3)
    assert np.array_equal(s1, s2)


def test_mmq_64_512_4096(qg):
    aq, bq, *ref = case(64, 512, 4096)
    assert qg.debug_config(64, 512, 4096, MXFP4).startswith("mxfp4_mmq TT=4 RG=1 KS=8 ")
    check(qg, aq, bq, ref, "mxfp4_mmq", woff=1)


def test_mmq_64x64_tile_form(qg):
    """The 4-row-group form at the smallest M and N that select it on this device: two tile rows of tokens (M = 65) and
    as many 64-row columns as fill the CUs; one column fewer stays in the 16-row form."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m, k = 65, 96
    cols = -(-cus // 2)
    n = 64 * (cols - 1) + 1
    assert " RG=4 KS=2 " in qg.debug_config(m, n, k, MXFP4) and " RG=1 " in qg.debug_config(m, n - 1, k, MXFP4)
    assert " RG=1 " in qg.debug_config(64, n, k, MXFP4)
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "mxfp4_mmq", woff=3)


def test_ldc_leaves_the_gap_untouched(qg):
    import torch
    for m, n, k in ((3, 67, 2912), (17, 67, 96)):
        aq, bq, c64, _, mag = case(m, n, k)
        wide = torch.full((m, n + 13), -7.5, dtype=torch.float32, device="cuda")
        qg.gemm_w4a8(dev(aq), MR.dev_at(bq, 1), m, n, k, MXFP4, out=wide[:, :n])
        w = host(wide)
        assert (w[:, n:] == -7.5).all()
        dense = host(qg.gemm_w4a8(dev(aq), MR.dev_at(bq, 1), m, n, k, MXFP4))
        assert np.array_equal(w[:, :n].view(np.uint32), dense.view(np.uint32))


def test_dequantize_bit_exact(qg):
    """16 codes x 256 exponents: 256 blocks, block i with e = i and every code twice (rotated by i, so each code sits in
    both nibbles), at an odd address. Exact, subnormals kept, +0.0f for code 8."""
    e = np.arange(256)
    code = (np.arange(32)[None] + e[:, None]) % 16
    b = MR.build(e, code)
    y = host(qg.dequantize(MR.dev_at(b, 1), MXFP4)).reshape(256, 32)
    with np.errstate(over="ignore"):
        want = MR.dequantize(b).reshape(256, 32)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
    assert (y.view(np.uint32)[code == 8] == 0).all()
    exact = MR.KV[code] * 2.0 ** (e[:, None] - 128.0)
    fits = np.abs(exact) < 2.0 ** 128
    assert (y.astype(np.float64)[fits] == exact[fits]).all()


@pytest.mark.parametrize("algo", [1, 2])
def test_extremes(qg, algo):
    """MR.extremes: e in {0, 1, 2, 3, 126..129} and up to 200, rows of all-zero codes, all code 8, all +12, all -12,
    against d_a at f16 subnormals, the smallest normal, 1.0 (with a block of -128: |sumi| = 49152) and 65504. Within
    MR.tol, and within the contract's own statement (2^-149 per subnormal term, no floor); no Inf, no NaN."""
    n, k = 16, 512
    aq, bq = MR.extremes(np.random.default_rng(8), n, k)
    ref = MR.gemm(aq, bq)
    assert ref[2].max() < 2.0 ** 127
    fam = "mxfp4_gemv" if algo == 1 else "mxfp4_mmq"
    c, _ = check(qg, aq, bq, ref, fam, algo=algo, woff=algo)
    assert np.isfinite(c).all() and (c[:, 8] == 0).all() and (c[:, 9] == 0).all()
    check(qg, aq, bq, ref, fam, algo=algo, woff=3, bound=MR.contract_bound(aq, bq, 0 if algo == 1 else MR.MMQ_W))


@pytest.mark.parametrize("algo", [1, 2])
def test_extremes_where_the_scale_product_is_no_fp32_number(qg, algo):
    """Subnormal d_a such as 3 * 2^-24 against e <= 2: d_a * scale(e) is rounded before it meets sumi (the contract's
    order), which costs up to 2^-150 |sumi| per term; MR.lossy_scale_slack, from the formats alone. fp32 subnormals are
    kept: were they flushed, the outputs of rows 0 and 1 would be zero."""
    n, k = 16, 512
    aq, bq = MR.extremes(np.random.default_rng(8), n, k, lossy=True)
    ref = MR.gemm(aq, bq)
    fam = "mxfp4_gemv" if algo == 1 else "mxfp4_mmq"
    bound = MR.contract_bound(aq, bq, 0 if algo == 1 else MR.MMQ_W) + MR.lossy_scale_slack(aq, bq)
    c, _ = check(qg, aq, bq, ref, fam, algo=algo, woff=2, bound=bound)
    assert np.isfinite(c).all() and (c[1:3, :2] != 0).all()


def test_nmse_against_fp32(qg):
    """Gaussian weights through the test-side quantizer: the product against the FP32 product of the dequantized weights
    and the FP32 activations under the project's 5e-3 bar, and against the float64 contract within tol."""
    rng = np.random.default_rng(0)
    k, n = 2880, 64
    w = rng.standard_normal((n, k)).astype(np.float32) * 0.05
    bq = MR.quantize(w)
    wd = MR.dequantize(bq).astype(np.float64)
    for m in (4, 12):
        a = rng.standard_normal((m, k)).astype(np.float32)
        aq_t = qg.quantize_q8_1(dev(a))
        aq = host(aq_t)
        c = host(qg.gemm_w4a8(aq_t, MR.dev_at(bq, 1), m, n, k, MXFP4)).astype(np.float64)
        ref = a.astype(np.float64) @ wd.T
        nmse = ((c - ref) ** 2).sum() / (ref ** 2).sum()
        print(f"MXFP4 M={m} NMSE vs FP32 on the dequantized weights = {nmse:.3e}")
        assert nmse <= 5e-3, nmse
        c64, _, mag = MR.gemm(aq, bq)
        assert (np.abs(c - c64) <= MR.tol(mag, k, 0 if m <= 8 else MR.MMQ_W)).all()


def test_seeded_sweep(qg):
    """The 16 seeded cases of MR.fuzz_cases. None is skipped; the largest error / bound ratio is printed."""
    worst = 0.0
    for i, m, n, k, woff, aoff in MR.fuzz_cases():
        aq, bq, *ref = case(m, n, k, seed=1000 + i)
        fam = "mxfp4_gemv" if m <= 8 else "mxfp4_mmq"
        before = WORST[fam]
        WORST[fam] = 0.0
        check(qg, aq, bq, ref, fam, woff=woff, aoff=aoff)
        worst = max(worst, WORST[fam])
        WORST[fam] = max(before, WORST[fam])
    print(f"MXFP4 sweep: largest err/tol = {worst:.3f}; whole module so far: {WORST}")
    assert worst <= 1.0


def test_captured_gemvs_stay_plain_nodes(qg):
    """Two consecutive MXFP4 GEMVs captured on one stream are two kernel nodes (the capture-time merge, which would make
    one grouped node of them, never sees them: its counters do not move) and replay to the eager bits."""
    import torch
    m, n, k = 2, 67, 2912
    aq, bq, *_ = case(m, n, k)
    a = dev(aq)
    ws = [MR.dev_at(np.roll(bq, i, axis=0), 1 + i) for i in range(2)]
    eager = [host(qg.gemm_w4a8(a, w, m, n, k, MXFP4)) for w in ws]
    outs = [torch.zeros((m, n), dtype=torch.float32, device="cuda") for _ in ws]
    torch.cuda.synchronize()
    s0 = qg.capture_fusion_stats()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for w, o in zip(ws, outs):
            qg.gemm_w4a8(a, w, m, n, k, MXFP4, out=o)
    assert qg.capture_fusion_stats() == s0
    g.replay()
    torch.cuda.synchronize()
    assert qg.capture_fusion_stats() == s0
    for e, o in zip(eager, outs):
        assert np.array_equal(e.view(np.uint32), host(o).view(np.uint32))


def test_from_ggml_view(qg):
    import torch
    from quant_gemm import ggml as G
    for m, n, k in ((2, 67, 2912), (17, 17, 96)):
        aq, bq, *_ = case(m, n, k)
        a, w = dev(aq), MR.dev_at(bq, 3)
        out = torch.empty((m, n), dtype=torch.float32, device="cuda")
        wv = G.view_of(w, G.MXFP4, k)
        assert list(wv.nb[:2]) == [17, k // 32 * 17] and list(wv.ne[:2]) == [k, n]
        G.gemm_w4a8_from_ggml(G.view_of(a, G.Q8_1, k), wv, G.view_of(out, G.F32, n))
        direct = host(qg.gemm_w4a8(a, w, m, n, k, MXFP4))
        assert np.array_equal(host(out).view(np.uint32), direct.view(np.uint32))


@pytest.mark.parametrize("m", [2, 12])
def test_f32_activations_through_workspace(qg, m):
    n, k = 33, 2912
    rng = np.random.default_rng(13)
    x = dev(rng.uniform(-1, 1, (m, k)).astype(np.float32))
    b = MR.dev_at(MR.random_mxfp4(rng, n, k), 1)
    fused = host(qg.gemm_w4a8_f32(x, b, MXFP4))
    two = host(qg.gemm_w4a8(qg.quantize_q8_1(x), b, m, n, k, MXFP4))
    assert np.array_equal(fused.view(np.uint32), two.view(np.uint32))
    with pytest.raises(RuntimeError):
        qg.gemm_w4a8_f32(x, b, MXFP4, workspace=False)
