"""Q3_K x Q8_1 on the GPU against the NumPy contract (tests/q3k_ref.py): isum (qg_debug_sumi) bit-equal, every output
within 2 (K/32 + W + 2) 2^-24 mag (W = 0 for q3k_gemv, QR.MMQ_W = 7 for q3k_mmq), relaunch bit-identical.
K = 256 .. 4352 are the six (LPR, ONE) forms of the GEMV, M = 1, 2, 3, 5, 8 its MT = 1, 2, 4, 8 (QG_ALGO_AUTO sends it
M <= 6, so its cases at M = 8 force it); N = 67 leaves partial row tiles. K = 768 is fewer super-blocks than K slices;
K = 2304 (odd K/256) alternates the rows' address parity."""
import functools

import numpy as np
import pytest

import q3k_ref as QR

pytestmark = pytest.mark.gpu

T = QR.Q3_K
GEMV_SHAPES = [(m, n, k) for m in (1, 2, 3, 5, 8) for n in (1, 67) for k in (256, 512, 1024, 2304, 4096, 4352)]
MMQ_SHAPES = [(m, n, k) for m in (9, 17, 33, 65) for n in (1, 17, 200) for k in (256, 768, 2304)]


def family(m, algo=0):
    return "q3k_mmq" if algo == 2 or (m > 6 and algo == 0) else "q3k_gemv"


@functools.lru_cache(maxsize=None)
def case(m, n, k):
    """Inputs and the float64 reference of one shape, computed once and shared (never modified)."""
    rng = np.random.default_rng([m, n, k])
    bq, aq = QR.random_q3k(rng, n, k), QR.random_q8_1(rng, m, k)
    return (aq, bq) + QR.gemm(aq, bq)


def check(qg, aq, bq, ref, fam, algo=0, woff=0, fill=0):
    """config names `fam` and equals its sumi twin; isum bit-equal; output within tolerance; relaunch identical. The
    weights start woff bytes past a 256-B boundary, in a buffer otherwise full of `fill`."""
    c64, isum, mag = ref
    (m, nb), n = aq.shape[:2], bq.shape[0]
    k = 32 * nb
    cfg = qg.debug_config(m, n, k, T, algo=algo)
    assert cfg.startswith(fam + " ") and cfg == qg.debug_config(m, n, k, T, algo=algo, sumi=True), cfg
    a, b = QR.dev_at(aq, 0), QR.dev_at(bq, woff, fill=fill)
    assert b.data_ptr() % 256 == woff
    s = qg.debug_sumi(a, b, m, n, k, T, algo).cpu().numpy()
    assert np.array_equal(s, isum)
    c = qg.gemm_w4a8(a, b, m, n, k, T, algo).cpu().numpy()
    tol = QR.tol(mag, k, 0 if fam == "q3k_gemv" else QR.MMQ_W)
    err = np.abs(c.astype(np.float64) - c64)
    print(f"{cfg} M={m} N={n} K={k} woff={woff}: max err/tol = {(err / np.maximum(tol, 1e-300)).max():.3f}")
    assert (err <= tol).all(), (err / tol).max()
    assert np.array_equal(c.view(np.uint32), qg.gemm_w4a8(a, b, m, n, k, T, algo).cpu().numpy().view(np.uint32))
    return c, s


def test_shapes_reach_every_form(qg):
    cfgs = [qg.debug_config(m, n, k, T, algo=int(m > 6)).split() for m, n, k in GEMV_SHAPES]  # forced beyond AUTO's 6
    seen = {" ".join(c[:5:2] + c[1:2]) for c in cfgs}
    want = {f"q3k_gemv LPR={lpr} ONE={one} MT={mt}" for mt in (1, 2, 4, 8) for lpr in (4, 16, 64) for one in (1, 0)}
    assert len(want) == 24 and want == seen, sorted(want ^ seen)
    assert qg.debug_config(1, 67, 256, T).split()[5] == "grid=2"
    assert qg.debug_config(6, 67, 256, T).startswith("q3k_gemv ") and qg.debug_config(7, 67, 256, T).startswith("q3k_mmq ")
    mmq = {" ".join(qg.debug_config(m, n, k, T).split()[:3]) for m, n, k in MMQ_SHAPES}
    assert mmq == {f"q3k_mmq TT={tt} RG=1" for tt in (1, 2, 4)}, mmq


@pytest.mark.parametrize("m,n,k", GEMV_SHAPES + MMQ_SHAPES)
def test_shapes(qg, m, n, k):
    aq, bq, *ref = case(m, n, k)
    algo = int(6 < m <= 8)  # the GEMV cases beyond AUTO's threshold are forced
    check(qg, aq, bq, ref, family(m, algo), algo=algo, woff=2 * ((m + n + k // 256) % 2))


def test_mmq_64x64_tile_form(qg):
    """The 4-row-group form at M = 65, K = 256 and the smallest N that selects it on this device: as many 64-row
    columns as, with two tile rows of tokens, fill the CUs; one row fewer stays in the 16-row form."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m, k = 65, 256
    n = 64 * (-(-cus // 2) - 1) + 1
    assert " RG=4 KS=2 " in qg.debug_config(m, n, k, T) and " RG=1 " in qg.debug_config(m, n - 1, k, T)
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "q3k_mmq", woff=2)


@pytest.mark.parametrize("woff", [0, 2])
@pytest.mark.parametrize("m,algo", [(3, 0), (17, 0), (1, 2), (8, 1), (8, 2)])
def test_both_weight_alignments(qg, m, algo, woff):
    """Weights 0 and 2 bytes past a 256-B boundary (a row of 9 super-blocks also alternates its rows), for both
    families, the forced MFMA kernel at M = 1 and both forced families at M = 8."""
    aq, bq, *ref = case(m, 67, 2304)
    _, s = check(qg, aq, bq, ref, family(m, algo), algo=algo, woff=woff)
    if m == 8:  # the two forced families at M = 8 agree on isum
        assert np.array_equal(s, check(qg, aq, bq, ref, family(m, 3 - algo), algo=3 - algo, woff=woff)[1])


@pytest.mark.parametrize("woff", [0, 2])
@pytest.mark.parametrize("m", [1, 9])
def test_bytes_outside_the_tensor_do_not_matter(qg, m, woff):
    """The smallest shape of each family in a buffer of 0x00 and of 0xFF: the dwords that straddle the tensor's ends
    are loaded, and what they hold outside it must not reach the result."""
    aq, bq, *ref = case(m, 1, 256)
    c0, _ = check(qg, aq, bq, ref, family(m), woff=woff, fill=0x00)
    c1, _ = check(qg, aq, bq, ref, family(m), woff=woff, fill=0xFF)
    assert np.array_equal(c0.view(np.uint32), c1.view(np.uint32))


@pytest.mark.parametrize("algo", [1, 2])
def test_extremes(qg, algo):
    """QR.extremes through both families: d subnormal, +-65504, zero and negative; sc = 0, 32, 63; the row whose isum is
    -2^19 with the pre-scaled operand byte at -128; sc = 63 with q = -4; sc = 0 with q = 3."""
    aq, bq = QR.extremes(np.random.default_rng(8), 4)
    c, s = check(qg, aq, bq, QR.gemm(aq, bq), family(4, algo), algo=algo, woff=2)
    assert (s[0, QR.MAX_ROW] == -2 ** 19).all()
    assert np.isfinite(c).all() and (c[:, QR.D0_ROW] == 0).all() and (c[:, QR.SC32_ROW] == 0).all()


def test_dequantize_bit_exact(qg):
    """All 8 codes x sc in {0, 1, 31, 32, 33, 63}, d of both signs, at 2 B past a 256-B boundary."""
    sc = np.array([0, 1, 31, 32, 33, 63, 0, 63, 1, 33, 31, 32, 63, 0, 32, 1])
    q = (np.arange(32)[None, None] + np.arange(8)[None, :, None] + np.arange(4)[:, None, None]) % 8 - 4
    b = QR.build(np.array([0.0123, -3.5, 65504.0, -2.0 ** -24]), np.stack([np.roll(sc, i) for i in range(4)]), q)
    y = qg.dequantize(QR.dev_at(b, 2), T).cpu().numpy().reshape(-1)
    assert np.array_equal(y.view(np.uint32), QR.dequantize(b).reshape(-1).view(np.uint32))


@pytest.mark.parametrize("k", [256, 4352])
@pytest.mark.parametrize("a_rows", [1, 2])
def test_moe_slots_have_the_eager_bits(qg, k, a_rows):
    """Every slot has the bits of the eager M = 1 product on its row and expert; an id out of range gives zeros."""
    import torch
    t, u, ne, n = 3, 2, 4, 67
    rng = np.random.default_rng([k, a_rows])
    experts = QR.random_q3k(rng, ne * n, k).reshape(ne, n, k // 256, 110)
    aq = QR.random_q8_1(rng, t * a_rows, k).reshape(t, a_rows, k // 32, 36)
    ids = np.array([[0, 3], [4, 2], [1, 1]], np.int32)
    assert qg.moe_config(t, u, n, k, T).startswith("moe:q3k_gemv ")
    a, w = QR.dev_at(aq, 0), QR.dev_at(experts, 2)
    c = qg.gemm_w4a8_moe(a, w, torch.from_numpy(ids).cuda(), t, u, n, k, T, a_rows=a_rows).cpu().numpy()
    for ti in range(t):
        for ui in range(u):
            e = int(ids[ti, ui])
            want = qg.gemm_w4a8(a[ti, ui % a_rows][None], w[e], 1, n, k, T).cpu().numpy()[0] if e < ne else np.zeros(n, np.float32)
            assert np.array_equal(c[ti, ui].view(np.uint32), want.view(np.uint32)), (ti, ui)
