"""IQ4_XS x Q8_1 on the GPU against the NumPy contract (tests/iq4xs_ref.py): sumi (qg_debug_sumi) bit-equal, every
output within 2 (K/32 + W + 2) 2^-24 mag (W = 0 for iq4xs_gemv, IR.MMQ_W = 8 for iq4xs_mmq), relaunch bit-identical.
K = 256 .. 4352 are the six (LPR, ONE) forms of the GEMV, M = 1, 2, 3, 5, 8 its MT = 1, 2, 4, 8; N = 67 leaves partial
row tiles and takes two workgroups at LPR = 4. K = 768 is fewer super-blocks than K slices."""
import functools

import numpy as np
import pytest

import iq4xs_ref as IR

pytestmark = pytest.mark.gpu

T = IR.IQ4_XS
GEMV_SHAPES = [(m, n, k) for m in (1, 2, 3, 5, 8) for n in (1, 67) for k in (256, 512, 1024, 2304, 4096, 4352)]
MMQ_SHAPES = [(m, n, k) for m in (9, 17, 33, 65) for n in (1, 17, 200) for k in (256, 768, 2304)]


def dev(x):
    return IR.dev_at(x, 0)


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(m, n, k):
    """Inputs and the float64 reference of one shape, computed once and shared (never modified)."""
    rng = np.random.default_rng([m, n, k])
    bq, aq = IR.random_iq4xs(rng, n, k), IR.random_q8_1(rng, m, k)
    return (aq, bq) + IR.gemm(aq, bq)


def check(qg, aq, bq, ref, fam, algo=0, woff=0):
    """config names `fam` and equals its sumi twin; sumi bit-equal; output within tolerance; relaunch identical. The
    weights start woff bytes past a 256-B boundary."""
    c64, sumi, mag = ref
    (m, nb), n = aq.shape[:2], bq.shape[0]
    k = 32 * nb
    cfg = qg.debug_config(m, n, k, T, algo=algo)
    assert cfg.startswith(fam + " ") and cfg == qg.debug_config(m, n, k, T, algo=algo, sumi=True), cfg
    a, b = dev(aq), IR.dev_at(bq, woff)
    assert b.data_ptr() % 256 == woff
    s = host(qg.debug_sumi(a, b, m, n, k, T, algo))
    assert np.array_equal(s, sumi)
    c = host(qg.gemm_w4a8(a, b, m, n, k, T, algo))
    tol = IR.tol(mag, k, 0 if fam == "iq4xs_gemv" else IR.MMQ_W)
    err = np.abs(c.astype(np.float64) - c64)
    print(f"{cfg} M={m} N={n} K={k} woff={woff}: max err/tol = {(err / tol).max():.3f}")
    assert (err <= tol).all(), (err / tol).max()
    assert np.array_equal(c.view(np.uint32), host(qg.gemm_w4a8(a, b, m, n, k, T, algo)).view(np.uint32))
    return c, s


def test_shapes_reach_every_form(qg):
    seen = {" ".join(qg.debug_config(m, n, k, T).split()[:5:2] + qg.debug_config(m, n, k, T).split()[1:2])
            for m, n, k in GEMV_SHAPES}
    want = {f"iq4xs_gemv LPR={lpr} ONE={one} MT={mt}" for mt in (1, 2, 4, 8) for lpr in (4, 16, 64) for one in (1, 0)}
    assert len(want) == 24 and want == seen, sorted(want ^ seen)
    assert qg.debug_config(1, 67, 256, T).split()[5] == "grid=2"
    mmq = {" ".join(qg.debug_config(m, n, k, T).split()[:3]) for m, n, k in MMQ_SHAPES}
    assert mmq == {f"iq4xs_mmq TT={tt} RG=1" for tt in (1, 2, 4)}, mmq


@pytest.mark.parametrize("m,n,k", GEMV_SHAPES)
def test_gemv_shapes(qg, m, n, k):
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "iq4xs_gemv", woff=8 * ((m + n + k // 256) % 2))


@pytest.mark.parametrize("m,n,k", MMQ_SHAPES)
def test_mmq_shapes(qg, m, n, k):
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "iq4xs_mmq", woff=8 * ((m + n + k // 256) % 2))


def test_mmq_64x64_tile_form(qg):
    """The 4-row-group form at M = 65, K = 256 and the smallest N that selects it on this device: as many 64-row
    columns as, with two tile rows of tokens, fill the CUs; one row fewer stays in the 16-row form."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m, k = 65, 256
    n = 64 * (-(-cus // 2) - 1) + 1
    assert " RG=4 KS=2 " in qg.debug_config(m, n, k, T) and " RG=1 " in qg.debug_config(m, n - 1, k, T)
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "iq4xs_mmq", woff=8)


@pytest.mark.parametrize("woff", [0, 8])
@pytest.mark.parametrize("m,algo", [(3, 0), (17, 0), (1, 2), (8, 1), (8, 2)])
def test_both_weight_alignments(qg, m, algo, woff):
    """Weights 0 and 8 bytes past a 256-B boundary (a row of 9 super-blocks also alternates its rows), for both
    families, the forced MFMA kernel at M = 1 and both forced families at M = 8."""
    aq, bq, *ref = case(m, 67, 2304)
    _, s = check(qg, aq, bq, ref, "iq4xs_mmq" if algo == 2 or m > 8 else "iq4xs_gemv", algo=algo, woff=woff)
    if m == 8:  # the two forced families at M = 8 agree on sumi
        assert np.array_equal(s, check(qg, aq, bq, ref, "iq4xs_gemv" if algo == 2 else "iq4xs_mmq", algo=3 - algo)[1])


@pytest.mark.parametrize("algo", [1, 2])
def test_extremes(qg, algo):
    """IR.extremes through both families: d subnormal, +-65504, zero and negative; ls = 0, 32, 63; the row whose int32
    product is the contract's maximum 16646144."""
    aq, bq = IR.extremes(np.random.default_rng(8), 4)
    c, _ = check(qg, aq, bq, IR.gemm(aq, bq), "iq4xs_gemv" if algo == 1 else "iq4xs_mmq", algo=algo, woff=8)
    assert np.isfinite(c).all() and (c[:, 5] == 0).all() and (c[:, 8] == 0).all()


def test_dequantize_bit_exact(qg):
    """All 16 codes (in both nibbles) x ls in {0, 1, 31, 32, 33, 63}, d of both signs, at 8 B past a 256-B boundary."""
    ls = np.array([0, 1, 31, 32, 33, 63, 0, 63])
    code = (np.arange(32)[None, None] + np.arange(8)[None, :, None] + np.arange(4)[:, None, None]) % 16
    b = IR.build(np.array([0.0123, -3.5, 65504.0, 2.0 ** -24]), np.stack([np.roll(ls, i) for i in range(4)]), code)
    y = host(qg.dequantize(IR.dev_at(b, 8), T)).reshape(-1)
    assert np.array_equal(y.view(np.uint32), IR.dequantize(b).reshape(-1).view(np.uint32))


@pytest.mark.parametrize("k", [256, 4352])
@pytest.mark.parametrize("a_rows", [1, 2])
def test_moe_slots_have_the_eager_bits(qg, k, a_rows):
    """Every slot has the bits of the eager M = 1 product on its row and expert; an id out of range gives zeros."""
    import torch
    t, u, ne, n = 3, 2, 4, 67
    rng = np.random.default_rng([k, a_rows])
    experts = IR.random_iq4xs(rng, ne * n, k).reshape(ne, n, k // 256, 136)
    aq = IR.random_q8_1(rng, t * a_rows, k).reshape(t, a_rows, k // 32, 36)
    ids = np.array([[0, 3], [4, 2], [1, 1]], np.int32)
    assert qg.moe_config(t, u, n, k, T).startswith("moe:iq4xs_gemv ")
    a, w = dev(aq), IR.dev_at(experts, 8)
    c = host(qg.gemm_w4a8_moe(a, w, torch.from_numpy(ids).cuda(), t, u, n, k, T, a_rows=a_rows))
    for ti in range(t):
        for ui in range(u):
            e = int(ids[ti, ui])
            want = host(qg.gemm_w4a8(a[ti, ui % a_rows][None], w[e], 1, n, k, T))[0] if e < ne else np.zeros(n, np.float32)
            assert np.array_equal(c[ti, ui].view(np.uint32), want.view(np.uint32)), (ti, ui)
