"""Q4_K x Q8_1 on the GPU, the branches tests/test_gpu_q4k.py does not reach: the decode GEMV's LDS opt-in above
64 KiB and its fallback to the MFMA kernel above 160 KiB, every lanes-per-row form with and without the unit loop
at every M tile, row counts either side of a workgroup, the MFMA kernel's 64 x 64 form over several super-blocks,
its clamps at N < 16, pointers at the contract's alignment (weights 16 B, activations 4 B, dequantizer 2 B), the
ends of the f16 scale formats, and a seeded sweep.

The bars are test_gpu_q4k.check's, unchanged: the debug_config family, bit-equal int32 dots, |c - C64| <=
KR.tol(mag, K, W) against the NumPy contract (W = 0 for q4k_gemv, 16 for q4k_mmq at any M), identical bits on a
second launch. Each test also asserts the debug_config substrings of the path it is there for.
"""
import functools
import re

import numpy as np
import pytest

import kquant_ref as KR
import test_gpu_q4k as T
from test_gpu_product import dev, host
from test_gpu_q4k import Q4_K, case, check

pytestmark = pytest.mark.gpu


def cfg_int(cfg, key):
    return int(re.search(rf"\b{key}=(\d+)", cfg).group(1))


def rows_per_workgroup(cfg):
    return (cfg_int(cfg, "WGS") // 64) * (64 // cfg_int(cfg, "LPR"))


# ---------------------------------------------------------------------------- 1. GEMV LDS classes
@pytest.mark.parametrize("m,n,k", [(8, 40, 6400), (8, 24, 14336), (8, 20, 15360)])
def test_gemv_lds_above_64k(qg, m, n, k):
    """The opt-in for more than 64 KiB of LDS (the product and the sumi instantiation each take it once)."""
    cfg = qg.debug_config(m, n, k, Q4_K)
    lds = m * (k // 256) * 336
    assert 65536 < lds <= 160 * 1024
    assert cfg_int(cfg, "lds") == lds, cfg
    assert "MT=8 LPR=64 WGS=1024 ONE=0" in cfg, cfg
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "q4k_gemv")


@pytest.mark.parametrize("m,n,k", [(8, 20, 15616), (5, 20, 25088)])
def test_gemv_lds_above_160k_falls_back(qg, m, n, k):
    """Records beyond 160 KiB: AUTO runs q4k_mmq at M <= 8 (within W = 16), the forced GEMV is refused (-3)."""
    import quant_gemm._lib as L
    assert m * (k // 256) * 336 > 160 * 1024
    assert qg.select_algo(m, n, k, Q4_K) == 2
    cfg = qg.debug_config(m, n, k, Q4_K)
    assert cfg.startswith("q4k_mmq TT=1 RG=1 KS=8 "), cfg
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "q4k_mmq")
    with pytest.raises(RuntimeError, match="unsupported"):
        qg.debug_config(m, n, k, Q4_K, algo=1)
    a, b = dev(aq), dev(bq)
    with pytest.raises(RuntimeError, match="unsupported"):
        qg.gemm_w4a8(a, b, m, n, k, Q4_K, algo=1)
    with pytest.raises(RuntimeError, match="unsupported"):
        qg.debug_sumi(a, b, m, n, k, Q4_K, algo=1)
    import torch
    out = torch.full((m, n), -7.0, dtype=torch.float32, device="cuda")
    P = L.ctypes.c_void_p
    assert L.load().qg_gemm_w4a8_ex(P(a.data_ptr()), P(b.data_ptr()), P(out.data_ptr()), m, n, k, Q4_K, 1, None) == -3
    assert (host(out) == -7.0).all()


# ---------------------------------------------------------------------------- 2. GEMV forms x M
# K -> (lanes per row, ONE): one unit per lane and the unit loop for each of the 4 / 16 / 64-lane forms; at 1280
# (20 units over 16 lanes) and 4352 (68 over 64) the last pass is ragged
GEMV_FORMS = {256: (4, 1), 768: (4, 0), 1024: (16, 1), 1280: (16, 0), 4096: (64, 1), 4352: (64, 0)}


@pytest.mark.parametrize("k", list(GEMV_FORMS))
@pytest.mark.parametrize("m", [1, 3, 6, 7])
def test_gemv_forms_and_m_guards(qg, m, k):
    n = 70
    lpr, one = GEMV_FORMS[k]
    cfg = qg.debug_config(m, n, k, Q4_K)
    mt = {1: 1, 3: 4, 6: 8, 7: 8}[m]  # M = 3, 6, 7 sit inside a tile of 4 or 8: the m < M guards
    assert f"MT={mt} LPR={lpr} " in cfg and f" ONE={one} " in cfg, cfg
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "q4k_gemv")


@pytest.mark.parametrize("k", list(GEMV_FORMS))
def test_gemv_rows_around_a_workgroup(qg, k):
    """N = 1 and N one either side of the rows per workgroup (read from the config, not assumed)."""
    m = 2
    lpr, one = GEMV_FORMS[k]
    cfg = qg.debug_config(m, 1, k, Q4_K)
    assert f"MT=2 LPR={lpr} " in cfg and f" ONE={one} " in cfg, cfg
    rpb = rows_per_workgroup(cfg)
    assert rpb == {4: 64, 16: 32, 64: 16}[lpr]
    for n in (1, rpb - 1, rpb, rpb + 1):
        assert cfg_int(qg.debug_config(m, n, k, Q4_K), "grid") == (n + rpb - 1) // rpb
        aq, bq, *ref = case(m, n, k)
        check(qg, aq, bq, ref, "q4k_gemv")


@pytest.mark.parametrize("m,n,k,lpr", [(1, 513 * 16 + 1, 4096, 64), (2, 513 * 64 + 1, 256, 4)])
def test_gemv_linear_tile_order(qg, m, n, k, lpr):
    """More than 512 workgroups: the linear tile order, for the 64-lane and the 4-lane form."""
    cfg = qg.debug_config(m, n, k, Q4_K)
    assert f"LPR={lpr} " in cfg and cfg_int(cfg, "grid") == 514, cfg
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "q4k_gemv")


# ---------------------------------------------------------------------------- 3. MMQ RG = 4, several super-blocks
def rg4_extent(cus=None):
    """The smallest ragged extent e with ceil(e / 64) * 2 >= CUs: against 65 in the other dimension it is the
    smallest grid, ragged both ways, that the rule ceil(N / 64) * ceil(M / 64) >= CUs sends to RG = 4. `cus`: the
    device's count unless given (the routing tests that run without a GPU give the library's answer there, 256)."""
    if cus is None:
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 64 * ((cus + 1) // 2 - 1) + 1, cus


@pytest.mark.parametrize("k", [768, 1024, 1280])
def test_mmq_rg4_several_superblocks(qg, k):
    """64 x 64 tiles, two K slices: K = 768 leaves slice 1 idle in the last step only, K = 1024 makes every slice
    prefetch the super-block two ahead and reuse a stage buffer after the barrier, K = 1280 does both (at K = 768
    the clamp to the last super-block hides a wrong prefetch distance: the only next super-block is the last)."""
    n, cus = rg4_extent()
    m = 65
    cfg = qg.debug_config(m, n, k, Q4_K)
    assert "TT=4 RG=4 KS=2" in cfg and f"grid={(n + 63) // 64}x2" in cfg, (cfg, cus)
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "q4k_mmq")


def test_mmq_rg4_many_token_tiles(qg):
    """The tiles the other way round: blockIdx.y far from 0."""
    m, cus = rg4_extent()
    n, k = 65, 512
    cfg = qg.debug_config(m, n, k, Q4_K)
    assert "TT=4 RG=4 KS=2" in cfg and f"grid=2x{(m + 63) // 64}" in cfg, (cfg, cus)
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "q4k_mmq")


# ---------------------------------------------------------------------------- 4. MMQ edges at RG = 1
@pytest.mark.parametrize("m,n,k,tt,grid", [(9, 1, 512, 1, "1x1"), (16, 15, 256, 1, "1x1"), (20, 17, 768, 2, "2x1"),
                                           (9, 32, 4096, 1, "2x1"), (200, 48, 512, 4, "3x4"), (31, 33, 2304, 2, "3x1")])
def test_mmq_rg1_edges(qg, m, n, k, tt, grid):
    """N below one 16-row group (the N - 1 clamps of the weight and header pointers), two full passes of the eight
    K slices (K = 4096), four token tiles in gridDim.y."""
    cfg = qg.debug_config(m, n, k, Q4_K)
    assert f"q4k_mmq TT={tt} RG=1 KS=8 grid={grid}" == cfg, cfg
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "q4k_mmq")


LINEAR_N_RG1, LINEAR_N_RG4 = 16 * 512 + 1, 64 * 512 + 1  # 513 tiles of 16 and of 64 weight rows


def linear_rg4_m(qg, wtype, n=LINEAR_N_RG4, k=256):
    """M for the 513 x gy grid of 64 x 64 tiles: 33 where 513 tiles fill the device (ceil(N / 64) * ceil(M / 64) >=
    CUs), otherwise grown in steps of 64 until the dispatch picks RG = 4."""
    m = 33
    while "RG=4" not in qg.debug_config(m, n, k, wtype):
        m += 64
        assert m <= 33 + 64 * 8, "no RG = 4 grid of 513 tiles on this device"
    return m


@pytest.mark.parametrize("rg", [1, 4])
def test_mmq_linear_tile_order(qg, rg):
    """gridDim.x = 513: past one dispatch round the tiles are taken in linear order, in the 16-row and the 64-row form."""
    k = 256
    if rg == 1:
        m, n, want = 9, LINEAR_N_RG1, "q4k_mmq TT=1 RG=1 KS=8 grid=513x1"
    else:
        m, n = linear_rg4_m(qg, Q4_K), LINEAR_N_RG4
        want = f"q4k_mmq TT=4 RG=4 KS=2 grid=513x{(m + 63) // 64}"
    cfg = qg.debug_config(m, n, k, Q4_K)
    assert cfg == want, cfg
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "q4k_mmq")


# ---------------------------------------------------------------------------- 5. pointers off 256 B
OFFSET_SHAPES = [("q4k_gemv", 3, 70, 1280), ("q4k_gemv", 1, 20, 4096), ("q4k_mmq", 17, 40, 768)]


@pytest.mark.parametrize("fam,m,n,k", OFFSET_SHAPES)
@pytest.mark.parametrize("woff,aoff", list(zip(KR.W_OFFSETS, KR.A_OFFSETS)))
def test_pointers_at_the_contract_alignment(qg, monkeypatch, woff, aoff, fam, m, n, k):
    """check() with its uploads placed woff / aoff bytes past a 256-B boundary; the bits equal the aligned call's."""
    seen = []

    def place(x):
        off = {36: aoff, 144: woff}[x.shape[-1]]
        t = KR.dev_at(x, off)
        seen.append(t.data_ptr() % 256)
        return t

    aq, bq, *ref = case(m, n, k)
    monkeypatch.setattr(T, "dev", place)
    c, s = check(qg, aq, bq, ref, fam)
    monkeypatch.undo()
    assert seen == [aoff % 256, woff % 256]
    c0 = host(qg.gemm_w4a8(dev(aq), dev(bq), m, n, k, Q4_K))
    assert np.array_equal(c.view(np.uint32), c0.view(np.uint32))


def test_dequantize_at_2_and_4_byte_offsets(qg):
    import torch
    import quant_gemm._lib as L
    P = L.ctypes.c_void_p
    b = KR.random_q4k(np.random.default_rng(21), 5, 768)
    x = KR.dev_at(b, 2)
    y = torch.full((b.size // 144 * 256 + 2,), -3.0, dtype=torch.float32, device="cuda")
    out = y[1:-1]
    assert x.data_ptr() % 4 == 2 and out.data_ptr() % 8 == 4
    assert L.load().qg_dequantize(Q4_K, P(x.data_ptr()), P(out.data_ptr()), out.numel(), None) == 0
    got = host(y)
    assert got[0] == -3.0 and got[-1] == -3.0
    assert np.array_equal(got[1:-1].view(np.uint32), KR.dequant(b).reshape(-1).view(np.uint32))
    # through the Python face (its own output buffer), the input still at the 2-B offset
    assert np.array_equal(host(qg.dequantize(x, Q4_K)).view(np.uint32), KR.dequant(b).view(np.uint32))
    assert L.load().qg_dequantize(Q4_K, P(x.data_ptr() + 1), P(out.data_ptr()), out.numel(), None) == -4


@pytest.mark.parametrize("woff,aoff", [(4, 0), (8, 0), (0, 2), (24, 4), (16, 6)])
def test_misaligned_pointers_are_refused(qg, woff, aoff):
    """Weights off 16 B or activations off 4 B: -4 from every entry, the output untouched."""
    import torch
    import quant_gemm._lib as L
    P = L.ctypes.c_void_p
    m, n, k = 3, 20, 512
    aq, bq, *_ = case(m, n, k)
    a, b = KR.dev_at(aq, aoff), KR.dev_at(bq, woff)
    out = torch.full((m, n), -9.0, dtype=torch.float32, device="cuda")
    sumi = torch.full((m, n, k // 32), -9, dtype=torch.int32, device="cuda")
    so = L.load()
    for algo in (0, 1, 2):
        assert so.qg_gemm_w4a8_ex(P(a.data_ptr()), P(b.data_ptr()), P(out.data_ptr()), m, n, k, Q4_K, algo, None) == -4
        assert so.qg_debug_sumi(P(a.data_ptr()), P(b.data_ptr()), P(sumi.data_ptr()), m, n, k, Q4_K, algo, None) == -4
    with pytest.raises(RuntimeError, match="misaligned"):
        qg.gemm_w4a8(a, b, m, n, k, Q4_K, out=out)
    assert (host(out) == -9.0).all() and (host(sumi) == -9).all()


# ---------------------------------------------------------------------------- 6. the ends of the scale formats
@functools.lru_cache(maxsize=None)
def extreme_case(m):
    aq, bq = KR.extremes(np.random.default_rng([6, m]), m)
    return (aq, bq) + KR.gemm(aq, bq)


@pytest.mark.parametrize("m", [2, 12])
def test_scale_extremes(qg, m):
    """f16 subnormal, smallest normal and +-65504 weight scales, subnormal d_a, large negative s_a, sc / m at 0
    and 63 and at the 6-bit values whose high bits sit in another byte: each class in its own weight row."""
    aq, bq, *ref = extreme_case(m)
    c64, _, mag = ref
    assert np.isfinite(c64).all() and mag.max() < 1e18 and (mag > 0).all()
    check(qg, aq, bq, ref, "q4k_gemv" if m <= 8 else "q4k_mmq")
    if m <= 8:  # the MFMA kernel, forced, on the same two tokens
        check(qg, aq, bq, ref, "q4k_mmq", algo=2)


def test_scale_extremes_dequantize(qg):
    _, bq, *_ = extreme_case(2)
    y = host(qg.dequantize(dev(bq), Q4_K))
    want = KR.dequant(bq)
    assert np.isfinite(want).all()
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------------------- 7. seeded sweep
@pytest.mark.parametrize("i,m,n,k,woff,aoff", KR.fuzz_cases())
def test_random_shapes_offsets_and_strided_out(qg, i, m, n, k, woff, aoff):
    """Random shape and pointer offsets, the output written through out= into the top-left corner of a
    sentinel-filled [M + 1, N + pad] buffer."""
    import torch
    rng = np.random.default_rng(7000 + i)
    aq, bq = KR.random_q8_1(rng, m, k), KR.random_q4k(rng, n, k)
    pad = int(rng.integers(1, 40))
    c64, sumi, mag = KR.gemm(aq, bq)
    fam = qg.debug_config(m, n, k, Q4_K).split(" ")[0]
    assert fam == ("q4k_gemv" if m <= 8 else "q4k_mmq")  # (K <= 5120: no M <= 8 shape of the sweep exceeds the LDS)
    a, b = KR.dev_at(aq, aoff), KR.dev_at(bq, woff)
    buf = torch.full((m + 1, n + pad), -12345.0, dtype=torch.float32, device="cuda")
    out = qg.gemm_w4a8(a, b, m, n, k, Q4_K, out=buf[:m, :n])
    assert out.data_ptr() == buf.data_ptr()
    got = host(buf)
    assert (got[:m, n:] == -12345.0).all() and (got[m] == -12345.0).all(), "wrote outside the slice"
    tol = KR.tol(mag, k, 0 if fam == "q4k_gemv" else 16)
    err = np.abs(got[:m, :n].astype(np.float64) - c64)
    print(f"{fam} M={m} N={n} K={k} w+{woff} a+{aoff}: max err/tol = {(err / tol).max():.3f}")
    assert (err <= tol).all(), (err / tol).max()
    assert np.array_equal(host(qg.debug_sumi(a, b, m, n, k, Q4_K)), sumi)
