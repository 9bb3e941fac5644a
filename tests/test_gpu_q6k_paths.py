"""Q6_K x Q8_1 on the GPU, the branches tests/test_gpu_q6k.py does not reach: q6k_mmq's 64 x 64 form with data in
both K slices, its prefetch and reload loop and gridDim.y > 1 in the 16-row form, the linear tile order past 512
workgroups in both kernels, the decode GEMV's largest LDS classes and its fallback to the MFMA kernel above 160 KiB,
every lanes-per-row form at the M that sit inside a tile and at row counts either side of a workgroup, the bytes
around the tensors, the dequantizer and the refusals on real buffers, and a seeded sweep to K = 5120.

Every product goes through check_guarded: the bars are test_gpu_q6k.check's (the debug_config family and its sumi
twin, bit-equal int32 dots, |c - C64| <= QR.tol(mag, K, W) against the NumPy contract with W = 0 for q6k_gemv and 8
for q6k_mmq at any M, identical bits on a second launch), and the output is written through out= into the interior
of a sentinel-filled [M + 2, N + pad] buffer (row stride above N), the dots through qg_debug_sumi between guard
ints: a store outside the [M, N] window fails the test. Each test also asserts the debug_config substrings of the
path it is there for. The shape tables below import without torch; tests/test_q6k_cpu.py checks them against
debug_config with no GPU.
"""
import functools

import numpy as np
import pytest

import q6k_ref as QR
from test_gpu_q4k_paths import LINEAR_N_RG1, LINEAR_N_RG4, cfg_int, linear_rg4_m, rg4_extent, rows_per_workgroup
from test_gpu_q6k import Q6_K, case, dev, host

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------- the shape tables
RG4_K = (768, 1024, 1280)
MMQ_RG1_EDGES = [(9, 1, 512, "q6k_mmq TT=1 RG=1 KS=8 grid=1x1"),      # N = 1: the N - 1 clamps of wq / wh[e]
                 (16, 15, 256, "q6k_mmq TT=1 RG=1 KS=8 grid=1x1"),
                 (9, 32, 4096, "q6k_mmq TT=1 RG=1 KS=8 grid=2x1"),     # two full passes of the eight slices
                 (31, 33, 2304, "q6k_mmq TT=2 RG=1 KS=8 grid=3x1"),    # nine super-blocks: a ragged second pass
                 (20, 17, 4352, "q6k_mmq TT=2 RG=1 KS=8 grid=2x1"),    # 17 super-blocks: three passes, the last ragged
                 (200, 48, 512, "q6k_mmq TT=4 RG=1 KS=8 grid=3x4")]    # blockIdx.y up to 3, a token tail of 8
# 514 workgroups of 16 and of 64 rows, then 513: on an even grid a tile order that pairs neighbours up wrongly is still
# a permutation of the tiles and changes no result; on an odd one it leaves the last tile undone
LINEAR_GEMV = [(1, 513 * 16 + 1, 4096, 64, 514), (2, 513 * 64 + 1, 256, 4, 514),
               (1, 512 * 16 + 1, 4096, 64, 513), (2, 512 * 64 + 1, 256, 4, 513)]
LINEAR_MMQ_RG1 = (9, LINEAR_N_RG1, 256, "q6k_mmq TT=1 RG=1 KS=8 grid=513x1")
GEMV_LDS_TOP = [(8, 20, 17152, 162944), (5, 20, 27392, 162640)]  # the largest records the GEMV serves (160 KiB = 163840)
GEMV_LDS_OVER = [(8, 20, 17408), (5, 20, 27648)]                  # one super-block more: 165376 and 164160 bytes
# K -> (lanes per row, ONE): one unit per lane and the unit loop for each of the 4 / 16 / 64-lane forms; at 1280 (20
# units over 16 lanes) and 4352 (68 over 64) the last pass is ragged
GEMV_FORMS = {256: (4, 1), 768: (4, 0), 1024: (16, 1), 1280: (16, 0), 4096: (64, 1), 4352: (64, 0)}
GEMV_GUARD_M = {1: 1, 3: 4, 6: 8, 7: 8}  # M -> MT: M = 3, 6, 7 sit inside a tile of 4 or 8 (the m < M guards)
GEMV_RPB = {4: 64, 16: 32, 64: 16}       # lanes per row -> rows per workgroup
FILL_SHAPES = [("q6k_gemv", 3, 33, 768), ("q6k_gemv", 1, 17, 256), ("q6k_mmq", 17, 17, 768), ("q6k_mmq", 9, 1, 512)]
CAPTURED_MMQ = (17, 17, 768, "q6k_mmq TT=2 RG=1 KS=8 grid=2x1")


def rg4_shapes(cus=None):
    """(m, n, k, config) of the 64 x 64 form: M = 65 against the smallest ragged N that fills `cus` CUs (the
    device's unless given), and the same extent in M against N = 65."""
    e, _ = rg4_extent(cus)
    t = (e + 63) // 64
    return ([(65, e, k, f"q6k_mmq TT=4 RG=4 KS=2 grid={t}x2") for k in RG4_K]
            + [(e, 65, 512, f"q6k_mmq TT=4 RG=4 KS=2 grid=2x{t}")])


def path_table(qg, cus=None):
    """Every (m, n, k, algo, exact config or None, config substrings) a test of this module names."""
    rows = [(m, n, k, 0, cfg, ()) for m, n, k, cfg in rg4_shapes(cus) + MMQ_RG1_EDGES + [LINEAR_MMQ_RG1, CAPTURED_MMQ]]
    m = linear_rg4_m(qg, Q6_K)
    rows.append((m, LINEAR_N_RG4, 256, 0, f"q6k_mmq TT=4 RG=4 KS=2 grid=513x{(m + 63) // 64}", ()))
    rows += [(m, n, k, 0, None, ("q6k_gemv ", f" LPR={lpr} ", f" grid={grid} ")) for m, n, k, lpr, grid in LINEAR_GEMV]
    rows += [(m, n, k, 0, None, ("q6k_gemv MT=8 LPR=64 WGS=1024 ONE=0 ", f" lds={lds}")) for m, n, k, lds in GEMV_LDS_TOP]
    for m, n, k in GEMV_LDS_OVER:
        rows += [(m, n, k, algo, None, ("q6k_mmq TT=1 RG=1 KS=8 ",)) for algo in (0, 2)]
    for k, (lpr, one) in GEMV_FORMS.items():
        rows += [(m, 70, k, 0, None, (f"q6k_gemv MT={mt} LPR={lpr} ", f" ONE={one} ")) for m, mt in GEMV_GUARD_M.items()]
        rpb = GEMV_RPB[lpr]
        rows += [(2, n, k, 0, None, (f"q6k_gemv MT=2 LPR={lpr} ", f" ONE={one} grid={(n + rpb - 1) // rpb} "))
                 for n in (1, rpb - 1, rpb, rpb + 1)]
    rows += [(m, n, k, 0, None, (fam + " ",)) for fam, m, n, k in FILL_SHAPES]
    rows.append((3, 16, 512, 2, "q6k_mmq TT=1 RG=1 KS=8 grid=1x1", ()))  # the forced MFMA kernel on the extremes
    return rows


def assert_config(cfg, exact, needles=()):
    if exact is not None:
        assert cfg == exact, (cfg, exact)
    for s in needles:
        assert s in cfg + " ", (cfg, s)


# ---------------------------------------------------------------------------- 1. guarded outputs
F_SENT, I_SENT = -12345.0, 0x5A5A5A5A  # no int32 dot reaches I_SENT (|isum| <= 2^24)
WORST = {"q6k_gemv": 0.0, "q6k_mmq": 0.0, "last": 0.0}  # the largest error / bound ratio per family, and the last one


def stream_ptr():
    import torch
    import quant_gemm._lib as L
    return L.ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def guarded_sumi(a, b, m, n, k, algo=0):
    """qg_debug_sumi into an int32 buffer with 64 + (N % 7) guard ints before and 64 after: (status, dots, guards intact)."""
    import torch
    import quant_gemm._lib as L
    P = L.ctypes.c_void_p
    g0, g1, count = 64 + n % 7, 64, m * n * (k // 32)
    buf = torch.full((g0 + count + g1,), I_SENT, dtype=torch.int32, device="cuda")
    rc = L.load().qg_debug_sumi(P(a.data_ptr()), P(b.data_ptr()), P(buf.data_ptr() + 4 * g0), m, n, k, Q6_K, algo, stream_ptr())
    h = host(buf)
    intact = bool((h[:g0] == I_SENT).all() and (h[g0 + count:] == I_SENT).all())
    return rc, h[g0:g0 + count].reshape(m, n, k // 32), intact


def guarded_product(qg, a, b, m, n, k, algo, pad):
    """gemm_w4a8 through out= into rows 1..M, columns 0..N-1 of a sentinel-filled [M + 2, N + pad] buffer: the window,
    and whether everything around it is still the sentinel."""
    import torch
    buf = torch.full((m + 2, n + pad), F_SENT, dtype=torch.float32, device="cuda")
    out = buf[1:m + 1, :n]
    assert qg.gemm_w4a8(a, b, m, n, k, Q6_K, algo, out=out).data_ptr() == out.data_ptr()
    got = host(buf)
    outside = np.ones(got.shape, bool)
    outside[1:m + 1, :n] = False
    return got[1:m + 1, :n].copy(), bool((got[outside] == np.float32(F_SENT)).all()), got


def check_guarded(qg, aq, bq, ref, fam, algo=0, a=None, b=None, pad=None):
    """test_gpu_q6k.check with both outputs inside guards: config names `fam` and equals its sumi twin; isum bit-equal
    and nothing written around it; output within tolerance, nothing written outside its [M, N] window at a row stride
    of N + pad; a relaunch gives the same bits, window and surroundings."""
    c64, isum, mag = ref
    (m, nb), n = aq.shape[:2], bq.shape[0]
    k = 32 * nb
    cfg = qg.debug_config(m, n, k, Q6_K, algo=algo)
    assert cfg.startswith(fam + " "), cfg
    assert cfg == qg.debug_config(m, n, k, Q6_K, algo=algo, sumi=True)
    a = dev(aq) if a is None else a
    b = dev(bq) if b is None else b
    pad = 1 + (7 * m + 3 * n + nb) % 37 if pad is None else pad
    assert pad >= 1
    rc, s, intact = guarded_sumi(a, b, m, n, k, algo)
    assert rc == 0, rc
    assert intact, "qg_debug_sumi wrote outside its [M, N, K/32] buffer"
    assert np.array_equal(s, isum)
    c, clean, whole = guarded_product(qg, a, b, m, n, k, algo, pad)
    assert clean, f"wrote outside the [M, N] window (ldc = {n + pad})"
    tol = QR.tol(mag, k, 0 if fam == "q6k_gemv" else 8)
    err = np.abs(c.astype(np.float64) - c64)
    ratio = float((err / tol).max())
    WORST[fam] = max(WORST[fam], ratio)
    WORST["last"] = ratio
    print(f"{cfg} M={m} N={n} K={k} ldc={n + pad}: max err/tol = {ratio:.3f}")
    assert (err <= tol).all(), ratio
    _, _, again = guarded_product(qg, a, b, m, n, k, algo, pad)
    assert np.array_equal(whole.view(np.uint32), again.view(np.uint32))
    return c, s


# ---------------------------------------------------------------------------- 2. q6k_mmq at RG = 4, live K slices
@pytest.mark.parametrize("i", range(len(RG4_K) + 1))
def test_mmq_rg4_live_slices(qg, i):
    """64 x 64 tiles, two K slices, both with data: K = 768 leaves slice 1 idle in the last step only, K = 1024 makes
    every slice prefetch the super-block two ahead and reuse a stage buffer after the barrier, K = 1280 does both; the
    last case turns the grid round (blockIdx.y far from 0, K = 512: one super-block per slice)."""
    m, n, k, want = rg4_shapes()[i]
    assert_config(qg.debug_config(m, n, k, Q6_K), want)
    aq, bq, *ref = case(m, n, k)
    check_guarded(qg, aq, bq, ref, "q6k_mmq")


# ---------------------------------------------------------------------------- 3. q6k_mmq at RG = 1: loop and grid edges
@pytest.mark.parametrize("m,n,k,want", MMQ_RG1_EDGES)
def test_mmq_rg1_edges(qg, m, n, k, want):
    assert_config(qg.debug_config(m, n, k, Q6_K), want)
    aq, bq, *ref = case(m, n, k)
    check_guarded(qg, aq, bq, ref, "q6k_mmq")


# ---------------------------------------------------------------------------- 4. linear tile order
@pytest.mark.parametrize("m,n,k,lpr,grid", LINEAR_GEMV)
def test_gemv_linear_tile_order(qg, m, n, k, lpr, grid):
    """More than 512 workgroups: the linear tile order, for the 64-lane and the 4-lane form, on an even and an odd grid."""
    cfg = qg.debug_config(m, n, k, Q6_K)
    assert_config(cfg, None, ("q6k_gemv ", f" LPR={lpr} ", f" grid={grid} "))
    aq, bq, *ref = case(m, n, k)
    check_guarded(qg, aq, bq, ref, "q6k_gemv")


@pytest.mark.parametrize("rg", [1, 4])
def test_mmq_linear_tile_order(qg, rg):
    """gridDim.x = 513 in the 16-row and in the 64-row form (M grown from 33 where 513 tiles do not fill the device)."""
    if rg == 1:
        m, n, k, want = LINEAR_MMQ_RG1
    else:
        m, n, k = linear_rg4_m(qg, Q6_K), LINEAR_N_RG4, 256
        want = f"q6k_mmq TT=4 RG=4 KS=2 grid=513x{(m + 63) // 64}"
    assert_config(qg.debug_config(m, n, k, Q6_K), want)
    aq, bq, *ref = case(m, n, k)
    check_guarded(qg, aq, bq, ref, "q6k_mmq")


# ---------------------------------------------------------------------------- 5. GEMV LDS classes
@pytest.mark.parametrize("m,n,k,lds", GEMV_LDS_TOP)
def test_gemv_lds_at_the_160k_end(qg, m, n, k, lds):
    """The last super-block count whose records (M * K/256 * 304 bytes) the GEMV serves, at M = 8 and at M = 5 in MT = 8."""
    assert lds == m * (k // 256) * 304 <= 160 * 1024 < m * (k // 256 + 1) * 304
    assert_config(qg.debug_config(m, n, k, Q6_K), None, ("q6k_gemv MT=8 LPR=64 WGS=1024 ONE=0 ", f" lds={lds}"))
    aq, bq, *ref = case(m, n, k)
    check_guarded(qg, aq, bq, ref, "q6k_gemv")


@pytest.mark.parametrize("m,n,k", GEMV_LDS_OVER)
def test_gemv_lds_above_160k_falls_back(qg, m, n, k):
    """Records beyond 160 KiB: AUTO runs q6k_mmq at M <= 8 (within W = 8; 68 and 108 super-blocks, which no M >= 9 shape
    of the suite has), the forced GEMV is refused (-3) by every entry with the output untouched."""
    import torch
    import quant_gemm._lib as L
    P = L.ctypes.c_void_p
    assert m * (k // 256) * 304 > 160 * 1024
    assert qg.select_algo(m, n, k, Q6_K) == 2
    assert qg.debug_config(m, n, k, Q6_K).startswith("q6k_mmq TT=1 RG=1 KS=8 ")
    aq, bq, *ref = case(m, n, k)
    a, b = dev(aq), dev(bq)
    check_guarded(qg, aq, bq, ref, "q6k_mmq", a=a, b=b)
    with pytest.raises(RuntimeError, match="unsupported"):
        qg.debug_config(m, n, k, Q6_K, algo=1)
    with pytest.raises(RuntimeError, match="unsupported"):
        qg.gemm_w4a8(a, b, m, n, k, Q6_K, algo=1)
    with pytest.raises(RuntimeError, match="unsupported"):
        qg.debug_sumi(a, b, m, n, k, Q6_K, algo=1)
    out = torch.full((m, n), F_SENT, dtype=torch.float32, device="cuda")
    assert L.load().qg_gemm_w4a8_ex(P(a.data_ptr()), P(b.data_ptr()), P(out.data_ptr()), m, n, k, Q6_K, 1, stream_ptr()) == -3
    assert (host(out) == np.float32(F_SENT)).all()
    rc, _, intact = guarded_sumi(a, b, m, n, k, algo=1)
    assert rc == -3 and intact


# ---------------------------------------------------------------------------- 6. GEMV forms x M guards x row edges
@pytest.mark.parametrize("k", list(GEMV_FORMS))
@pytest.mark.parametrize("m", list(GEMV_GUARD_M))
def test_gemv_forms_and_m_guards(qg, m, k):
    """Every (lanes per row, ONE) form at M = 1 and at M = 3, 6, 7, inside a tile of 4 / 8 / 8: a store at m >= M lands
    in the guard row below the window."""
    n = 70
    lpr, one = GEMV_FORMS[k]
    assert_config(qg.debug_config(m, n, k, Q6_K), None, (f"q6k_gemv MT={GEMV_GUARD_M[m]} LPR={lpr} ", f" ONE={one} "))
    aq, bq, *ref = case(m, n, k)
    check_guarded(qg, aq, bq, ref, "q6k_gemv")


@pytest.mark.parametrize("k", list(GEMV_FORMS))
def test_gemv_rows_around_a_workgroup(qg, k):
    """N = 1 and N one either side of the rows per workgroup (read from the config, not assumed)."""
    m = 2
    lpr, one = GEMV_FORMS[k]
    cfg = qg.debug_config(m, 1, k, Q6_K)
    assert_config(cfg, None, (f"q6k_gemv MT=2 LPR={lpr} ", f" ONE={one} "))
    rpb = rows_per_workgroup(cfg)
    assert rpb == GEMV_RPB[lpr]
    for n in (1, rpb - 1, rpb, rpb + 1):
        assert cfg_int(qg.debug_config(m, n, k, Q6_K), "grid") == (n + rpb - 1) // rpb
        aq, bq, *ref = case(m, n, k)
        check_guarded(qg, aq, bq, ref, "q6k_gemv")


# ---------------------------------------------------------------------------- 7. the bytes around the tensors
@pytest.mark.parametrize("fam,m,n,k", FILL_SHAPES)
@pytest.mark.parametrize("woff", [0, 2, 18])
@pytest.mark.parametrize("aoff", [0, 4, 12])
def test_bytes_around_the_tensors_reach_no_result(qg, aoff, woff, fam, m, n, k):
    """Weights and activations inside flat buffers whose every other byte is 0xFF (f16 pairs: NaN; codes: 63; scales:
    -1), then 0x00: both pass the bars and give the same bits. What the kernels read past a piece, and the rows,
    units and tokens they clamp, is never used. (Where they read is by construction; this does not probe it.)"""
    aq, bq, *ref = case(m, n, k)
    res = []
    for fill in (0xFF, 0x00):
        a, b = QR.dev_at(aq, aoff, fill), QR.dev_at(bq, woff, fill)
        assert b.data_ptr() % 256 == woff and a.data_ptr() % 256 == aoff
        res.append(check_guarded(qg, aq, bq, ref, fam, a=a, b=b))
    (c1, s1), (c0, s0) = res
    assert np.array_equal(c1.view(np.uint32), c0.view(np.uint32)) and np.array_equal(s1, s0)


# ---------------------------------------------------------------------------- 8. around the kernels
def test_dequantize_at_a_2_byte_offset(qg):
    import torch
    import quant_gemm._lib as L
    P = L.ctypes.c_void_p
    bq = QR.random_q6k(np.random.default_rng(21), 5, 768)
    x = QR.dev_at(bq, 2)
    y = torch.full((bq.size // 210 * 256 + 2,), -3.0, dtype=torch.float32, device="cuda")
    out = y[1:-1]
    assert x.data_ptr() % 4 == 2 and out.data_ptr() % 8 == 4
    assert L.load().qg_dequantize(Q6_K, P(x.data_ptr()), P(out.data_ptr()), out.numel(), stream_ptr()) == 0
    got = host(y)
    assert got[0] == -3.0 and got[-1] == -3.0
    assert np.array_equal(got[1:-1].view(np.uint32), QR.dequant(bq).reshape(-1).view(np.uint32))
    # through the Python face (its own output buffer), the input still at the 2-B offset
    assert np.array_equal(host(qg.dequantize(x, Q6_K)).view(np.uint32), QR.dequant(bq).view(np.uint32))
    assert L.load().qg_dequantize(Q6_K, P(x.data_ptr() + 1), P(out.data_ptr()), out.numel(), stream_ptr()) == -4
    assert np.array_equal(host(y).view(np.uint32), got.view(np.uint32))


@functools.lru_cache(maxsize=None)
def extreme_case(m):
    aq, bq = QR.extremes(np.random.default_rng([7, m]), m, 16, 512)
    return (aq, bq) + QR.gemm(aq, bq)


def test_dequantize_extremes(qg):
    """d at the f16 subnormals, the smallest normal and +-65504, scales -128 / 127 / 0, codes all 0 and all 63."""
    _, bq, *_ = extreme_case(3)
    want = QR.dequant(bq)
    assert np.isfinite(want).all() and np.abs(want).max() == 65504.0 * 128 * 32
    y = host(qg.dequantize(dev(bq), Q6_K))
    assert np.isfinite(y).all()
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("woff,aoff", [(1, 0), (3, 4), (17, 0), (0, 2), (2, 6), (18, 1)])
def test_misaligned_pointers_are_refused(qg, woff, aoff):
    """Weights at an odd address or activations off 4 B, on real buffers: -4 from every entry for every algo, the
    Python face raises, the output and the sumi buffer untouched."""
    import torch
    import quant_gemm._lib as L
    P = L.ctypes.c_void_p
    m, n, k = 3, 20, 512
    aq, bq, *_ = case(m, n, k)
    a, b = QR.dev_at(aq, aoff), QR.dev_at(bq, woff)
    assert b.data_ptr() % 2 == 1 or a.data_ptr() % 4 != 0
    out = torch.full((m, n), F_SENT, dtype=torch.float32, device="cuda")
    so = L.load()
    for algo in (0, 1, 2):
        assert so.qg_gemm_w4a8_ex(P(a.data_ptr()), P(b.data_ptr()), P(out.data_ptr()), m, n, k, Q6_K, algo, stream_ptr()) == -4
        rc, _, intact = guarded_sumi(a, b, m, n, k, algo)
        assert rc == -4 and intact
    with pytest.raises(RuntimeError, match="misaligned"):
        qg.gemm_w4a8(a, b, m, n, k, Q6_K, out=out)
    with pytest.raises(RuntimeError, match="misaligned"):
        qg.debug_sumi(a, b, m, n, k, Q6_K)
    assert (host(out) == np.float32(F_SENT)).all()


def test_forced_mmq_on_extremes(qg):
    """The ends of the scale formats (QR.extremes) at M = 3 through the forced MFMA kernel: within W = 8, finite, the
    all-zero-scale row exactly 0, the dots those of the GEMV."""
    aq, bq, *ref = extreme_case(3)
    assert np.abs(ref[1]).max() == 2 ** 24
    assert_config(qg.debug_config(3, 16, 512, Q6_K, algo=2), "q6k_mmq TT=1 RG=1 KS=8 grid=1x1")
    c, s2 = check_guarded(qg, aq, bq, ref, "q6k_mmq", algo=2)
    assert np.isfinite(c).all() and (c[:, 7] == 0).all()
    _, s1 = check_guarded(qg, aq, bq, ref, "q6k_gemv", algo=1)
    assert np.array_equal(s1, s2)


def test_captured_mmq_replays_the_eager_bits(qg):
    import torch
    m, n, k, want = CAPTURED_MMQ
    assert_config(qg.debug_config(m, n, k, Q6_K), want)
    aq, bq, *ref = case(m, n, k)
    a, b = dev(aq), dev(bq)
    eager, _ = check_guarded(qg, aq, bq, ref, "q6k_mmq", a=a, b=b)
    out = torch.full((m, n), F_SENT, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        qg.gemm_w4a8(a, b, m, n, k, Q6_K, out=out)
    g.replay()
    assert np.array_equal(host(out).view(np.uint32), eager.view(np.uint32))


# ---------------------------------------------------------------------------- 9. seeded sweep
def test_seeded_path_sweep(qg):
    """24 seeded cases (QR.path_fuzz_cases): M over every tile form, N in 1..300, K = 256 * (1..20), weights 2 / 18 and
    activations 4 / 8 / 12 bytes past a 256-B boundary, each through check_guarded. None is skipped; the largest
    error / bound ratio is printed and must be <= 1."""
    worst = 0.0
    for i, m, n, k, woff, aoff in QR.path_fuzz_cases():
        aq, bq, *ref = case(m, n, k, seed=2000 + i)
        fam = "q6k_gemv" if m <= 8 else "q6k_mmq"  # (K <= 5120: no M <= 8 shape of the sweep exceeds the LDS)
        check_guarded(qg, aq, bq, ref, fam, a=QR.dev_at(aq, aoff), b=QR.dev_at(bq, woff))
        worst = max(worst, WORST["last"])
    print(f"Q6_K path sweep: largest err/tol = {worst:.3f}; whole module so far: "
          f"q6k_gemv {WORST['q6k_gemv']:.3f}, q6k_mmq {WORST['q6k_mmq']:.3f}")
    assert worst <= 1.0
