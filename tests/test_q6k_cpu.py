"""Q6_K (ggml type 14) without a GPU: the format model (tests/q6k_ref.py), the C-ABI's validation and routing for the
type, the view adapter's checks and the host twin against the NumPy contract. No kernel is launched."""
import ctypes

import numpy as np
import pytest

import q6k_ref as QR

Q6_K = 14
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def so():
    import quant_gemm._lib as L
    return L.load()


# ---------------------------------------------------------------------------- the model itself
def test_build_fields_round_trip():
    rng = np.random.default_rng(3)
    b = QR.random_q6k(rng, 3, 768)
    d, sc, q = QR.fields(b)
    assert q.min() >= -32 and q.max() <= 31 and sc.min() >= -128 and sc.max() <= 127
    assert np.array_equal(QR.build(d, sc, q), b)


def test_element_placement_follows_the_formula():
    """256 blocks with one nonzero code each: element e = 128h + 32c + l lives in ql[64h + 32(c & 1) + l] (nibble
    c >> 1) and qh[32h + l] (bit pair c), and nowhere else."""
    for code in (63, 0x15, 0x2A):
        q = np.full((256, 256), -32, np.int32)
        q[np.arange(256), np.arange(256)] = code - 32
        b = QR.build(np.ones(256), np.ones((256, 16), np.int8), q)
        for e in range(256):
            h, p = divmod(e, 128)
            c, l = divmod(p, 32)
            want = np.zeros(210, np.uint8)
            want[64 * h + 32 * (c & 1) + l] = (code & 15) << (4 * (c >> 1))
            want[128 + 32 * h + l] = (code >> 4) << (2 * c)
            want[192:208] = 1
            want[208:210] = np.array([1.0], np.float16).view(np.uint8)
            assert np.array_equal(b[e], want), (code, e)
        assert np.array_equal(QR.fields(b)[2], q)


def test_code_dwords_match_the_byte_definition():
    """The dword form the kernels use (masks of a ql dword pair and a qh dword, then the carry-free -32) equals the
    per-element definition, for every block c of a half."""
    rng = np.random.default_rng(1)
    b = rng.integers(0, 256, (500, 210), dtype=np.uint8)
    _, _, q = QR.fields(b)
    for h in range(2):
        for j in range(8):  # dword j of the 32-byte pieces
            a = b[:, 64 * h + 4 * j:64 * h + 4 * j + 4].copy().view("<u4")[:, 0].astype(np.uint64)
            bb = b[:, 64 * h + 32 + 4 * j:64 * h + 36 + 4 * j].copy().view("<u4")[:, 0].astype(np.uint64)
            hh = b[:, 128 + 32 * h + 4 * j:128 + 32 * h + 4 * j + 4].copy().view("<u4")[:, 0].astype(np.uint64)
            u = [(a & 0x0F0F0F0F) | ((hh << 4) & 0x30303030), (bb & 0x0F0F0F0F) | ((hh << 2) & 0x30303030),
                 ((a >> 4) & 0x0F0F0F0F) | (hh & 0x30303030), ((bb >> 4) & 0x0F0F0F0F) | ((hh >> 2) & 0x30303030)]
            for c in range(4):
                s = (((u[c] | 0x80808080) - 0x20202020) ^ 0x80808080) & 0xFFFFFFFF
                got = s.astype("<u4").view(np.int8).reshape(-1, 4).astype(np.int32)
                e0 = 128 * h + 32 * c + 4 * j
                assert np.array_equal(got, q[:, e0:e0 + 4]), (h, j, c)


def test_dequant_follows_the_definition():
    rng = np.random.default_rng(4)
    b = QR.random_q6k(rng, 2, 512)
    d, sc, q = QR.fields(b)
    y = QR.dequant(b).reshape(2, 2, 256)
    for e in (0, 17, 100, 255):
        want = np.float32(np.float32(d[1, 1] * np.float32(sc[1, 1, e // 16])) * np.float32(q[1, 1, e]))
        assert y[1, 1, e] == want


def test_gemm_model_against_a_direct_loop():
    rng = np.random.default_rng(5)
    aq, bq = QR.random_q8_1(rng, 2, 512), QR.random_q6k(rng, 3, 512)
    c64, isum, mag = QR.gemm(aq, bq)
    d, sc, q = QR.fields(bq)
    da, qa = QR.q8_1_fields(aq)
    for m, n, blk in ((0, 0, 0), (1, 2, 9), (1, 1, 15)):
        sb, b = divmod(blk, 8)
        s0 = int((qa[m, blk, :16] * q[n, sb, 32 * b:32 * b + 16]).sum())
        s1 = int((qa[m, blk, 16:] * q[n, sb, 32 * b + 16:32 * b + 32]).sum())
        assert isum[m, n, blk] == sc[n, sb, 2 * b] * s0 + sc[n, sb, 2 * b + 1] * s1
    want = sum(float(d[2, blk // 8]) * da[1, blk] * int(isum[1, 2, blk]) for blk in range(16))
    assert abs(c64[1, 2] - want) <= 1e-12 * mag[1, 2]


def test_extremes_builder_holds_what_it_claims():
    for m in (2, 12):
        aq, bq = QR.extremes(np.random.default_rng([6, m]), m)
        d, sc, q = QR.fields(bq)
        assert np.isfinite(d).all()
        sub = lambda x: ((np.abs(x) >= 2.0 ** -24) & (np.abs(x) < 2.0 ** -14)).all()
        assert sub(d[:2]) and (d[:2] > 0).any() and (d[:2] < 0).any()
        assert (np.abs(d[2]) == 2.0 ** -14).all() and (d[3] == 65504).all() and (d[4] == -65504).all()
        assert (sc[5] == -128).all() and (sc[6] == 127).all() and (sc[7] == 0).all()
        assert (q[8] == -32).all() and (q[9] == 31).all()
        da, qa = QR.q8_1_fields(aq)
        assert sub(da[0]) and (da[1] == 65504).all() and (qa[1] == -128).all()
        c64, isum, mag = QR.gemm(aq, bq)
        assert np.isfinite(c64).all() and np.abs(isum[1, 10]).max() == 2 ** 24
        assert (c64[:, 7] == 0).all()


def test_fuzz_cases_are_seeded_and_cover_both_families():
    cases = QR.fuzz_cases()
    assert cases == QR.fuzz_cases() and len(cases) == 16
    assert all(m in QR.SWEEP_M and 1 <= n <= 200 and k % 256 == 0 and 256 <= k <= 3072 for _, m, n, k, _, _ in cases)
    assert {w for *_, w, _ in cases} == set(QR.W_OFFSETS) and {a for *_, a in cases} == set(QR.A_OFFSETS)
    ms = [m for _, m, *_ in cases]
    assert sum(m <= 8 for m in ms) >= 4 and sum(m > 8 for m in ms) >= 4


# ---------------------------------------------------------------------------- the C ABI
def test_static_queries(so):
    assert so.qg_block_bytes(Q6_K) == 210 and so.qg_block_elems(Q6_K) == 256
    assert so.qg_block_bytes(12) == 144 and so.qg_block_bytes(13) == 0 and so.qg_block_elems(13) == 0
    import quant_gemm as qg
    import quant_gemm.host as host
    from quant_gemm import ggml as G
    assert qg.Q6_K == 14 and qg.BLOCK_BYTES[qg.Q6_K] == 210 and qg.block_elems(qg.Q6_K) == 256
    assert qg.Q6_K in qg.GEMM_WEIGHT_TYPES and qg.Q6_K not in qg.WEIGHT_TYPES and "Q6_K" in qg.__all__
    assert host.BLOCK_BYTES[14] == 210 and G.Q6_K == 14


def test_validation_codes_without_launch(so):
    fake = P(4096)  # never dereferenced: validation fails first
    for k in (288, 0, -256, 128):
        assert so.qg_gemm_w4a8(fake, fake, fake, 1, 1, k, Q6_K, None) == -2, k          # K % 256
    assert so.qg_gemm_w4a8(fake, P(4097), fake, 1, 1, 256, Q6_K, None) == -4             # weights at an odd address
    assert so.qg_gemm_w4a8(P(4098), fake, fake, 1, 1, 256, Q6_K, None) == -4             # activations off 4 B
    assert so.qg_gemm_w4a8_ex(fake, fake, fake, 1, 1, 256, Q6_K, 3, None) == -3          # generic
    assert so.qg_gemm_w4a8_ex(fake, fake, fake, 1, 1, 256, Q6_K, 4, None) == -3          # ragged
    assert so.qg_gemm_w4a8(None, None, None, 0, 5, 256, Q6_K, None) == 0                 # M = 0: no-op
    assert so.qg_gemm_w4a8(None, None, None, 5, 0, 256, Q6_K, None) == 0                 # N = 0: no-op
    assert so.qg_gemm_w4a8(fake, fake, fake, -1, 1, 256, Q6_K, None) == -1
    assert so.qg_gemm_w4a8(None, fake, fake, 1, 1, 256, Q6_K, None) == -1
    assert so.qg_gemm_w4a8_ldc(fake, fake, fake, 2, 64, 288, 64, Q6_K, 0, None) == -2
    assert so.qg_gemm_w4a8_ldc(fake, P(4099), fake, 2, 64, 256, 64, Q6_K, 0, None) == -4
    assert so.qg_debug_sumi(fake, fake, fake, 1, 1, 288, Q6_K, 0, None) == -2
    assert so.qg_debug_sumi(fake, P(4097), fake, 1, 1, 256, Q6_K, 0, None) == -4
    assert so.qg_dequantize(Q6_K, fake, fake, 288, None) == -2
    assert so.qg_dequantize(Q6_K, None, None, 0, None) == 0
    # the order: K before the alignment, the algorithm after it
    assert so.qg_gemm_w4a8_ex(fake, P(4097), fake, 1, 1, 288, Q6_K, 3, None) == -2
    assert so.qg_gemm_w4a8_ex(fake, P(4097), fake, 1, 1, 256, Q6_K, 3, None) == -4
    # FP32 activations: only through a workspace
    assert so.qg_gemm_w4a8_f32(fake, fake, fake, 2, 64, 512, Q6_K, None, 0, None) == -3
    assert so.qg_gemm_w4a8_f32(fake, fake, fake, 2, 64, 288, Q6_K, fake, 1 << 20, None) == -2
    assert so.qg_gemm_w4a8_f32(fake, P(4097), fake, 2, 64, 512, Q6_K, fake, 1 << 20, None) == -4


def test_weights_two_bytes_off_a_dword_are_taken(so):
    """2-B alignment is all the format guarantees: B at 4n + 2 passes validation (the query entries name a kernel)."""
    buf = ctypes.create_string_buffer(256)
    assert so.qg_debug_config(1, 64, 512, Q6_K, 0, 0, buf, 256) == 0 and buf.value.startswith(b"q6k_gemv ")
    fake = P(4096)
    # an empty call after full validation of a 2-B aligned weights pointer
    assert so.qg_gemm_w4a8(fake, P(4098), fake, 0, 1, 256, Q6_K, None) == 0


def test_layout_entries_refuse_q6k(so):
    """Tiled, repacked, prepacked, padded, _ws, grouped, strided-batched forms and the quantizer: -3, nothing launched."""
    fake = P(4096)
    m, n, k = 2, 64, 512
    assert so.qg_tile_weights(fake, fake, n, k, Q6_K, None) == -3
    assert so.qg_repack_weights(fake, fake, n, k, Q6_K, None) == -3
    assert so.qg_gemm_w4a8_grouped(fake, 1, m, k, Q6_K, None) == -3
    assert so.qg_gemm_w4a8_strided_batched(fake, 0, fake, 0, fake, 0, 1, m, n, k, Q6_K, None) == -3
    assert so.qg_gemm_w4a8_tiled(fake, fake, fake, m, n, k, Q6_K, None) == -3
    assert so.qg_gemm_w4a8_tiled_act(fake, fake, fake, m, n, k, Q6_K, None) == -3
    assert so.qg_quantize(Q6_K, 0, fake, fake, k, None) == -3
    assert so.qg_gemm_w4a8_ws(fake, fake, fake, m, n, k, Q6_K, fake, 1 << 20, None) == -3
    assert so.qg_gemm_w4a8_padded(fake, fake, fake, m, n, k, Q6_K, None) == -3
    assert so.qg_gemm_w4a8_prepacked(fake, fake, fake, m, n, k, Q6_K, fake, 1 << 20, None) == -3
    assert so.qg_tile_weights_bytes(n, k, Q6_K) == 0 and so.qg_repack_weights_bytes(n, k, Q6_K) == 0
    assert so.qg_gemm_w4a8_workspace_size(m, n, k, Q6_K) == 0


def test_routing_and_config(so):
    import quant_gemm as qg
    assert so.qg_select_algo(1, 4096, 4096, Q6_K) == 1 and so.qg_select_algo(8, 4096, 4096, Q6_K) == 1
    assert so.qg_select_algo(9, 4096, 4096, Q6_K) == 2 and so.qg_select_algo(512, 4096, 4096, Q6_K) == 2
    assert so.qg_select_algo(1, 4096, 288, Q6_K) == -1
    for m, fam in ((1, "q6k_gemv "), (8, "q6k_gemv "), (9, "q6k_mmq "), (512, "q6k_mmq ")):
        cfg = qg.debug_config(m, 4096, 4096, Q6_K)
        assert cfg.startswith(fam), cfg
        assert cfg == qg.debug_config(m, 4096, 4096, Q6_K, sumi=True)
    assert qg.debug_config(8, 4096, 4096, Q6_K, algo=2).startswith("q6k_mmq ")
    assert qg.debug_config(4, 4096, 4096, Q6_K, algo=1).startswith("q6k_gemv ")
    with pytest.raises(RuntimeError):
        qg.debug_config(9, 4096, 4096, Q6_K, algo=1)  # the GEMV is M <= 8


def test_routing_at_the_gemv_lds_limit(so):
    """The GEMV's records take M * K/256 * 304 bytes: up to 160 KiB the GEMV, beyond it q6k_mmq even at M <= 8."""
    import quant_gemm as qg
    assert 8 * 67 * 304 <= 160 * 1024 < 8 * 68 * 304
    for m, k, algo, fam in ((8, 256 * 67, 1, "q6k_gemv "), (8, 256 * 68, 2, "q6k_mmq "), (1, 256 * 200, 1, "q6k_gemv ")):
        assert so.qg_select_algo(m, 20, k, Q6_K) == algo, (m, k)
        cfg = qg.debug_config(m, 20, k, Q6_K)
        assert cfg.startswith(fam), cfg
        assert cfg == qg.debug_config(m, 20, k, Q6_K, sumi=True)
        if algo == 1:
            assert f"lds={m * (k // 256) * 304}" in cfg, cfg
    buf = ctypes.create_string_buffer(256)
    assert so.qg_debug_config(8, 20, 256 * 68, Q6_K, 1, 0, buf, 256) == -3  # the forced GEMV is refused
    assert qg.debug_config(8, 20, 256 * 68, Q6_K, algo=2).startswith("q6k_mmq TT=1 RG=1 KS=8 ")


def test_every_instantiation_has_a_shape():
    """The shapes tests/test_gpu_q6k.py runs reach every (MT, LPR, ONE) of q6k_gemv and every (TT, RG) of q6k_mmq
    the dispatch can pick (RG = 4 needs ceil(N/64) * ceil(M/64) >= the device's CUs: 256 when none is visible)."""
    import quant_gemm as qg
    import test_gpu_q6k as T
    seen = set()
    for m, n, k in T.all_product_shapes():
        cfg = qg.debug_config(m, n, k, Q6_K)
        seen.add(" ".join(w for w in cfg.split() if w.split("=")[0] in ("q6k_gemv", "q6k_mmq", "MT", "LPR", "ONE", "TT", "RG")))
    gemv = {f"q6k_gemv MT={mt} LPR={lpr} ONE={one}" for mt in (1, 2, 4, 8) for lpr in (4, 16, 64) for one in (1, 0)}
    # (ONE = 1 is K / 64 <= LPR, one unit per lane: K = 256 at LPR = 4, K = 1024 at LPR = 16, K = 4096 at LPR = 64;
    # every other K of a form runs the unit loop)
    assert len(gemv) == 24 and gemv <= seen, sorted(gemv - seen)
    assert {f"q6k_mmq TT={tt} RG=1" for tt in (1, 2, 4)} | {"q6k_mmq TT=4 RG=4"} <= seen, sorted(seen)


def _visible_cus():
    """None (ask the device) where a GPU is visible, else 256, the library's answer without one."""
    try:
        import torch
        return None if torch.cuda.is_available() else 256
    except ImportError:
        return 256


def test_path_tables_reach_what_their_tests_name():
    """The shape tables of tests/test_gpu_q6k_paths.py against debug_config alone: each shape reaches the instantiation,
    grid and LDS size its GPU test names, and the refusals are refusals."""
    import quant_gemm as qg
    import test_gpu_q6k_paths as T
    rows = T.path_table(qg, _visible_cus())
    assert len(rows) == len(set(rows)) and len(rows) > 70
    for m, n, k, algo, exact, needles in rows:
        cfg = qg.debug_config(m, n, k, Q6_K, algo=algo)
        T.assert_config(cfg, exact, needles)
        assert cfg == qg.debug_config(m, n, k, Q6_K, algo=algo, sumi=True)
    for m, n, k, lds in T.GEMV_LDS_TOP:
        assert lds == m * (k // 256) * 304 <= 160 * 1024 < m * (k // 256 + 1) * 304
    for m, n, k in T.GEMV_LDS_OVER:
        assert qg.select_algo(m, n, k, Q6_K) == 2
        with pytest.raises(RuntimeError, match="unsupported"):
            qg.debug_config(m, n, k, Q6_K, algo=1)
    # the 64 x 64 form against this device's CUs: the extent one tile column short stays in the 16-row form
    m, n, k, _ = T.rg4_shapes(_visible_cus())[0]
    assert " RG=1 " in qg.debug_config(m, n - 64, k, Q6_K)
    # what each loop case is there for: passes of the eight (RG = 1) or two (RG = 4) K slices
    passes = {(m, n, k): -(-(k // 256) // 8) for m, n, k, _ in T.MMQ_RG1_EDGES}
    assert passes[(9, 32, 4096)] == 2 and passes[(31, 33, 2304)] == 2 and passes[(20, 17, 4352)] == 3
    assert [-(-(k // 256) // 2) for k in T.RG4_K] == [2, 2, 3]


def test_path_fuzz_cases_are_seeded_and_reach_the_loops():
    cases = QR.path_fuzz_cases()
    assert cases == QR.path_fuzz_cases() and len(cases) == 24
    assert all(m in QR.PATH_SWEEP_M and 1 <= n <= 300 and k % 256 == 0 and 256 <= k <= 5120 for _, m, n, k, _, _ in cases)
    assert {w for *_, w, _ in cases} == set(QR.W_OFFSETS) and {a for *_, a in cases} == set(QR.A_OFFSETS)
    ms = [m for _, m, *_ in cases]
    assert sum(m <= 8 for m in ms) >= 6 and sum(m >= 9 for m in ms) >= 6
    assert 8 * 20 * 304 <= 160 * 1024  # every M <= 8 case is the GEMV's
    deep = [m for _, m, _, k, _, _ in cases if m >= 9 and k > 2048]  # MFMA cases with a second pass of the K slices
    assert len(deep) >= 3 and any(17 <= m <= 32 for m in deep), deep


# ---------------------------------------------------------------------------- the view entry
def _view(ptr, qtype, k, rows, row_bytes, elem_bytes):
    from quant_gemm import ggml as G
    v = G.TensorView()
    v.data, v.type = ptr, qtype
    v.ne[:] = [k, rows, 1, 1]
    v.nb[:] = [elem_bytes, row_bytes, row_bytes * rows, row_bytes * rows]
    return v


def test_view_of_builds_the_210_byte_view():
    from quant_gemm import ggml as G

    class Dev:
        def data_ptr(self): return 4098
        def numel(self): return 5 * 3 * 210
        def element_size(self): return 1

    v = G.view_of(Dev(), G.Q6_K, 768)
    assert v.type == 14 and list(v.ne) == [768, 5, 1, 1] and list(v.nb[:2]) == [210, 630] and v.data == 4098


def test_view_entry_refusals_for_q6k(so):
    """qg_gemm_w4a8_from_view validates before it touches a pointer: fake pointers, nothing launched."""
    from quant_gemm import ggml as G
    m, n, k = 3, 40, 512

    def call(act=None, w=None, out=None, kernel_type=b"auto", k_act=k, k_w=k):
        act = act or _view(4096, G.Q8_1, k_act, m, k_act // 32 * 36, 36)
        w = w or _view(8192, Q6_K, k_w, n, k_w // 256 * 210, 210)
        out = out or _view(16384, G.F32, n, m, n * 4, 4)
        return so.qg_gemm_w4a8_from_view(ctypes.byref(act), ctypes.byref(w), ctypes.byref(out), kernel_type, None)

    assert call(w=_view(8192, Q6_K, k, n, k // 256 * 210 + 2, 210)) == -3   # rows padded by 2 bytes
    assert call(w=_view(8192, Q6_K, k, n, k // 256 * 144, 144)) == -3       # Q4_K's row stride: not dense Q6_K rows
    assert call(k_act=288, k_w=288) == -2                                   # K % 256 (a multiple of 32)
    assert call(k_w=768) == -1                                              # w.ne[0] != act.ne[0]
    assert call(act=_view(4096, G.F32, k, m, k * 4, 4)) == -3               # activations must be Q8_1
    assert call(kernel_type=b"ragged") == -3 and call(kernel_type=b"generic") == -3
    assert call(kernel_type=b"no such kernel") == -1
    assert call(w=_view(8192 + 1, Q6_K, k, n, k // 256 * 210, 210)) == -4   # weights at an odd address
    assert call(act=_view(4096 + 2, G.Q8_1, k, m, k // 32 * 36, 36)) == -4  # activations off 4 B


# ---------------------------------------------------------------------------- the host twin
@pytest.mark.parametrize("m,n,k", [(1, 1, 256), (3, 37, 768), (9, 20, 2304)])
def test_host_twin_matches_contract(m, n, k):
    """Within tol(w = 0) of the model, and the same bits for 1, 4 and 40 threads."""
    import quant_gemm.host as host
    rng = np.random.default_rng([m, n, k])
    bq, aq = QR.random_q6k(rng, n, k), QR.random_q8_1(rng, m, k)
    c64, _, mag = QR.gemm(aq, bq)
    c1 = host.gemm_w4a8(aq, bq, m, n, k, Q6_K, threads=1)
    err = np.abs(c1.astype(np.float64) - c64)
    assert (err <= QR.tol(mag, k, 0)).all(), (err / QR.tol(mag, k, 0)).max()
    for threads in (4, 40):
        ct = host.gemm_w4a8(aq, bq, m, n, k, Q6_K, threads=threads)
        assert np.array_equal(c1.view(np.uint32), ct.view(np.uint32)), threads


def test_host_twin_extremes_and_bad_k():
    import quant_gemm.host as host
    m, n, k = 3, 16, 512
    aq, bq = QR.extremes(np.random.default_rng(8), m, n, k)
    c64, _, mag = QR.gemm(aq, bq)
    c1 = host.gemm_w4a8(aq, bq, m, n, k, Q6_K, threads=1)
    err = np.abs(c1.astype(np.float64) - c64)
    assert (err <= QR.tol(mag, k, 0)).all(), (err / QR.tol(mag, k, 0)).max()
    assert np.array_equal(c1.view(np.uint32), host.gemm_w4a8(aq, bq, m, n, k, Q6_K, threads=40).view(np.uint32))
    with pytest.raises(RuntimeError):
        host.gemm_w4a8(aq[:, :9], bq[:, :1], m, n, 288, Q6_K)  # K % 256
