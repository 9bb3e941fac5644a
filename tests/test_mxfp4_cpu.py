"""MXFP4 (ggml type 39) without a GPU: the format model (tests/mxfp4_ref.py), the C ABI's static queries, validation and
routing for the type, the GGUF reader, and the host twins against the NumPy contract. No kernel is launched."""
import ctypes

import numpy as np
import pytest

import mxfp4_ref as MR

MXFP4 = 39
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def so():
    import quant_gemm._lib as L
    return L.load()


def _cfg(so, m, n, k, algo=0, sumi=0):
    buf = ctypes.create_string_buffer(256)
    rc = so.qg_debug_config(m, n, k, MXFP4, algo, sumi, buf, 256)
    return rc, buf.value.decode()


# ---------------------------------------------------------------------------- static queries and constants
def test_static_queries(so):
    assert so.qg_block_bytes(MXFP4) == 17 and so.qg_block_elems(MXFP4) == 32
    assert so.qg_block_bytes(38) == 0 and so.qg_block_bytes(40) == 0 and so.qg_block_elems(40) == 0
    import quant_gemm as qg
    import quant_gemm.host as host
    from quant_gemm import ggml as G
    assert qg.MXFP4 == 39 and qg.BLOCK_BYTES[qg.MXFP4] == 17 and qg.block_elems(qg.MXFP4) == 32
    assert qg.MXFP4 in qg.GEMM_WEIGHT_TYPES and qg.MXFP4 not in qg.WEIGHT_TYPES and "MXFP4" in qg.__all__
    assert host.BLOCK_BYTES[39] == 17 and G.MXFP4 == 39


# ---------------------------------------------------------------------------- the model itself
def test_scale_anchors_and_all_256_values():
    bits = MR.scale_bits(np.arange(256))
    assert bits[0] == 0x00200000 and bits[1] == 0x00400000 and bits[2] == 0x00800000 and bits[255] == 0x7F000000
    s = MR.scale(np.arange(256))
    assert s[127] == 0.5 and s[128] == 1.0 and np.isfinite(s).all()
    assert np.array_equal(s.astype(np.float64), 2.0 ** (np.arange(256) - 128.0))
    b = MR.build(np.array([127]), np.arange(32)[None] % 16)
    assert np.array_equal(MR.dequantize(b)[:8], np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], np.float32))


def test_build_codes_round_trip_and_nibble_order():
    rng = np.random.default_rng(2)
    b = MR.random_mxfp4(rng, 3, 96)
    assert np.array_equal(MR.build(b[..., 0], MR.codes(b)), b)
    one = np.zeros((1, 17), np.uint8)
    one[0, 1 + 5] = 0xA3  # element 5 has code 3, element 21 code 10
    c = MR.codes(one)[0]
    assert c[5] == 3 and c[21] == 10 and c.sum() == 13


def _all_codes_all_exponents():
    """256 blocks, block i with e = i and every code twice (rotated by i, so each sits in both nibbles over the set)."""
    e = np.arange(256)
    code = (np.arange(32)[None] + e[:, None]) % 16
    return MR.build(e, code), e, code


def test_host_dequantize_bit_exact_over_codes_and_exponents():
    import quant_gemm.host as host
    b, e, code = _all_codes_all_exponents()
    got = host.dequantize_mxfp4(b).reshape(256, 32)
    exact = MR.KV[code] * 2.0 ** (e[:, None] - 128.0)
    with np.errstate(over="ignore"):  # e >= 253 with the largest codes: beyond fp32, Inf as fp32 gives it
        want = exact.astype(np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    with np.errstate(over="ignore"):
        assert np.array_equal(got.view(np.uint32), MR.dequantize(b).reshape(256, 32).view(np.uint32))
    assert (got.view(np.uint32)[code == 8] == 0).all()  # code 8 is +0.0f, whatever e
    fits = np.abs(exact) < 2.0 ** 128
    assert (got.astype(np.float64)[fits] == exact[fits]).all() and fits[:253].all()  # exact, subnormals kept


def test_gemm_model_against_a_direct_loop():
    rng = np.random.default_rng(5)
    aq, bq = MR.random_q8_1(rng, 2, 96), MR.random_mxfp4(rng, 3, 96)
    c64, sumi, mag = MR.gemm(aq, bq)
    da, _, qa = MR.q8_1_fields(aq)
    kv = MR.KV[MR.codes(bq)]
    for m, n, b in ((0, 0, 0), (1, 2, 2), (1, 1, 1)):
        assert sumi[m, n, b] == int((qa[m, b] * kv[n, b]).sum())
    want = sum(da[1, b] * 2.0 ** (int(bq[2, b, 0]) - 128) * int(sumi[1, 2, b]) for b in range(3))
    assert abs(c64[1, 2] - want) <= 1e-12 * mag[1, 2]


def test_extremes_builder_holds_what_it_claims():
    for lossy in (False, True):
        aq, bq = MR.extremes(np.random.default_rng(6), lossy=lossy)
        assert [int(bq[r, 0, 0]) for r in range(8)] == list(MR.EXTREME_E)
        c = MR.codes(bq)
        assert (c[8] == 0).all() and (c[9] == 8).all() and (c[10] == 7).all() and (c[11] == 15).all()
        assert bq[12, :, 0].min() == 160 and bq[12, :, 0].max() == 200
        da, _, qa = MR.q8_1_fields(aq)
        assert ((da[0] >= 2.0 ** -24) & (da[0] < 2.0 ** -14)).all() and (da[1] == 2.0 ** -14).all()
        assert (da[2] == 1.0).all() and (da[3] == 65504).all() and (qa[2, 0] == -128).all()
        c64, sumi, mag = MR.gemm(aq, bq)
        assert np.isfinite(c64).all() and mag.max() < 2.0 ** 127
        assert sumi[2, 10, 0] == -49152 and sumi[2, 11, 0] == 49152 and np.abs(sumi).max() == 49152 < 2 ** 24
        assert (c64[:, 8] == 0).all() and (c64[:, 9] == 0).all()
        # the subnormal allowance is confined to the rows of e <= 3, and to d_a <= 1 there
        slack = MR.subnormal_slack(aq, bq)
        assert (slack[3] == 0).all() and (slack[:, 4:] == 0).all() and (slack[0, :4] > 0).all() and (slack[2, :2] > 0).all()
        assert (MR.lossy_scale_slack(aq, bq)[0, :3] > 0).all() == lossy
        assert (MR.lossy_scale_slack(aq, bq)[1:] == 0).all()


def test_fuzz_cases_are_seeded_and_cover_both_families():
    cases = MR.fuzz_cases()
    assert cases == MR.fuzz_cases() and len(cases) == 16
    assert all(m in MR.SWEEP_M and 1 <= n <= 200 and k % 32 == 0 and 32 <= k <= 3072 for _, m, n, k, _, _ in cases)
    assert {w for *_, w, _ in cases} == set(MR.W_OFFSETS) and {a for *_, a in cases} == set(MR.A_OFFSETS)
    ms = [m for _, m, *_ in cases]
    assert sum(m <= 8 for m in ms) >= 5 and sum(m > 8 for m in ms) >= 5


def test_quantizer_picks_the_nearest_table_value():
    x = np.array([[0.0, 0.5, -0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -6.0, 5.1, 0.2] + [0.0] * 20])
    b = MR.quantize(x)
    assert b[0, 0, 0] == 127  # amax = 6 = 12 * 2^-1
    y = MR.dequantize(b)[0]
    assert np.array_equal(y[:12], np.array([0, 0.5, -0.5, 1, 1.5, 2, 3, 4, 6, -6, 6, 0], np.float32))
    assert np.array_equal(MR.dequantize(MR.quantize(np.zeros((1, 32))))[0], np.zeros(32, np.float32))


# ---------------------------------------------------------------------------- the C ABI
def test_validation_codes_without_launch(so):
    fake = P(4096)  # never dereferenced: validation fails first
    for k in (48, 0, -32, 16):
        assert so.qg_gemm_w4a8(fake, fake, fake, 1, 1, k, MXFP4, None) == -2, k          # K % 32
    assert so.qg_gemm_w4a8(P(4098), fake, fake, 1, 1, 32, MXFP4, None) == -4             # activations off 4 B
    assert so.qg_gemm_w4a8_ex(fake, fake, fake, 1, 1, 32, MXFP4, 3, None) == -3          # generic
    assert so.qg_gemm_w4a8_ex(fake, fake, fake, 1, 1, 32, MXFP4, 4, None) == -3          # ragged
    assert so.qg_gemm_w4a8(None, None, None, 0, 5, 32, MXFP4, None) == 0                 # M = 0: no-op
    assert so.qg_gemm_w4a8(None, None, None, 5, 0, 32, MXFP4, None) == 0                 # N = 0: no-op
    assert so.qg_gemm_w4a8(fake, fake, fake, -1, 1, 32, MXFP4, None) == -1
    assert so.qg_gemm_w4a8(None, fake, fake, 1, 1, 32, MXFP4, None) == -1
    assert so.qg_gemm_w4a8_ldc(fake, fake, fake, 2, 64, 48, 64, MXFP4, 0, None) == -2
    assert so.qg_gemm_w4a8_ldc(P(4097), fake, fake, 2, 64, 32, 64, MXFP4, 0, None) == -4
    assert so.qg_debug_sumi(fake, fake, fake, 1, 1, 48, MXFP4, 0, None) == -2
    assert so.qg_debug_sumi(P(4098), fake, fake, 1, 1, 32, MXFP4, 0, None) == -4
    assert so.qg_dequantize(MXFP4, fake, fake, 48, None) == -2
    assert so.qg_dequantize(MXFP4, None, None, 0, None) == 0
    # the order: K before the alignment, the algorithm after it
    assert so.qg_gemm_w4a8_ex(P(4098), fake, fake, 1, 1, 48, MXFP4, 3, None) == -2
    assert so.qg_gemm_w4a8_ex(P(4098), fake, fake, 1, 1, 32, MXFP4, 3, None) == -4
    # FP32 activations: only through a workspace
    assert so.qg_gemm_w4a8_f32(fake, fake, fake, 2, 64, 64, MXFP4, None, 0, None) == -3
    assert so.qg_gemm_w4a8_f32(fake, fake, fake, 2, 64, 48, MXFP4, fake, 1 << 20, None) == -2
    assert so.qg_gemm_w4a8_f32(P(4098), fake, fake, 2, 64, 64, MXFP4, fake, 1 << 20, None) == -4


def test_weights_at_any_byte_are_taken(so):
    """B has no alignment requirement: at every offset in a dword an empty call passes full validation, where an
    activation pointer off 4 B does not; the launch-free query names a kernel."""
    fake = P(4096)
    for off in (1, 2, 3):
        assert so.qg_gemm_w4a8(fake, P(4096 + off), fake, 0, 1, 32, MXFP4, None) == 0
        assert so.qg_gemm_w4a8_ldc(fake, P(4096 + off), fake, 0, 64, 32, 64, MXFP4, 0, None) == 0
        assert so.qg_debug_sumi(fake, P(4096 + off), fake, 0, 1, 32, MXFP4, 0, None) == 0
        assert so.qg_gemm_w4a8_moe(fake, 1, P(4096 + off), 4, fake, 2, fake, 0, 0, 2, 64, 96, MXFP4, None) == 0
    assert so.qg_gemm_w4a8(P(4098), P(4097), fake, 0, 1, 32, MXFP4, None) == 0  # (an empty call checks no pointer)
    rc, cfg = _cfg(so, 1, 64, 96)
    assert rc == 0 and cfg.startswith("mxfp4_gemv ")


def test_layout_entries_refuse_mxfp4(so):
    """Tiled, repacked, prepacked, padded, _ws, grouped, strided-batched and weight-major forms, the quantizer and the
    four other expert entries: -3, nothing launched."""
    fake = P(4096)
    m, n, k = 2, 64, 512
    assert so.qg_tile_weights(fake, fake, n, k, MXFP4, None) == -3
    assert so.qg_repack_weights(fake, fake, n, k, MXFP4, None) == -3
    assert so.qg_gemm_w4a8_grouped(fake, 1, m, k, MXFP4, None) == -3
    assert so.qg_gemm_w4a8_strided_batched(fake, 0, fake, 0, fake, 0, 1, m, n, k, MXFP4, None) == -3
    assert so.qg_gemm_w4a8_tiled(fake, fake, fake, m, n, k, MXFP4, None) == -3
    assert so.qg_gemm_w4a8_tiled_act(fake, fake, fake, m, n, k, MXFP4, None) == -3
    assert so.qg_quantize(MXFP4, 0, fake, fake, k, None) == -3
    assert so.qg_gemm_w4a8_ws(fake, fake, fake, m, n, k, MXFP4, fake, 1 << 20, None) == -3
    assert so.qg_gemm_w4a8_padded(fake, fake, fake, m, n, k, MXFP4, None) == -3
    assert so.qg_gemm_w4a8_prepacked(fake, fake, fake, m, n, k, MXFP4, fake, 1 << 20, None) == -3
    assert so.qg_tile_weights_bytes(n, k, MXFP4) == 0 and so.qg_repack_weights_bytes(n, k, MXFP4) == 0
    assert so.qg_gemm_w4a8_workspace_size(m, n, k, MXFP4) == 0
    t, u, ne = 2, 2, 4
    big = 1 << 24
    assert so.qg_gemm_w4a8_moe_prefill(fake, 1, fake, ne, fake, u, fake, 0, t, u, n, k, MXFP4, fake, big, None) == -3
    assert so.qg_gemm_w4a8_moe_batch(fake, 1, fake, ne, fake, u, fake, 0, t, u, n, k, MXFP4, fake, big, None) == -3
    assert so.qg_gemm_w4a8_moe_glu(fake, fake, fake, ne, fake, u, fake, 0, t, u, n, k, MXFP4, 2, None) == -3
    assert so.qg_gemm_w4a8_moe_down(fake, fake, ne, fake, u, None, u, fake, 0, t, u, n, k, MXFP4, None) == -3
    buf = ctypes.create_string_buffer(256)
    assert so.qg_moe_prefill_config(t, u, ne, n, k, MXFP4, buf, 256) == -3
    assert so.qg_moe_batch_config(t, u, ne, n, k, MXFP4, buf, 256) == -3
    assert so.qg_moe_glu_config(t, u, n, k, MXFP4, buf, 256) == -3
    assert so.qg_moe_down_config(t, u, n, k, MXFP4, buf, 256) == -3


GEMV_MAX_M = 8  # AUTO's threshold: the decode GEMV up to here, the MFMA prefill beyond


def test_routing_and_config(so):
    import quant_gemm as qg
    for m in (1, 5, GEMV_MAX_M):
        assert so.qg_select_algo(m, 4096, 4096, MXFP4) == 1
        assert qg.debug_config(m, 4096, 4096, MXFP4).startswith("mxfp4_gemv ")
    for m in (GEMV_MAX_M + 1, 512):
        assert so.qg_select_algo(m, 4096, 4096, MXFP4) == 2
        assert qg.debug_config(m, 4096, 4096, MXFP4).startswith("mxfp4_mmq ")
    assert so.qg_select_algo(1, 4096, 48, MXFP4) == -1
    for m in (1, 8, 9, 512):
        assert qg.debug_config(m, 4096, 4096, MXFP4) == qg.debug_config(m, 4096, 4096, MXFP4, sumi=True)
    assert qg.debug_config(8, 4096, 4096, MXFP4, algo=2).startswith("mxfp4_mmq TT=1 RG=1 KS=8 ")
    assert qg.debug_config(1, 4096, 4096, MXFP4, algo=2).startswith("mxfp4_mmq TT=1 ")
    assert qg.debug_config(4, 4096, 4096, MXFP4, algo=1).startswith("mxfp4_gemv MT=4 ")
    with pytest.raises(RuntimeError):
        qg.debug_config(9, 4096, 4096, MXFP4, algo=1)  # the GEMV is M <= 8
    assert qg.debug_config(17, 40, 96, MXFP4).startswith("mxfp4_mmq TT=2 RG=1 ")
    assert qg.debug_config(65, 40, 96, MXFP4).startswith("mxfp4_mmq TT=4 RG=1 ")


def test_routing_at_the_gemv_lds_limit(so):
    """The GEMV's records take M * K/32 * 48 bytes: up to 160 KiB the GEMV, beyond it mxfp4_mmq even at small M."""
    import quant_gemm as qg
    assert 8 * 426 * 48 <= 160 * 1024 < 8 * 427 * 48 and 1 * 3413 * 48 <= 160 * 1024 < 1 * 3414 * 48
    for m, nb, algo, fam in ((8, 426, 1, "mxfp4_gemv "), (8, 427, 2, "mxfp4_mmq "), (1, 3413, 1, "mxfp4_gemv "),
                             (1, 3414, 2, "mxfp4_mmq "), (2, 2000, 2, "mxfp4_mmq ")):
        k = 32 * nb
        assert so.qg_select_algo(m, 20, k, MXFP4) == algo, (m, k)
        cfg = qg.debug_config(m, 20, k, MXFP4)
        assert cfg.startswith(fam), cfg
        if algo == 1:
            assert f"lds={m * nb * 48}" in cfg, cfg
    assert _cfg(so, 8, 20, 32 * 427, algo=1)[0] == -3  # the forced GEMV is refused


@pytest.mark.parametrize("nb,lpr,wgs,one", [(1, 4, 256, 1), (3, 4, 256, 1), (4, 4, 256, 1), (5, 4, 256, 0), (15, 4, 256, 0),
                                            (16, 16, 512, 1), (17, 16, 512, 0), (63, 16, 512, 0), (64, 64, 1024, 1),
                                            (90, 64, 1024, 0), (91, 64, 1024, 0), (128, 64, 1024, 0), (448, 64, 1024, 0)])
def test_gemv_instantiation_ladder(nb, lpr, wgs, one):
    """Lanes per row, workgroup size and the loop-free form by K / 32: 4 lanes below 16 blocks, 16 below 64, a wave from
    64 on; ONE where no lane owns a second block. MT is the smallest of 1, 2, 4, 8 that holds M."""
    import quant_gemm as qg
    n = 67
    rpb = (wgs // 64) * (64 // lpr)
    for m, mt in ((1, 1), (2, 2), (3, 4), (5, 8), (8, 8)):
        if m * nb * 48 > 160 * 1024:
            continue
        want = f"mxfp4_gemv MT={mt} LPR={lpr} WGS={wgs} ONE={one} grid={-(-n // rpb)} lds={m * nb * 48}"
        assert qg.debug_config(m, n, 32 * nb, MXFP4) == want


def test_moe_config_names_the_single_calls_form(so):
    import quant_gemm as qg
    for n, k in ((67, 96), (200, 2880), (67, 2912), (2880, 2880), (64, 512)):
        single = dict(w.split("=") for w in qg.debug_config(1, n, k, MXFP4).split()[1:])
        cfg = qg.moe_config(3, 4, n, k, MXFP4)
        assert cfg.startswith("moe:mxfp4_gemv "), cfg
        got = dict(w.split("=") for w in cfg.split()[1:])
        assert all(got[key] == single[key] for key in ("LPR", "WGS", "ONE", "lds")), (cfg, single)
        assert got["grid"] == f"{single['grid']}x12"
    buf = ctypes.create_string_buffer(256)
    assert so.qg_moe_config(1, 4, 64, 32 * 3414, MXFP4, buf, 256) == -3  # records of one row beyond the LDS
    assert so.qg_moe_config(1, 4, 64, 48, MXFP4, buf, 256) == -2
    fake = P(4096)
    assert so.qg_gemm_w4a8_moe(P(4098), 1, fake, 4, fake, 2, fake, 0, 1, 2, 64, 96, MXFP4, None) == -4  # A off 4 B
    assert so.qg_gemm_w4a8_moe(fake, 1, fake, 4, P(4098), 2, fake, 0, 1, 2, 64, 96, MXFP4, None) == -4  # ids off 4 B
    assert so.qg_gemm_w4a8_moe(fake, 3, fake, 4, fake, 2, fake, 0, 1, 2, 64, 96, MXFP4, None) == -1    # a_rows


# ---------------------------------------------------------------------------- the view entries
def _view(ptr, qtype, k, rows, row_bytes, elem_bytes):
    from quant_gemm import ggml as G
    v = G.TensorView()
    v.data, v.type = ptr, qtype
    v.ne[:] = [k, rows, 1, 1]
    v.nb[:] = [elem_bytes, row_bytes, row_bytes * rows, row_bytes * rows]
    return v


def test_view_of_builds_the_17_byte_view():
    from quant_gemm import ggml as G

    class Dev:
        def data_ptr(self): return 4099
        def numel(self): return 5 * 3 * 17
        def element_size(self): return 1

    v = G.view_of(Dev(), G.MXFP4, 96)
    assert v.type == 39 and list(v.ne) == [96, 5, 1, 1] and list(v.nb[:2]) == [17, 51] and v.data == 4099


def test_view_entry_refusals_for_mxfp4(so):
    """qg_gemm_w4a8_from_view validates before it touches a pointer: fake pointers, nothing launched."""
    from quant_gemm import ggml as G
    m, n, k = 3, 40, 96

    def call(act=None, w=None, out=None, kernel_type=b"auto", k_act=k, k_w=k):
        act = act or _view(4096, G.Q8_1, k_act, m, k_act // 32 * 36, 36)
        w = w or _view(8192, MXFP4, k_w, n, k_w // 32 * 17, 17)
        out = out or _view(16384, G.F32, n, m, n * 4, 4)
        return so.qg_gemm_w4a8_from_view(ctypes.byref(act), ctypes.byref(w), ctypes.byref(out), kernel_type, None)

    assert call(w=_view(8192, MXFP4, k, n, k // 32 * 17 + 1, 17)) == -3     # rows padded by a byte
    assert call(w=_view(8192, MXFP4, k, n, k // 32 * 18, 18)) == -3         # Q4_0's row stride: not dense MXFP4 rows
    assert call(k_act=48, k_w=48) == -2
    assert call(k_w=128) == -1                                              # w.ne[0] != act.ne[0]
    assert call(act=_view(4096, G.F32, k, m, k * 4, 4)) == -3               # activations must be Q8_1
    assert call(kernel_type=b"ragged") == -3 and call(kernel_type=b"generic") == -3
    assert call(act=_view(4096 + 2, G.Q8_1, k, m, k // 32 * 36, 36)) == -4  # activations off 4 B


# ---------------------------------------------------------------------------- GGUF
def test_gguf_reads_a_type_39_tensor(tmp_path):
    from gguf_writer import write_gguf
    from quant_gemm import ggml as G
    rng = np.random.default_rng(9)
    b = MR.random_mxfp4(rng, 3, 64)  # ne = [64, 3]: 3 rows of 2 blocks, 102 bytes
    p = tmp_path / "m.gguf"
    write_gguf(p, [], [("blk.0.ffn_down_exps.weight", 39, [64, 3], b.tobytes()), ("q6k", 14, [256, 2], b"\0" * 420)])
    with G.GGUFFile(p) as f:
        t = f.tensors["blk.0.ffn_down_exps.weight"]
        assert t.type == 39 and t.nbytes == 3 * 2 * 17 and t.shape == (3, 2, 17)
        assert np.array_equal(f.host_bytes("blk.0.ffn_down_exps.weight"), b)

        class Dev:
            def data_ptr(self): return 4097

        v = f.view("blk.0.ffn_down_exps.weight", Dev())
        assert v.type == 39 and list(v.ne) == [64, 3, 1, 1] and list(v.nb)[:2] == [17, 34] and v.data == 4097
        assert f.tensors["q6k"].nbytes == 0  # type 14 stays listed, not readable
    bad = tmp_path / "bad.gguf"
    write_gguf(bad, [], [("w", 39, [48, 3], b"\0" * 102)])
    with pytest.raises(RuntimeError):
        G.GGUFFile(bad)


# ---------------------------------------------------------------------------- the host twins
@pytest.mark.parametrize("m,n,k", [(1, 1, 32), (3, 5, 96), (2, 7, 2912)])
def test_host_twin_matches_contract(m, n, k):
    """Within tol(w = 0) of the model, and the same bits for 1, 3 and 16 threads."""
    import quant_gemm.host as host
    rng = np.random.default_rng([m, n, k])
    bq, aq = MR.random_mxfp4(rng, n, k), MR.random_q8_1(rng, m, k)
    c64, _, mag = MR.gemm(aq, bq)
    c1 = host.gemm_w4a8(aq, bq, m, n, k, MXFP4, threads=1)
    err = np.abs(c1.astype(np.float64) - c64)
    assert (err <= MR.tol(mag, k, 0)).all(), (err / MR.tol(mag, k, 0)).max()
    for threads in (3, 16):
        ct = host.gemm_w4a8(aq, bq, m, n, k, MXFP4, threads=threads)
        assert np.array_equal(c1.view(np.uint32), ct.view(np.uint32)), threads
    with pytest.raises(RuntimeError):
        host.gemm_w4a8(aq, bq, m, n, k + 16, MXFP4)


def test_host_twin_extremes():
    """The contract's bound at the ends of both scale formats, the 2^-149 per term only where a term or d_a * scale(e)
    is subnormal; no Inf, no NaN."""
    import quant_gemm.host as host
    n, k = 16, 512
    aq, bq = MR.extremes(np.random.default_rng(8), n, k)
    c64, _, mag = MR.gemm(aq, bq)
    assert mag.max() < 2.0 ** 127
    c1 = host.gemm_w4a8(aq, bq, 4, n, k, MXFP4, threads=1)
    assert np.isfinite(c1).all()
    err = np.abs(c1.astype(np.float64) - c64)
    assert (err <= MR.tol(mag, k, 0)).all(), (err / MR.tol(mag, k, 0)).max()
    # and the contract's own statement, without tol()'s 1e-30 floor: these subnormals cost at most 2^-149 per term
    bound = MR.contract_bound(aq, bq, 0)
    assert (err <= bound).all(), (err[err > bound], bound[err > bound])
    assert np.array_equal(c1.view(np.uint32), host.gemm_w4a8(aq, bq, 4, n, k, MXFP4, threads=16).view(np.uint32))


def test_host_twin_where_the_scale_product_is_no_fp32_number():
    """d_a * scale(e) below 2^-149's grid (a subnormal d_a such as 3 * 2^-24 against e <= 2): the contract's order
    rounds that product first, so the term is off by up to 2^-150 |sumi|, far more than 2^-149. The bound that holds
    is lossy_scale_slack's, from the formats alone; DESIGN.md 3h says what this means for the contract's wording."""
    import quant_gemm.host as host
    n, k = 16, 512
    aq, bq = MR.extremes(np.random.default_rng(8), n, k, lossy=True)
    c64, _, mag = MR.gemm(aq, bq)
    c1 = host.gemm_w4a8(aq, bq, 4, n, k, MXFP4, threads=1)
    err = np.abs(c1.astype(np.float64) - c64)
    assert (err <= MR.tol(mag, k, 0)).all()  # tol()'s 1e-30 floor covers all of this
    narrow = MR.contract_bound(aq, bq, 0)
    bound = narrow + MR.lossy_scale_slack(aq, bq)
    assert (err <= bound).all(), (err[err > bound], bound[err > bound])
    assert (err[0, :3] > narrow[0, :3]).any()  # the 2^-149 per term does not cover these outputs
    assert (err[1:] <= narrow[1:]).all() and (err[:, 3:] <= narrow[:, 3:]).all()


def test_host_moe_twin_is_the_per_slot_product():
    import quant_gemm.host as host
    rng = np.random.default_rng(11)
    t, u, ne, n, k = 3, 2, 4, 7, 96
    experts = MR.random_mxfp4(rng, ne * n, k).reshape(ne, n, k // 32, 17)
    ids = np.array([[0, 3], [-1, 2], [4, 1]], np.int32)  # -1 and n_expert name no expert
    for a_rows in (1, u):
        aq = MR.random_q8_1(rng, t * a_rows, k).reshape(t, a_rows, k // 32, 36)
        c = host.gemm_w4a8_moe(aq, experts, ids, t, u, n, k, MXFP4, a_rows=a_rows, threads=3)
        for ti in range(t):
            for ui in range(u):
                e = int(ids[ti, ui])
                if 0 <= e < ne:
                    want = host.gemm_w4a8(aq[ti, ui % a_rows][None], experts[e], 1, n, k, MXFP4)[0]
                else:
                    want = np.zeros(n, np.float32)
                assert np.array_equal(c[ti, ui].view(np.uint32), want.view(np.uint32)), (a_rows, ti, ui)
