"""Q4_K (ggml type 12) without a GPU: the format model, the C-ABI's validation and routing for the type, the host
twin against the NumPy contract (tests/kquant_ref.py), and the GGUF reader. No kernel is launched."""
import ctypes

import numpy as np
import pytest

import kquant_ref as KR
from gguf_writer import as_bytes, write_gguf

Q4_K = 12
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def so():
    import quant_gemm._lib as L
    return L.load()


def test_scale_pack_unpack_round_trip():
    """All 64 x 64 (sc, m) values, in the low half (j < 4) and in the high half (j >= 4) of the 12 bytes."""
    v = np.arange(64)
    sc, m = [a.reshape(-1) for a in np.meshgrid(v, v, indexing="ij")]
    for half in (0, 4):
        scs = np.zeros((sc.size, 8), np.uint8)
        ms = np.zeros((sc.size, 8), np.uint8)
        for j in range(4):  # each position of the half takes the pair, rotated so positions differ
            scs[:, half + j] = np.roll(sc, j)
            ms[:, half + j] = np.roll(m, 3 * j)
        # the other half holds the complement pattern, so cross-talk between the halves would show
        scs[:, 4 - half:8 - half] = 63 - scs[:, half:half + 4]
        ms[:, 4 - half:8 - half] = 63 - ms[:, half:half + 4]
        q = KR.pack_scales(scs, ms)
        assert q.shape == (sc.size, 12) and q.dtype == np.uint8
        sc2, m2 = KR.unpack_scales(q)
        assert np.array_equal(sc2, scs) and np.array_equal(m2, ms)


def test_unpack_matches_dword_formulas():
    """The dword form of the unpacking (what the kernels use) equals the per-byte definition."""
    rng = np.random.default_rng(1)
    q = rng.integers(0, 256, (1000, 12), dtype=np.uint8)
    u = q.view("<u4").astype(np.uint64)
    u0, u1, u2 = u[:, 0], u[:, 1], u[:, 2]
    parts = [u0 & 0x3F3F3F3F, (u2 & 0x0F0F0F0F) | ((u0 >> 2) & 0x30303030),
             u1 & 0x3F3F3F3F, ((u2 >> 4) & 0x0F0F0F0F) | ((u1 >> 2) & 0x30303030)]
    by = lambda x: np.stack([(x >> (8 * i)) & 0xFF for i in range(4)], -1).astype(np.int32)
    sc, m = KR.unpack_scales(q)
    assert np.array_equal(np.concatenate([by(parts[0]), by(parts[1])], -1), sc)
    assert np.array_equal(np.concatenate([by(parts[2]), by(parts[3])], -1), m)


def test_static_queries(so):
    assert so.qg_block_bytes(Q4_K) == 144
    assert [so.qg_block_elems(t) for t in (2, 9, 12, 0)] == [32, 32, 256, 0]
    import quant_gemm as qg
    assert qg.Q4_K == 12 and qg.BLOCK_BYTES[qg.Q4_K] == 144 and qg.block_elems(qg.Q4_K) == 256


def test_validation_codes_without_launch(so):
    fake = P(4096)  # never dereferenced: validation fails first
    assert so.qg_gemm_w4a8(fake, fake, fake, 1, 1, 288, Q4_K, None) == -2            # K % 256
    assert so.qg_gemm_w4a8(fake, fake, fake, 1, 1, 0, Q4_K, None) == -2
    assert so.qg_gemm_w4a8(fake, P(4096 + 4), fake, 1, 1, 256, Q4_K, None) == -4     # weights at 16n + 4
    assert so.qg_gemm_w4a8(P(4098), fake, fake, 1, 1, 256, Q4_K, None) == -4         # activations off 4 B
    assert so.qg_gemm_w4a8_ex(fake, fake, fake, 1, 1, 256, Q4_K, 3, None) == -3      # generic
    assert so.qg_gemm_w4a8_ex(fake, fake, fake, 1, 1, 256, Q4_K, 4, None) == -3      # ragged
    assert so.qg_gemm_w4a8(None, None, None, 0, 5, 256, Q4_K, None) == 0             # M = 0: no-op
    assert so.qg_gemm_w4a8_ldc(fake, fake, fake, 2, 64, 288, 64, Q4_K, 0, None) == -2
    assert so.qg_debug_sumi(fake, fake, fake, 1, 1, 288, Q4_K, 0, None) == -2
    assert so.qg_dequantize(Q4_K, fake, fake, 288, None) == -2


def test_layout_entries_refuse_q4k(so):
    """Tiled, repacked, grouped, strided-batched forms and the quantizer have no Q4_K: -3, nothing launched."""
    fake = P(4096)
    m, n, k = 2, 64, 512
    assert so.qg_tile_weights(fake, fake, n, k, Q4_K, None) == -3
    assert so.qg_repack_weights(fake, fake, n, k, Q4_K, None) == -3
    assert so.qg_gemm_w4a8_grouped(fake, 1, m, k, Q4_K, None) == -3
    assert so.qg_gemm_w4a8_strided_batched(fake, 0, fake, 0, fake, 0, 1, m, n, k, Q4_K, None) == -3
    assert so.qg_gemm_w4a8_tiled(fake, fake, fake, m, n, k, Q4_K, None) == -3
    assert so.qg_quantize(Q4_K, 0, fake, fake, k, None) == -3
    assert so.qg_gemm_w4a8_f32(fake, fake, fake, m, n, k, Q4_K, None, 0, None) == -3  # no workspace
    assert so.qg_gemm_w4a8_ws(fake, fake, fake, m, n, k, Q4_K, fake, 1 << 20, None) == -3
    assert so.qg_gemm_w4a8_padded(fake, fake, fake, m, n, k, Q4_K, None) == -3
    assert so.qg_gemm_w4a8_prepacked(fake, fake, fake, m, n, k, Q4_K, fake, 1 << 20, None) == -3
    assert so.qg_tile_weights_bytes(n, k, Q4_K) == 0 and so.qg_repack_weights_bytes(n, k, Q4_K) == 0


def test_routing_and_config(so):
    import quant_gemm as qg
    assert so.qg_select_algo(1, 4096, 4096, Q4_K) == 1 and so.qg_select_algo(8, 4096, 4096, Q4_K) == 1
    assert so.qg_select_algo(9, 4096, 4096, Q4_K) == 2 and so.qg_select_algo(512, 4096, 4096, Q4_K) == 2
    assert so.qg_select_algo(1, 4096, 288, Q4_K) == -1
    for m, fam in ((1, "q4k_gemv "), (8, "q4k_gemv "), (9, "q4k_mmq "), (512, "q4k_mmq ")):
        cfg = qg.debug_config(m, 4096, 4096, Q4_K)
        assert cfg.startswith(fam), cfg
        assert cfg == qg.debug_config(m, 4096, 4096, Q4_K, sumi=True)
    # both families can be forced across the threshold
    assert qg.debug_config(8, 4096, 4096, Q4_K, algo=2).startswith("q4k_mmq ")
    assert qg.debug_config(4, 4096, 4096, Q4_K, algo=1).startswith("q4k_gemv ")
    with pytest.raises(RuntimeError):
        qg.debug_config(9, 4096, 4096, Q4_K, algo=1)  # the GEMV is M <= 8


def test_host_twin_matches_contract():
    import quant_gemm.host as host
    m, n, k = 3, 37, 768
    rng = np.random.default_rng(12)
    bq, aq = KR.random_q4k(rng, n, k), KR.random_q8_1(rng, m, k)
    c64, _, mag = KR.gemm(aq, bq)
    c1 = host.gemm_w4a8(aq, bq, m, n, k, Q4_K, threads=1)
    c4 = host.gemm_w4a8(aq, bq, m, n, k, Q4_K, threads=4)
    err = np.abs(c1.astype(np.float64) - c64)
    assert (err <= KR.tol(mag, k, 0)).all(), (err / KR.tol(mag, k, 0)).max()
    assert np.array_equal(c1.view(np.uint32), c4.view(np.uint32))
    with pytest.raises(RuntimeError):
        host.gemm_w4a8(aq[:, :9], bq[:, :1], m, n, 288, Q4_K)  # K % 256


def test_dequant_model_is_consistent():
    """fields / build are inverses and dequant follows the definition (guards the reference itself)."""
    rng = np.random.default_rng(3)
    b = KR.random_q4k(rng, 2, 512)
    d, dmin, sc, m, q = KR.fields(b)
    assert np.array_equal(KR.build(d, dmin, sc, m, q), b)
    y = KR.dequant(b).reshape(2, 2, 8, 32)
    e = (1, 1, 5, 7)  # element 7 of sub-block 5: the high nibble of qs[32 * 2 + 7]
    qv = b[1, 1, 16 + 64 + 7] >> 4
    want = np.float32(np.float32(d[1, 1] * np.float32(sc[1, 1, 5])) * np.float32(qv)) - np.float32(
        dmin[1, 1] * np.float32(m[1, 1, 5]))
    assert y[e] == want


def test_gguf_q4k_tensor(tmp_path):
    from quant_gemm import ggml as G
    rng = np.random.default_rng(5)
    w = KR.random_q4k(rng, 3, 512)
    path = str(tmp_path / "q4k.gguf")
    write_gguf(path, [], [("w", Q4_K, [512, 3], as_bytes(w))])
    with G.GGUFFile(path) as f:
        t = f.tensors["w"]
        assert t.type == Q4_K and t.nbytes == 3 * 2 * 144
        assert t.shape == (3, 2, 144)
        assert np.array_equal(f.host_bytes("w"), w)

        class Dev:  # stands in for an uploaded tensor: the view only takes its pointer
            def data_ptr(self):
                return 4096

        v = f.view("w", Dev())
        assert list(v.nb[:2]) == [144, 288] and list(v.ne[:2]) == [512, 3] and v.type == Q4_K
    bad = str(tmp_path / "bad.gguf")
    write_gguf(bad, [], [("w", Q4_K, [288, 2], b"\0" * 288)])
    with pytest.raises(RuntimeError):
        G.GGUFFile(bad)


# ---------------------------------------------------------------------------- routing at the LDS and grid boundaries
def test_routing_at_the_gemv_lds_limit(so):
    """The GEMV's records take M * K/256 * 336 bytes: up to 160 KiB the GEMV, beyond it q4k_mmq even at M <= 8."""
    import quant_gemm as qg
    assert 8 * 60 * 336 <= 160 * 1024 < 8 * 61 * 336 and 5 * 98 * 336 > 160 * 1024
    for m, k, algo, fam in ((8, 15360, 1, "q4k_gemv "), (8, 15616, 2, "q4k_mmq "), (5, 25088, 2, "q4k_mmq "),
                            (5, 24832, 1, "q4k_gemv "), (1, 25088, 1, "q4k_gemv ")):
        assert so.qg_select_algo(m, 20, k, Q4_K) == algo, (m, k)
        cfg = qg.debug_config(m, 20, k, Q4_K)
        assert cfg.startswith(fam), cfg
        assert cfg == qg.debug_config(m, 20, k, Q4_K, sumi=True)
        if algo == 1:
            assert f"lds={m * (k // 256) * 336}" in cfg, cfg
    buf = ctypes.create_string_buffer(256)
    for m, k in ((8, 15616), (5, 25088)):
        assert so.qg_debug_config(m, 20, k, Q4_K, 1, 0, buf, 256) == -3  # the forced GEMV is refused
        assert so.qg_debug_config(m, 20, k, Q4_K, 1, 1, buf, 256) == -3
        with pytest.raises(RuntimeError, match="unsupported"):
            qg.debug_config(m, 20, k, Q4_K, algo=1)
        assert qg.debug_config(m, 20, k, Q4_K, algo=2).startswith("q4k_mmq TT=1 RG=1 KS=8 ")


def test_mmq_tile_choice(so):
    """TT follows M (16 | 17 and 32 | 33); 64 x 64 tiles (RG = 4, two K slices) once ceil(N/64) * ceil(M/64) fills
    the CUs (256 when no device is visible, and on a whole MI355X)."""
    import quant_gemm as qg
    for m, tt in ((16, 1), (17, 2), (32, 2), (33, 4)):
        assert qg.debug_config(m, 64, 512, Q4_K).startswith(f"q4k_mmq TT={tt} RG=1 KS=8 "), m
    assert qg.debug_config(512, 4096, 4096, Q4_K) == "q4k_mmq TT=4 RG=4 KS=2 grid=64x8"
    assert qg.debug_config(64, 4096, 4096, Q4_K) == "q4k_mmq TT=4 RG=1 KS=8 grid=256x1"


# ---------------------------------------------------------------------------- the host twin
@pytest.mark.parametrize("k", [256, 2304])
@pytest.mark.parametrize("n", [1, 37])
@pytest.mark.parametrize("m", [1, 8, 9])
def test_host_twin_shapes(m, n, k):
    """Within KR.tol(mag, K, 0), and the same bits for 1, 3, N + 5 and 64 threads (more threads than rows)."""
    import quant_gemm.host as host
    rng = np.random.default_rng([m, n, k])
    bq, aq = KR.random_q4k(rng, n, k), KR.random_q8_1(rng, m, k)
    c64, _, mag = KR.gemm(aq, bq)
    c1 = host.gemm_w4a8(aq, bq, m, n, k, Q4_K, threads=1)
    err = np.abs(c1.astype(np.float64) - c64)
    assert (err <= KR.tol(mag, k, 0)).all(), (err / KR.tol(mag, k, 0)).max()
    for threads in (3, n + 5, 64):
        ct = host.gemm_w4a8(aq, bq, m, n, k, Q4_K, threads=threads)
        assert np.array_equal(c1.view(np.uint32), ct.view(np.uint32)), threads


@pytest.mark.parametrize("m", [2, 12])
def test_host_twin_scale_extremes(m):
    """f16 subnormals, the smallest normal and +-65504 through the twin's own half_to_float."""
    import quant_gemm.host as host
    n, k = 32, 512
    aq, bq = KR.extremes(np.random.default_rng([6, m]), m, n, k)
    c64, _, mag = KR.gemm(aq, bq)
    c1 = host.gemm_w4a8(aq, bq, m, n, k, Q4_K, threads=1)
    err = np.abs(c1.astype(np.float64) - c64)
    assert (err <= KR.tol(mag, k, 0)).all(), (err / KR.tol(mag, k, 0)).max()
    c40 = host.gemm_w4a8(aq, bq, m, n, k, Q4_K, threads=40)
    assert np.array_equal(c1.view(np.uint32), c40.view(np.uint32))


# ---------------------------------------------------------------------------- the view entry
def _view(ptr, qtype, k, rows, row_bytes, elem_bytes):
    from quant_gemm import ggml as G
    v = G.TensorView()
    v.data, v.type = ptr, qtype
    v.ne[:] = [k, rows, 1, 1]
    v.nb[:] = [elem_bytes, row_bytes, row_bytes * rows, row_bytes * rows]
    return v


def test_view_entry_refusals_for_q4k(so):
    """qg_gemm_w4a8_from_view validates before it touches a pointer: fake pointers, nothing launched."""
    from quant_gemm import ggml as G
    m, n, k = 3, 40, 512

    def call(act=None, w=None, out=None, kernel_type=b"auto", k_act=k, k_w=k):
        act = act or _view(4096, G.Q8_1, k_act, m, k_act // 32 * 36, 36)
        w = w or _view(8192, Q4_K, k_w, n, k_w // 256 * 144, 144)
        out = out or _view(16384, G.F32, n, m, n * 4, 4)
        return so.qg_gemm_w4a8_from_view(ctypes.byref(act), ctypes.byref(w), ctypes.byref(out), kernel_type, None)

    assert call(w=_view(8192, Q4_K, k, n, k // 256 * 144 + 16, 144)) == -3   # rows padded by 16 bytes
    assert call(k_act=288, k_w=288) == -2                                    # K % 256 (a multiple of 32)
    assert call(k_w=768) == -1                                               # w.ne[0] != act.ne[0]
    assert call(act=_view(4096, G.Q8_0, k, m, k // 32 * 34, 34)) == -3       # activations must be Q8_1
    assert call(act=_view(4096, G.F32, k, m, k * 4, 4)) == -3
    assert call(kernel_type=b"ragged") == -3                                 # no ragged (or generic) Q4_K kernel
    assert call(kernel_type=b"generic") == -3
    assert call(kernel_type=b"no such kernel") == -1
    assert call(w=_view(8192 + 8, Q4_K, k, n, k // 256 * 144, 144)) == -4    # weights off 16 B
    assert call(act=_view(4096 + 2, G.Q8_1, k, m, k // 32 * 36, 36)) == -4   # activations off 4 B


# ---------------------------------------------------------------------------- the reference's own helpers
def test_extremes_builder_holds_what_it_claims():
    """KR.extremes round-trips through KR.fields: every class is where the docstring says, nothing is Inf or NaN."""
    for m in (2, 12):
        aq, bq = KR.extremes(np.random.default_rng([6, m]), m)
        assert aq.shape == (m, 16, 36) and bq.shape == (32, 2, 144)
        d, dmin, sc, mn, q = KR.fields(bq)
        assert np.array_equal(KR.build(d, dmin, sc, mn, q), bq)
        assert np.isfinite(d).all() and np.isfinite(dmin).all()
        sub = lambda x: ((np.abs(x) >= 2.0 ** -24) & (np.abs(x) < 2.0 ** -14)).all()
        assert sub(d[:4]) and sub(dmin[:4])
        for x in (d[:4], dmin[:4]):  # both signs, the smallest and the largest subnormal
            assert (x > 0).any() and (x < 0).any()
        assert np.abs(d[:4]).min() == 2.0 ** -24 and np.abs(np.concatenate([d[:4], dmin[:4]])).max() == 1023 * 2.0 ** -24
        assert (np.abs(d[4]) == 2.0 ** -14).all() and (np.abs(dmin[4]) == 2.0 ** -14).all()
        assert (np.abs(d[5:9]) == 65504).all() and (np.abs(dmin[5:9]) == 65504).all()
        assert {(np.sign(d[r, 0]), np.sign(dmin[r, 0])) for r in range(5, 9)} == {(1, 1), (-1, -1), (1, -1), (-1, 1)}
        assert (sc[5] == 63).all() and (mn[5] == 63).all() and (q[5] == 15).all()
        assert (sc[9] == 0).all() and (mn[9] == 63).all() and (sc[10] == 63).all() and (mn[10] == 0).all()
        for r in range(11, 15):
            assert sorted(sc[r, 0, 4:]) == [16, 32, 48, 63] and sorted(mn[r, 0, 4:]) == [16, 32, 48, 63]
        assert {tuple(sc[r, 0, 4:]) for r in range(11, 15)} == {tuple(np.roll([16, 32, 48, 63], i)) for i in range(4)}
        da, sa, qa = KR.q8_1_fields(aq)
        assert np.isfinite(da).all() and np.isfinite(sa).all()
        assert sub(da[0]) and sub(sa[0]) and (sa[0] < 0).any() and (sa[0] > 0).any()
        assert sub(da[1, :8]) and (sa[1, :8] <= -36000).all() and sa[1].min() == -65504
        assert (da[1, 8:] == 65504).all() and (qa[1, 8:] == 127).all()
        c64, sumi, mag = KR.gemm(aq, bq)
        assert np.isfinite(c64).all() and mag.max() < 2.0 ** 60 and (mag > 0).all()
        # the largest single term of the contract: d = d_a = 65504, sc = 63, sumi = 15 * 127 * 32
        assert sumi[1, 5, 8] == 15 * 127 * 32 and mag[1, 5] >= 65504.0 * 63 * 65504 * 60960


def test_fuzz_cases_cover_both_families_and_all_offsets():
    cases = KR.fuzz_cases()
    assert cases == KR.fuzz_cases() and len(cases) == 24
    assert all(1 <= n <= 300 and k % 256 == 0 and 256 <= k <= 5120 for _, _, n, k, _, _ in cases)
    assert {w for *_, w, _ in cases} == set(KR.W_OFFSETS) and {a for *_, a in cases} == set(KR.A_OFFSETS)
    ms = [m for _, m, *_ in cases]
    assert min(ms) <= 8 < max(ms) and sum(m <= 8 for m in ms) >= 6 and sum(m > 8 for m in ms) >= 6
    # every M <= 8 shape of the sweep fits the GEMV's LDS, so the family follows M alone
    assert all(m * (k // 256) * 336 <= 160 * 1024 for _, m, _, k, _, _ in cases if m <= 8)
    lanes = {4 if k < 1024 else 16 if k < 4096 else 64 for _, m, _, k, _, _ in cases if m <= 8}
    assert lanes == {4, 16, 64}
