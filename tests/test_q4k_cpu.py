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
