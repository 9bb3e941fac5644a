"""Q3_K (ggml type 11) without a GPU: the C ABI's static queries, validation and routing for the type, the GGUF reader,
and the host twins against the NumPy contract (tests/q3k_ref.py). No kernel is launched."""
import ctypes

import numpy as np
import pytest

import q3k_ref as QR

T = QR.Q3_K
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def so():
    import quant_gemm._lib as L
    return L.load()


def test_static_queries(so):
    import quant_gemm as qg
    import quant_gemm.host as host
    from quant_gemm import ggml as G
    assert so.qg_block_bytes(T) == 110 and so.qg_block_elems(T) == 256
    assert qg.Q3_K == 11 and qg.BLOCK_BYTES[11] == 110 and qg.Q3_K in qg.GEMM_WEIGHT_TYPES and "Q3_K" in qg.__all__
    assert host.BLOCK_BYTES[11] == 110 and G.Q3_K == 11 and G._BE[11] == 256


def test_the_model_round_trips_and_reaches_the_extremes():
    rng = np.random.default_rng(1)
    b = QR.random_q3k(rng, 5, 512)
    d, sc, q = QR.fields(b)
    assert np.array_equal(QR.build(d, sc, q), b) and sc.min() == 0 and sc.max() == 63 and (q.min(), q.max()) == (-4, 3)
    aq, bq = QR.extremes(rng, 3)
    c64, isum, mag = QR.gemm(aq, bq)
    assert np.isfinite(c64).all() and (np.abs(c64) <= mag).all() and mag.max() < 2.0 ** 127
    assert (isum[0, QR.MAX_ROW] == -2 ** 19).all() and np.abs(isum).max() == 2 ** 19
    assert (isum[0, QR.MAX_ROW + 1] == 31 * 4 * 128 * 32).all() and (isum[0, QR.MAX_ROW + 2] == 32 * 3 * 128 * 32).all()
    assert (c64[:, QR.D0_ROW] == 0).all() and (c64[:, QR.SC32_ROW] == 0).all()


def test_validation_order_on_fake_pointers(so):
    fake = P(4096)  # never dereferenced: validation fails first, or the call is empty
    assert so.qg_gemm_w4a8(fake, fake, fake, 1, 1, 288, T, None) == -2
    assert so.qg_gemm_w4a8(fake, P(4097), fake, 1, 1, 288, T, None) == -2      # K before the alignment
    assert so.qg_gemm_w4a8(fake, P(4097), fake, 1, 1, 256, T, None) == -4      # weights at an odd address
    assert so.qg_gemm_w4a8(P(4098), fake, fake, 1, 1, 256, T, None) == -4      # activations off 4 B
    assert so.qg_gemm_w4a8_ex(fake, P(4098), fake, 1, 1, 256, T, 3, None) == -3  # 2 mod 4 passes on: the generic algo
    assert so.qg_gemm_w4a8_ex(fake, P(4099), fake, 1, 1, 256, T, 3, None) == -4
    assert so.qg_gemm_w4a8(None, None, None, 0, 5, 256, T, None) == 0
    assert so.qg_debug_sumi(fake, P(4097), fake, 1, 1, 256, T, 0, None) == -4
    assert so.qg_dequantize(T, fake, fake, 288, None) == -2
    assert so.qg_dequantize(T, P(4097), fake, 256, None) == -4
    assert so.qg_gemm_w4a8_f32(fake, fake, fake, 2, 64, 256, T, None, 0, None) == -3
    assert so.qg_gemm_w4a8_moe(fake, 1, P(4097), 4, fake, 2, fake, 0, 3, 2, 64, 256, T, None) == -4
    assert so.qg_gemm_w4a8_moe(fake, 1, P(4098), 4, fake, 2, fake, 0, 0, 2, 64, 256, T, None) == 0


def test_the_other_entries_refuse_the_type(so):
    fake, buf = P(4096), ctypes.create_string_buffer(256)
    m, n, k, t, u, ne, big = 2, 64, 512, 2, 2, 4, 1 << 24
    assert so.qg_tile_weights(fake, fake, n, k, T, None) == -3
    assert so.qg_repack_weights(fake, fake, n, k, T, None) == -3
    assert so.qg_gemm_w4a8_grouped(fake, 1, m, k, T, None) == -3
    assert so.qg_gemm_w4a8_strided_batched(fake, 0, fake, 0, fake, 0, 1, m, n, k, T, None) == -3
    assert so.qg_gemm_w4a8_tiled(fake, fake, fake, m, n, k, T, None) == -3
    assert so.qg_gemm_w4a8_ws(fake, fake, fake, m, n, k, T, fake, big, None) == -3
    assert so.qg_quantize(T, 0, fake, fake, k, None) == -3
    assert so.qg_gemm_w4a8_moe_prefill(fake, 1, fake, ne, fake, u, fake, 0, t, u, n, k, T, fake, big, None) == -3
    assert so.qg_gemm_w4a8_moe_batch(fake, 1, fake, ne, fake, u, fake, 0, t, u, n, k, T, fake, big, None) == -3
    assert so.qg_gemm_w4a8_moe_glu(fake, fake, fake, ne, fake, u, fake, 0, t, u, n, k, T, 2, None) == -3
    assert so.qg_gemm_w4a8_moe_down(fake, fake, ne, fake, u, None, u, fake, 0, t, u, n, k, T, None) == -3
    for cfg in (so.qg_moe_glu_bias_config, so.qg_moe_down_bias_config):
        assert cfg(t, u, n, k, T, buf, 256) == -3
    for cfg in (so.qg_moe_prefill_bias_config, so.qg_moe_batch_bias_config):
        assert cfg(t, u, ne, n, k, T, buf, 256) == -3


@pytest.mark.parametrize("k,lpr,wgs,one", [(256, 4, 256, 1), (512, 4, 256, 0), (1024, 16, 512, 1), (2304, 16, 512, 0),
                                           (4096, 64, 1024, 1), (4352, 64, 1024, 0)])
def test_config_strings(so, k, lpr, wgs, one):
    import quant_gemm as qg
    rpb = wgs // lpr
    for m, mt in ((1, 1), (3, 4), (6, 8)):  # AUTO: the GEMV up to M = 6 (profiles/q3k/ab_q3k_threshold.txt)
        want = f"q3k_gemv MT={mt} LPR={lpr} WGS={wgs} ONE={one} grid={-(-67 // rpb)} lds={m * (k // 256) * 304}"
        assert qg.debug_config(m, 67, k, T) == want == qg.debug_config(m, 67, k, T, sumi=True)
        assert so.qg_select_algo(m, 67, k, T) == 1
    assert qg.debug_config(7, 67, k, T).startswith("q3k_mmq TT=1 RG=1 KS=8 grid=5x1") and so.qg_select_algo(7, 67, k, T) == 2
    assert qg.debug_config(8, 67, k, T, algo=1).startswith(f"q3k_gemv MT=8 LPR={lpr} ")  # forced up to M = 8
    assert qg.debug_config(6, 67, k, T, algo=2).startswith("q3k_mmq TT=1 ")
    assert qg.moe_config(3, 2, 67, k, T) == f"moe:q3k_gemv LPR={lpr} WGS={wgs} ONE={one} grid={-(-67 // rpb)}x6 lds={k // 256 * 304}"


def test_gguf_reads_a_type_11_tensor(tmp_path):
    from gguf_writer import write_gguf
    from quant_gemm import ggml as G
    b = QR.random_q3k(np.random.default_rng(9), 3, 512)
    p = tmp_path / "m.gguf"
    write_gguf(p, [], [("blk.0.ffn_down.weight", 11, [512, 3], b.tobytes())])
    with G.GGUFFile(p) as f:
        t = f.tensors["blk.0.ffn_down.weight"]
        assert t.type == 11 and t.nbytes == 3 * 2 * 110 and t.shape == (3, 2, 110)
        assert np.array_equal(f.host_bytes("blk.0.ffn_down.weight"), b)
    bad = tmp_path / "bad.gguf"
    write_gguf(bad, [], [("w", 11, [128, 3], b"\0" * 165)])
    with pytest.raises(RuntimeError):
        G.GGUFFile(bad)


@pytest.mark.parametrize("m,n,k", [(1, 1, 256), (3, 5, 768), (2, 7, 2304)])
def test_host_twin_matches_contract(m, n, k):
    """Within tol(W = 0) of the model, random rows and the extremes, and the same bits for 1 and 3 threads."""
    import quant_gemm.host as host
    rng = np.random.default_rng([m, n, k])
    for aq, bq in ((QR.random_q8_1(rng, m, k), QR.random_q3k(rng, n, k)), QR.extremes(rng, m, k)):
        n_ = bq.shape[0]
        c64, _, mag = QR.gemm(aq, bq)
        c1 = host.gemm_w4a8(aq, bq, m, n_, k, T, threads=1)
        err, tol = np.abs(c1.astype(np.float64) - c64), QR.tol(mag, k, 0)
        assert np.isfinite(c1).all() and (err <= tol).all(), (err / tol).max()
        assert np.array_equal(c1.view(np.uint32), host.gemm_w4a8(aq, bq, m, n_, k, T, threads=3).view(np.uint32))
    with pytest.raises(RuntimeError):
        host.gemm_w4a8(aq, bq, m, n_, k + 32, T)


def test_host_moe_twin_is_the_per_slot_product():
    import quant_gemm.host as host
    rng = np.random.default_rng(11)
    t, u, ne, n, k = 3, 2, 4, 7, 512
    experts = QR.random_q3k(rng, ne * n, k).reshape(ne, n, k // 256, 110)
    ids = np.array([[0, 3], [-1, 2], [4, 1]], np.int32)  # -1 and n_expert name no expert
    for a_rows in (1, u):
        aq = QR.random_q8_1(rng, t * a_rows, k).reshape(t, a_rows, k // 32, 36)
        c = host.gemm_w4a8_moe(aq, experts, ids, t, u, n, k, T, a_rows=a_rows, threads=3)
        for ti in range(t):
            for ui in range(u):
                e = int(ids[ti, ui])
                want = host.gemm_w4a8(aq[ti, ui % a_rows][None], experts[e], 1, n, k, T)[0] if 0 <= e < ne else np.zeros(n, np.float32)
                assert np.array_equal(c[ti, ui].view(np.uint32), want.view(np.uint32)), (a_rows, ti, ui)
