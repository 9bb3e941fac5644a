"""IQ4_XS (ggml type 23) without a GPU: the C ABI's static queries, validation and routing for the type, the GGUF
reader, and the host twins against the NumPy contract (tests/iq4xs_ref.py). No kernel is launched."""
import ctypes

import numpy as np
import pytest

import iq4xs_ref as IR

T = IR.IQ4_XS
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def so():
    import quant_gemm._lib as L
    return L.load()


def test_static_queries(so):
    import quant_gemm as qg
    import quant_gemm.host as host
    from quant_gemm import ggml as G
    assert so.qg_block_bytes(T) == 136 and so.qg_block_elems(T) == 256
    assert qg.IQ4_XS == 23 and qg.BLOCK_BYTES[23] == 136 and qg.IQ4_XS in qg.GEMM_WEIGHT_TYPES and "IQ4_XS" in qg.__all__
    assert host.BLOCK_BYTES[23] == 136 and G.IQ4_XS == 23 and G._BE[23] == 256


def test_the_model_round_trips_and_stays_finite_at_the_extremes():
    rng = np.random.default_rng(1)
    b = IR.random_iq4xs(rng, 5, 512)
    d, ls, code = IR.fields(b)
    assert np.array_equal(IR.build(d, ls, code), b) and 0 <= ls.min() < 8 and 56 <= ls.max() <= 63
    aq, bq = IR.extremes(rng, 3)
    c64, sumi, mag = IR.gemm(aq, bq)
    assert np.isfinite(c64).all() and (np.abs(c64) <= mag).all() and mag.max() < 2.0 ** 127
    _, els, _ = IR.fields(bq)
    assert np.abs((els[IR.MAX_ROW, 0] - 32) * sumi[0, IR.MAX_ROW, :8]).max() == 16646144
    assert (c64[:, 5] == 0).all() and (c64[:, 8] == 0).all()  # d = 0, ls = 32


def test_validation_order_on_fake_pointers(so):
    fake = P(4096)  # never dereferenced: validation fails first, or the call is empty
    assert so.qg_gemm_w4a8(fake, fake, fake, 1, 1, 288, T, None) == -2
    assert so.qg_gemm_w4a8(fake, P(4100), fake, 1, 1, 288, T, None) == -2      # K before the alignment
    assert so.qg_gemm_w4a8(fake, P(4100), fake, 1, 1, 256, T, None) == -4      # weights 4 B past 8
    assert so.qg_gemm_w4a8(P(4098), fake, fake, 1, 1, 256, T, None) == -4      # activations off 4 B
    assert so.qg_gemm_w4a8_ex(fake, P(4104), fake, 1, 1, 256, T, 3, None) == -3  # 8 B passes on: the generic algo
    assert so.qg_gemm_w4a8_ex(fake, P(4100), fake, 1, 1, 256, T, 3, None) == -4
    assert so.qg_gemm_w4a8(None, None, None, 0, 5, 256, T, None) == 0
    assert so.qg_debug_sumi(fake, P(4100), fake, 1, 1, 256, T, 0, None) == -4
    assert so.qg_dequantize(T, fake, fake, 288, None) == -2
    assert so.qg_gemm_w4a8_f32(fake, fake, fake, 2, 64, 256, T, None, 0, None) == -3
    assert so.qg_gemm_w4a8_moe(fake, 1, P(4100), 4, fake, 2, fake, 0, 3, 2, 64, 256, T, None) == -4
    assert so.qg_gemm_w4a8_moe(fake, 1, P(4104), 4, fake, 2, fake, 0, 0, 2, 64, 256, T, None) == 0


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
    for m, mt in ((1, 1), (3, 4), (8, 8)):
        want = f"iq4xs_gemv MT={mt} LPR={lpr} WGS={wgs} ONE={one} grid={-(-67 // rpb)} lds={m * (k // 256) * 304}"
        assert qg.debug_config(m, 67, k, T) == want == qg.debug_config(m, 67, k, T, sumi=True)
        assert so.qg_select_algo(m, 67, k, T) == 1
    assert qg.debug_config(9, 67, k, T).startswith("iq4xs_mmq TT=1 RG=1 KS=8 grid=5x1") and so.qg_select_algo(9, 67, k, T) == 2
    assert qg.debug_config(8, 67, k, T, algo=2).startswith("iq4xs_mmq TT=1 ")
    assert qg.moe_config(3, 2, 67, k, T) == f"moe:iq4xs_gemv LPR={lpr} WGS={wgs} ONE={one} grid={-(-67 // rpb)}x6 lds={k // 256 * 304}"


def test_gguf_reads_a_type_23_tensor(tmp_path):
    from gguf_writer import write_gguf
    from quant_gemm import ggml as G
    b = IR.random_iq4xs(np.random.default_rng(9), 3, 512)
    p = tmp_path / "m.gguf"
    write_gguf(p, [], [("blk.0.ffn_down.weight", 23, [512, 3], b.tobytes())])
    with G.GGUFFile(p) as f:
        t = f.tensors["blk.0.ffn_down.weight"]
        assert t.type == 23 and t.nbytes == 3 * 2 * 136 and t.shape == (3, 2, 136)
        assert np.array_equal(f.host_bytes("blk.0.ffn_down.weight"), b)
    bad = tmp_path / "bad.gguf"
    write_gguf(bad, [], [("w", 23, [128, 3], b"\0" * 204)])
    with pytest.raises(RuntimeError):
        G.GGUFFile(bad)


@pytest.mark.parametrize("m,n,k", [(1, 1, 256), (3, 5, 768), (2, 7, 2304)])
def test_host_twin_matches_contract(m, n, k):
    """Within tol(W = 0) of the model, random rows and the extremes, and the same bits for 1 and 3 threads."""
    import quant_gemm.host as host
    rng = np.random.default_rng([m, n, k])
    for aq, bq in ((IR.random_q8_1(rng, m, k), IR.random_iq4xs(rng, n, k)), IR.extremes(rng, m, k)):
        n_ = bq.shape[0]
        c64, _, mag = IR.gemm(aq, bq)
        c1 = host.gemm_w4a8(aq, bq, m, n_, k, T, threads=1)
        err, tol = np.abs(c1.astype(np.float64) - c64), IR.tol(mag, k, 0)
        assert np.isfinite(c1).all() and (err <= tol).all(), (err / tol).max()
        assert np.array_equal(c1.view(np.uint32), host.gemm_w4a8(aq, bq, m, n_, k, T, threads=3).view(np.uint32))
    with pytest.raises(RuntimeError):
        host.gemm_w4a8(aq, bq, m, n_, k + 32, T)


def test_host_moe_twin_is_the_per_slot_product():
    import quant_gemm.host as host
    rng = np.random.default_rng(11)
    t, u, ne, n, k = 3, 2, 4, 7, 512
    experts = IR.random_iq4xs(rng, ne * n, k).reshape(ne, n, k // 256, 136)
    ids = np.array([[0, 3], [-1, 2], [4, 1]], np.int32)  # -1 and n_expert name no expert
    for a_rows in (1, u):
        aq = IR.random_q8_1(rng, t * a_rows, k).reshape(t, a_rows, k // 32, 36)
        c = host.gemm_w4a8_moe(aq, experts, ids, t, u, n, k, T, a_rows=a_rows, threads=3)
        for ti in range(t):
            for ui in range(u):
                e = int(ids[ti, ui])
                want = host.gemm_w4a8(aq[ti, ui % a_rows][None], experts[e], 1, n, k, T)[0] if 0 <= e < ne else np.zeros(n, np.float32)
                assert np.array_equal(c[ti, ui].view(np.uint32), want.view(np.uint32)), (a_rows, ti, ui)
