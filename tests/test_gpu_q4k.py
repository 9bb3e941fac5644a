"""Q4_K x Q8_1 on the GPU: the decode GEMV (q4k_gemv, M <= 8) and the MFMA prefill (q4k_mmq, M >= 9) against the
NumPy contract (tests/kquant_ref.py).

Every fp32 output must satisfy |c - C64| <= 2 (K/32 + W + 2) 2^-24 mag + 1e-30 with W = 0 for q4k_gemv and 16 for
q4k_mmq (the project's summation_tol / reassoc_tol form: twice the fp32 bound for K/32 + W terms of about three
roundings each); the per-sub-block int32 dots must be bit-equal; two launches must give identical bits.
"""
import functools

import numpy as np
import pytest

import kquant_ref as KR
from gguf_writer import as_bytes, write_gguf
from test_gpu_product import dev, host

pytestmark = pytest.mark.gpu

Q4_K = 12
GEMV_SHAPES = [(1, 64, 256), (2, 33, 2304), (4, 1000, 1024), (8, 48, 512), (5, 300, 4096), (1, 4096, 4096),
               (4, 32000, 1024)]
MMQ_SHAPES = [(9, 64, 256), (16, 16, 256), (17, 300, 2304), (32, 1000, 1024), (64, 4096, 512), (33, 8200, 512),
              # enough 64 x 64 tiles to fill 256 CUs: the 4-row-group form (RG=4), ragged in both dimensions
              (65, 16400, 256)]


@functools.lru_cache(maxsize=None)
def case(m, n, k, seed=0):
    """Inputs and the float64 reference of one shape, computed once and shared (never modified)."""
    rng = np.random.default_rng([m, n, k, seed])
    bq, aq = KR.random_q4k(rng, n, k), KR.random_q8_1(rng, m, k)
    return (aq, bq) + KR.gemm(aq, bq)


def check(qg, aq, bq, ref, fam, algo=0):
    """config names `fam` and equals its sumi twin; sumi bit-equal; output within tolerance; relaunch identical."""
    c64, sumi, mag = ref
    (m, nb), n = aq.shape[:2], bq.shape[0]
    k = 32 * nb
    cfg = qg.debug_config(m, n, k, Q4_K, algo=algo)
    assert cfg.startswith(fam + " "), cfg
    assert cfg == qg.debug_config(m, n, k, Q4_K, algo=algo, sumi=True)
    a, b = dev(aq), dev(bq)
    s = host(qg.debug_sumi(a, b, m, n, k, Q4_K, algo))
    assert np.array_equal(s, sumi)
    c = host(qg.gemm_w4a8(a, b, m, n, k, Q4_K, algo))
    tol = KR.tol(mag, k, 0 if fam == "q4k_gemv" else 16)
    err = np.abs(c.astype(np.float64) - c64)
    print(f"{fam} M={m} N={n} K={k}: max err/tol = {(err / tol).max():.3f}")
    assert (err <= tol).all(), (err / tol).max()
    c2 = host(qg.gemm_w4a8(a, b, m, n, k, Q4_K, algo))
    assert np.array_equal(c.view(np.uint32), c2.view(np.uint32))
    return c, s


@pytest.mark.parametrize("m,n,k", GEMV_SHAPES)
def test_gemv_shapes(qg, m, n, k):
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "q4k_gemv")


@pytest.mark.parametrize("m,n,k", MMQ_SHAPES)
def test_mmq_shapes(qg, m, n, k):
    aq, bq, *ref = case(m, n, k)
    check(qg, aq, bq, ref, "q4k_mmq")


@pytest.mark.parametrize("m", [2, 20])
def test_ldc_rows_leave_padding_untouched(qg, m):
    import torch
    n, k, pad = 100, 512, 5
    aq, bq, c64, _, mag = case(m, n, k)
    buf = torch.full((m, n + pad), -12345.0, dtype=torch.float32, device="cuda")
    out = qg.gemm_w4a8(dev(aq), dev(bq), m, n, k, Q4_K, out=buf[:, :n])
    assert out.data_ptr() == buf.data_ptr()
    got = host(buf)
    assert (got[:, n:] == -12345.0).all()
    err = np.abs(got[:, :n].astype(np.float64) - c64)
    assert (err <= KR.tol(mag, k, 0 if m <= 8 else 16)).all()
    dense = host(qg.gemm_w4a8(dev(aq), dev(bq), m, n, k, Q4_K))
    assert np.array_equal(dense.view(np.uint32), np.ascontiguousarray(got[:, :n]).view(np.uint32))


def test_forced_families_across_the_threshold(qg):
    """algo 1 at M = 8 and algo 2 at M = 4 are served, each within its tolerance, with identical sumi."""
    for m, n, k in ((8, 200, 1024), (4, 200, 1024)):
        aq, bq, *ref = case(m, n, k)
        _, s1 = check(qg, aq, bq, ref, "q4k_gemv", algo=1)
        _, s2 = check(qg, aq, bq, ref, "q4k_mmq", algo=2)
        assert np.array_equal(s1, s2)


@pytest.mark.parametrize("m", [2, 16])
def test_extremes(qg, m):
    n, k = 32, 512
    nsb = k // 256
    fam = "q4k_gemv" if m <= 8 else "q4k_mmq"
    rng = np.random.default_rng(7)
    aq = KR.random_q8_1(rng, m, k)
    sign = np.where(np.arange(m) % 2 == 0, 127, -127).astype(np.int8)
    aq[..., 4:36] = sign.view(np.uint8)[:, None, None]
    # all sc = m = 63, all nibbles 15 against +-127: the largest |sumi| = 15 * 127 * 32
    d = rng.uniform(-0.01, 0.01, (n, nsb))
    dmin = rng.uniform(-0.05, 0.05, (n, nsb))
    full = np.full((n, nsb, 8), 63, np.uint8)
    bq = KR.build(d, dmin, full, full, np.full((n, nsb, 8, 32), 15, np.uint8))
    ref = KR.gemm(aq, bq)
    assert np.abs(ref[1]).max() == 15 * 127 * 32
    check(qg, aq, bq, ref, fam)
    # a row of super-blocks with d = 0, one with dmin = 0
    aq2, bq2 = KR.random_q8_1(rng, m, k), KR.random_q4k(rng, n, k)
    bq2[0, :, 0:2] = 0
    bq2[1, :, 2:4] = 0
    check(qg, aq2, bq2, KR.gemm(aq2, bq2), fam)
    # zero Q8_1 blocks: every output is a zero
    aq0 = np.zeros_like(aq2)
    c, _ = check(qg, aq0, bq2, KR.gemm(aq0, bq2), fam)
    assert (c == 0).all()


def test_dequantize_bit_exact(qg):
    rng = np.random.default_rng(11)
    b = KR.random_q4k(rng, 7, 1024)
    y = host(qg.dequantize(dev(b), Q4_K))
    assert y.shape == (7, 1024)
    assert np.array_equal(y.view(np.uint32), KR.dequant(b).view(np.uint32))


def test_nmse_against_fp32(qg):
    """U[-1, 1] inputs, weights through the test-side quantizer: NMSE against the float64 product <= 5e-3 (the
    project's bar; the NumPy model of the contract gives 3.65e-3 on these inputs)."""
    m, n, k = 4, 512, 4096
    rng = np.random.default_rng(0)
    a = rng.uniform(-1, 1, (m, k)).astype(np.float32)
    w = rng.uniform(-1, 1, (n, k)).astype(np.float32)
    bq = KR.quantize(w)
    aq = qg.quantize_q8_1(dev(a))
    c = host(qg.gemm_w4a8(aq, dev(bq), m, n, k, Q4_K)).astype(np.float64)
    ref = a.astype(np.float64) @ w.astype(np.float64).T
    nmse = ((c - ref) ** 2).sum() / (ref ** 2).sum()
    print(f"Q4_K NMSE vs FP32 = {nmse:.3e}")
    assert nmse <= 5e-3, nmse


@pytest.mark.parametrize("m", [2, 12])
def test_f32_activations_through_workspace(qg, m):
    n, k = 64, 512
    rng = np.random.default_rng(13)
    x = dev(rng.uniform(-1, 1, (m, k)).astype(np.float32))
    b = dev(KR.random_q4k(rng, n, k))
    fused = host(qg.gemm_w4a8_f32(x, b, Q4_K))
    two = host(qg.gemm_w4a8(qg.quantize_q8_1(x), b, m, n, k, Q4_K))
    assert np.array_equal(fused.view(np.uint32), two.view(np.uint32))
    with pytest.raises(RuntimeError):
        qg.gemm_w4a8_f32(x, b, Q4_K, workspace=False)


def test_from_gguf_view(qg, tmp_path):
    import torch
    from quant_gemm import ggml as G
    m, n, k = 3, 40, 512
    aq, bq, *_ = case(m, n, k)
    path = str(tmp_path / "q4k.gguf")
    write_gguf(path, [], [("blk.0.ffn_up.weight", Q4_K, [k, n], as_bytes(bq))])
    a = dev(aq)
    out = torch.empty((m, n), dtype=torch.float32, device="cuda")
    with G.GGUFFile(path) as f:
        w = f.to_device("blk.0.ffn_up.weight")
        assert tuple(w.shape) == (n, k // 256, 144)
        wv = f.view("blk.0.ffn_up.weight", w)
        assert list(wv.nb[:2]) == [144, (k // 256) * 144]
        G.gemm_w4a8_from_ggml(G.view_of(a, G.Q8_1, k), wv, G.view_of(out, G.F32, n))
    direct = host(qg.gemm_w4a8(a, w, m, n, k, Q4_K))
    assert np.array_equal(host(out).view(np.uint32), direct.view(np.uint32))
