"""Pin the CPU oracle (oracle/qg_oracle.c) before trusting it as the parity checker.

Every expected value here comes from the reference: its own recorded known answers, its
self-contained KAT programs compiled from /root/reference into oracle/_ref/ (when present), and
golden vectors produced by its runnable Python definitions (tests/golden/make_golden.py).
"""
import glob
import json
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
REF_BIN = os.path.join(os.path.dirname(HERE), "oracle", "_ref")

with open(os.path.join(GOLD, "kat.json")) as f:
    KAT = json.load(f)


def test_half_conversion_exhaustive(O):
    # every fp16 bit pattern -> float matches numpy; float -> half RNE matches numpy on a sweep
    L = O.lib()
    bits = np.arange(0, 1 << 16, dtype=np.uint32)
    ref = bits.astype(np.uint16).view(np.float16).astype(np.float32)
    got = np.array([L.qgo_h2f(int(b)) for b in bits[::97]], np.float32)
    r = ref[::97]
    ok = (got == r) | (np.isnan(got) & np.isnan(r))
    assert ok.all()
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.standard_normal(20000).astype(np.float32) * 10.0 ** rng.integers(-9, 6, 20000),
                         np.float32([0.0, -0.0, 65504.0, 65520.0, 1e-8, 6.1e-5, 5.96e-8, 2.98e-8])]).astype(np.float32)
    with np.errstate(over="ignore"):
        want = xs.astype(np.float16).view(np.uint16)
    got = np.array([L.qgo_f2h(float(x)) for x in xs], np.uint16)
    assert (got == want).all()


def test_kat3_dot4(O):
    for a, b, want in KAT["kat3_dp4a"]["cases"]:
        assert O.dot4(a, b) == want


def test_kat1_step4_compensation(O):
    k = KAT["kat1_step4_compensation"]
    a = np.array(k["a"], np.float32)[None]
    w = np.array(k["w"], np.float32)[None]
    fp32 = O.gemm_fp32(a, w)[0, 0]
    assert f"{fp32:.6f}" == k["fp32"]
    aq = O.quantize(a, O.Q8_1)
    wq = O.quantize(w, O.Q4_0)
    assert wq[0, 0, :2].view(np.uint16)[0] == int(k["d_w_half"], 16)
    assert aq[0, 0, :2].view(np.uint16)[0] == int(k["d_a_half"], 16)
    assert aq[0, 0, 2:4].view(np.uint16)[0] == int(k["s_a_half"], 16)
    assert wq[0, 0, 2:].tobytes().hex() == k["q4_qs"]
    assert aq[0, 0, 4:].view(np.int8).tolist() == k["q8_qs"]
    c, s = O.gemm_w4a8(aq, wq, O.Q4_0, want_sumi=True)
    assert int(s[0, 0, 0]) == k["sumi"]
    assert f"{c[0, 0]:.6f}" == k["with_compensation"]
    assert f"{O.vec_dot_q4_0_q8_1(wq, aq):.6f}" == k["with_compensation"]
    d_w = np.float32(np.float16(wq[0, 0, :2].view(np.float16)[0]))
    d_a = np.float32(aq[0, 0, :2].view(np.float16)[0])
    assert f"{np.float32(s[0, 0, 0]) * d_a * d_w:.6f}" == k["without_compensation"]


def _kat2_inputs():
    i = np.arange(32)
    return ((i % 16) - 8).astype(np.float32)[None], (i - 16).astype(np.float32)[None]


def test_kat2_cpu_ref_formula(O):
    k = KAT["kat2_test_cpu_ref"]
    w, a = _kat2_inputs()
    assert f"{O.gemm_fp32(a, w)[0, 0]:.6f}" == k["reference"]
    aq = O.quantize(a, O.Q8_1, variant=1)  # tests/framework to_q8_1: s = d * sum(q)
    wq = O.quantize(w, O.Q4_0)
    _, s = O.gemm_w4a8(aq, wq, O.Q4_0, want_sumi=True)
    assert int(s[0, 0, 0]) == k["sumi"]
    assert int(aq[0, 0, 4:].view(np.int8).astype(np.int32).sum()) == k["sum_a_q"]
    assert f"{np.float32(aq[0, 0, 2:4].view(np.float16)[0]):.6f}" == k["s_a"]
    # the KAT keeps fp32 (unrounded) scales: same block formula on those reproduces its output
    d_w = np.float32(8.0) / np.float32(7.0)
    d_a = np.float32(16.0) / np.float32(127.0)
    s_a = np.float32(k["sum_a_q"]) * d_a
    out = d_w * (d_a * np.float32(k["sumi"]) - np.float32(8.0) * s_a)
    assert f"{out:.6f}" == k["result"]


def _ref_kat_stdout(name):
    """What the reference's own KAT program `name` prints: the recording in tests/golden/ref_kat_stdout.json,
    which the live program must reproduce where oracle/_ref holds it (built when the reference tree is there)."""
    with open(os.path.join(GOLD, "ref_kat_stdout.json")) as f:
        recorded = "\n".join(json.load(f)[name]) + "\n"
    exe = os.path.join(REF_BIN, name)
    if os.path.exists(exe):
        assert subprocess.run([exe], capture_output=True, text=True, check=True).stdout == recorded
    return recorded


def test_kat2_against_compiled_reference(O):
    """The reference's own test_cpu_ref / test_dot / test_q8_1 output compared with the oracle."""
    out = _ref_kat_stdout("test_cpu_ref")
    w, a = _kat2_inputs()
    aq = O.quantize(a, O.Q8_1, variant=1)
    wq = O.quantize(w, O.Q4_0)
    _, s = O.gemm_w4a8(aq, wq, O.Q4_0, want_sumi=True)
    assert f"sumi = {int(s[0, 0, 0])}" in out
    qs0 = wq[0, 0, 2]
    assert f"qs[0]=0x{qs0:02x}" in out
    for i in range(4):
        assert f"qs[{i}]={int(aq[0, 0, 4 + i].view(np.int8))} " in out
    out2 = _ref_kat_stdout("test_dot")
    assert f"sumi = {int(s[0, 0, 0])}" in out2
    out3 = _ref_kat_stdout("test_q8_1")
    x = ((np.arange(32) - 16) * np.float32(0.1)).astype(np.float32)[None]
    q = O.quantize(x, O.Q8_1, variant=1)
    assert f"sum_q = {int(q[0, 0, 4:].view(np.int8).astype(np.int32).sum())}" in out3


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "w4a8_*.npz"))), ids=os.path.basename)
def test_golden_w4a8(O, path):
    """Oracle == the reference's Python definition on the same bytes (it sums in fp64, so allow
    fp32-summation-level differences), and the inputs regenerate bit-exactly."""
    g = np.load(path)
    m, n, k, t, seed = (int(g[x]) for x in ("m", "n", "k", "wtype", "seed"))
    a, b = O.fill_uniform_step4(m, n, k, seed)
    assert np.array_equal(a[0, :8], g["a_head"]) and np.array_equal(b[0, :8], g["b_head"])
    aq = O.quantize(a, O.Q8_1)
    bq = O.quantize(b, t)
    assert np.array_equal(aq, g["a_q"]) and np.array_equal(bq, g["b_q"])
    c, s = O.gemm_w4a8(aq, bq, t, want_sumi=True)
    tol = O.summation_tol(aq, bq, s, t) + 1e-6 * np.abs(g["c_ref"])
    assert (np.abs(c.astype(np.float64) - g["c_ref"]) <= tol).all()
    assert np.array_equal(O.gemm_fp32(a, b), g["c_fp32"])


def test_golden_plumbing_nmse(O):
    """BASELINE configs[0]: W4A8 vs FP32 NMSE equals the reference's recorded 4.2747e-3."""
    g = np.load(os.path.join(GOLD, "w4a8_q4_0_plumbing.npz"))
    c = O.gemm_w4a8(g["a_q"], g["b_q"], O.Q4_0)
    assert f"{O.nmse(c, g['c_fp32']):.4e}" == f"{KAT['nmse_vs_fp32']['m1_n128_k256']:.4e}"


def test_golden_quantize_q8_1(O):
    """Oracle Q8_1 bytes vs the reference definition's quantizer. The definition uses x/d and
    np.round (ties to even) where include/quantize.h uses x*(1/d) and roundf; the two can only
    differ by one code on elements whose scaled value is within an ulp of a .5 tie."""
    g = np.load(os.path.join(GOLD, "quantize_q8_1_m16k128.npz"))
    q = O.quantize(g["x"], O.Q8_1)
    ref = g["q_ref"]
    assert np.array_equal(q[..., :4], ref[..., :4])  # d and s halves identical
    diff = q[..., 4:].view(np.int8).astype(int) - ref[..., 4:].view(np.int8).astype(int)
    assert np.abs(diff).max() <= 1
    x = g["x"].reshape(16, 4, 32)
    d = np.abs(x).max(-1, keepdims=True) / np.float32(127.0)
    frac = np.abs((x * (np.float32(1.0) / d)) % 1.0 - 0.5)
    assert (frac[diff != 0] < 1e-4).all()


def test_definition_q8_1_matches_flashinfer_fixture(O):
    """The definition-semantics restatement (oracle.quantize_definition, variant 2: ties to even,
    true division, d = 1.0 for a zero block) reproduces the flashinfer Q8_1 definition's own output
    bytes (quantize/quantize_q8_1_k4096.json:66, same semantics) byte for byte — all 36 bytes of
    every block, where the include/quantize.h quantizer differs by one code at ties."""
    g = np.load(os.path.join(GOLD, "quantize_q8_1_m16k128.npz"))
    assert np.array_equal(O.quantize(g["x"], O.Q8_1, 2), g["q_ref"])


def test_definition_f16_scale_is_single_rounding(O):
    """The stored f16 d of the definitions (a Python float converted once) is the correctly rounded
    f16 of the exact quotient amax / 127 (/ 7): checked with exact rational arithmetic on every block
    of the parity set — and it equals f16(f32(amax / div)), the double rounding of include/quantize.h
    and of the GPU quantizer (f32(amax / div) is never an inexact f16 midpoint: one f32 step of amax
    moves the quotient by 64/127 or 4/7 of an f32 step of the quotient, more than half)."""
    from fractions import Fraction
    from qdef_cases import definition_inputs
    x = definition_inputs().reshape(-1, 32)
    for t, div in ((O.Q8_1, 127), (O.Q4_0, 7)):
        q = O.quantize_definition(x, t)
        dh = q[..., 0:2].copy().view(np.uint16)[:, 0, 0]
        amax = np.abs(x).max(axis=1)
        for i in range(x.shape[0]):
            if amax[i] == 0:
                assert dh[i] == 0x3C00
                continue
            f = Fraction(float(amax[i])) / div
            assert dh[i] == O.f16_round_exact(f.numerator, f.denominator), i
            assert dh[i] == np.float32(amax[i] / np.float32(div)).astype(np.float16).view(np.uint16)


def test_definition_mismatch_set_vs_quantize_h(O):
    """Where the definitions' semantics and the pinned include/quantize.h quantizer (variant 0) give
    different bytes, every difference is one of the documented causes, and each cause occurs in the
    parity set: an all-zero block's d (1.0 vs 0); a code one step apart at an exact round-half tie
    (even vs away) or where x / d and x * (1/d) straddle a half-integer. Nothing else (no nonzero
    block's d or s differs, no code more than one step apart)."""
    from qdef_cases import definition_inputs
    x = definition_inputs().reshape(-1, 32)
    amax = np.abs(x).max(axis=1)
    for t, div in ((O.Q8_1, 127.0), (O.Q4_0, 7.0)):
        v0, v2 = O.quantize(x, t, 0)[:, 0], O.quantize(x, t, 2)[:, 0]
        d32 = (amax / np.float32(div)).astype(np.float32)
        zero = amax == 0
        d0 = v0[:, 0:2].copy().view(np.uint16)[:, 0]
        d2 = v2[:, 0:2].copy().view(np.uint16)[:, 0]
        assert (d0[zero] == 0).all() and (d2[zero] == 0x3C00).all()
        assert np.array_equal(d0[~zero], d2[~zero])
        if t == O.Q8_1:
            assert np.array_equal(v0[:, 2:4], v2[:, 2:4])  # s identical
            c0, c2 = v0[:, 4:].view(np.int8).astype(int), v2[:, 4:].view(np.int8).astype(int)
        else:
            c0 = np.concatenate([v0[:, 2:] & 15, v0[:, 2:] >> 4], axis=1).astype(int)
            c2 = np.concatenate([v2[:, 2:] & 15, v2[:, 2:] >> 4], axis=1).astype(int)
        diff = c0 != c2
        assert (np.abs(c0 - c2) <= 1).all()
        with np.errstate(divide="ignore", invalid="ignore"):
            r = (x / np.where(zero, 1, d32)[:, None]).astype(np.float32)
        frac = np.abs(np.abs(r) % 1.0 - 0.5)
        assert (frac[diff] <= 1e-5 * np.maximum(1, np.abs(r[diff]))).all()
        assert (frac[diff] == 0).sum() >= 100  # exact ties present (x / d vs x * (1/d) straddling a
        # half-integer needs x / d within an f32 step of it: allowed above, about 1 % likely in this set)


@pytest.mark.parametrize("t", [2, 3, 6, 7])
def test_allquants_nmse_small(O, t):
    """All-quants formulas (no /4) stay within the FP32-anchored bounds at a CPU-fast size."""
    a, b = O.fill_uniform_step4(2, 256, 1024)
    c = O.gemm_w4a8(O.quantize(a, O.Q8_1), O.quantize(b, t), t)
    bound = {2: 8e-3, 3: 8e-3, 6: 3e-3, 7: 3e-3}[t]
    assert O.nmse(c, O.gemm_fp32(a, b)) < bound


def test_dequantize_roundtrip(O):
    a, b = O.fill_uniform_step4(4, 4, 256)
    for t in (2, 3, 6, 7, 8, 9):
        x = O.dequantize(O.quantize(b, t), t)
        assert np.abs(x - b).max() < {2: 0.08, 3: 0.075, 6: 0.04, 7: 0.04, 8: 0.005, 9: 0.005}[t]


def test_w8a8_oracle_paths_agree(O):
    """qgo_gemm_w4a8 with Q8_0 weights == the separate gemm_w8a8_reference restatement, bitwise."""
    a, b = O.fill_uniform_step4(3, 64, 1024)
    aq, bq = O.quantize(a, O.Q8_1), O.quantize(b, O.Q8_0)
    c = O.gemm_w4a8(aq, bq, O.Q8_0)
    assert np.array_equal(c, O.gemm_w8a8(aq, bq))
    assert O.nmse(c, O.gemm_fp32(a, b)) < 1e-4


def _fused_f16_quantize_numpy(x16: np.ndarray) -> np.ndarray:
    """Independent numpy restatement of kernels/gemm/gemm_fused.cuh:76-143 for one row."""
    f32 = np.float32
    out = np.zeros((x16.size // 32, 36), np.uint8)
    for b in range(x16.size // 32):
        x = x16[32 * b:32 * b + 32].astype(f32)
        mx, sm = np.abs(x), x.copy()
        for h in (16, 8, 4, 2):
            mx[:h] = np.maximum(mx[:h], mx[h:2 * h])
            sm[:h] = sm[:h] + sm[h:2 * h]
        amax, s = max(mx[0], mx[1]), f32(sm[0] + sm[1])
        dh = np.float16(f32(amax) / f32(127.0))
        d = f32(dh)
        inv = f32(1.0) / d if d != 0 else f32(0.0)
        v = (x * inv).astype(np.float64)
        q = np.clip(np.sign(v) * np.floor(np.abs(v) + 0.5), -127, 127).astype(np.int8)
        out[b, 0:2] = np.frombuffer(dh.tobytes(), np.uint8)
        out[b, 2:4] = np.frombuffer(np.float16(s).tobytes(), np.uint8)
        out[b, 4:] = q.view(np.uint8)
    return out


def test_fused_f16_quantizer_two_restatements_agree(O):
    """The C restatement (oracle) and an independent numpy one agree byte for byte; the reference's
    own fused kernel is CUDA-only and racy, so this row is pinned by restatement."""
    rng = np.random.default_rng(9)
    rows = [(rng.standard_normal(256) * s).astype(np.float16) for s in (1e-3, 1.0, 40.0, 2000.0)]
    rows.append(np.zeros(64, np.float16))
    rows.append(rng.choice(np.array([-1000.0, 0.25, 3.0, -0.125, 1e-3], np.float16), size=256))
    for x in rows:
        assert np.array_equal(O.quantize_q8_1_fused_f16(x), _fused_f16_quantize_numpy(x))


def test_fused_f16_gemm_oracle_transposes(O):
    """qgo_gemm_q4_0_fp16_fused (weight-major) == the activation-major W4A8 oracle on the same bytes."""
    rng = np.random.default_rng(4)
    act = rng.standard_normal((5, 512)).astype(np.float16)
    _, b = O.fill_uniform_step4(1, 24, 512)
    wq = O.quantize(b, O.Q4_0)
    out = O.gemm_q4_0_fp16_fused(wq, act)
    assert np.array_equal(out, O.gemm_w4a8(O.quantize_q8_1_fused_f16(act), wq, O.Q4_0).T)


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLD, "w4a16_*.npz"))), ids=os.path.basename)
def test_golden_w4a16(O, path):
    """W4A16 oracle vs the reference's own Python definition (w4a16_q4_0_fp32_n4096_k4096.json).

    That definition dequantizes a Q4_0 block in INTERLEAVED element order (lo nibble i -> element
    2i, hi nibble i -> 2i+1), unlike gemm_reference.h / ggml (lo -> i, hi -> 16+i), which this
    library follows. Re-ordering the activations to the ggml order makes the two the same
    product, which pins the arithmetic; the raw outputs differ (asserted, so the defect stays
    documented)."""
    g = np.load(path)
    a, bq, c_ref = g["a"], g["b_q"], g["c_ref"]
    m, k = a.shape
    blk = a.reshape(m, k // 32, 32)
    a_ggml = np.concatenate([blk[..., 0::2], blk[..., 1::2]], axis=-1).reshape(m, k)
    c = O.gemm_w4a16(a_ggml, bq)
    assert (np.abs(c.astype(np.float64) - c_ref) <= O.w16_tol(a_ggml, bq, O.Q4_0)).all()
    assert not np.allclose(O.gemm_w4a16(a, bq), c_ref, atol=1e-3)


def test_w8a16_oracle_vs_fp64(O):
    a, b = O.fill_uniform_step4(3, 40, 512)
    bq = O.quantize(b, O.Q8_0)
    c = O.gemm_w8a16(a, bq)
    exact = a.astype(np.float64) @ O.dequantize(bq, O.Q8_0).astype(np.float64).T
    assert (np.abs(c - exact) <= O.w16_tol(a, bq, O.Q8_0)).all()


# NMSE vs FP32 recorded in SURVEY.md Appendix A from the reference compiled in the survey container
# (gemm_w4a8_reference / gemm_fp32_reference; the all-quants row with the test_framework quantizers,
# tests/framework/test_framework.cuh:195-367, i.e. Q8_1 variant 1). Five significant figures of
# NMSE over 4096 outputs fingerprint the quantizer and dot restatements, incl. the Q4_1/Q5_0/Q5_1
# ones no reference-held byte vector pins.
@pytest.mark.parametrize("key,m,n,k", [("m1_n128_k256", 1, 128, 256), ("m1_n4096_k4096", 1, 4096, 4096),
                                       ("m32_n4096_k4096", 32, 4096, 4096), ("m1_n32000_k4096", 1, 32000, 4096)])
def test_recorded_nmse_q4_0(O, key, m, n, k):
    a, b = O.fill_uniform_step4(m, n, k, 42)
    c = O.gemm_w4a8(O.quantize(a, O.Q8_1), O.quantize(b, O.Q4_0))
    want = KAT["nmse_vs_fp32"][key]
    assert abs(O.nmse(c, O.gemm_fp32(a, b)) - want) <= 5e-5 * want


@pytest.mark.parametrize("name,t", [("q4_0", 2), ("q4_1", 3), ("q5_0", 6), ("q5_1", 7)])
def test_recorded_nmse_allquants(O, name, t):
    a, b = O.fill_uniform_step4(1, 4096, 4096, 42)
    c = O.gemm_w4a8(O.quantize(a, O.Q8_1, 1), O.quantize(b, t), t)
    want = KAT["nmse_vs_fp32"]["allquants_m1_n4096_k4096"][name]
    # printed with 5 significant figures; the FP32 reference's float summation may move the last
    assert abs(O.nmse(c, O.gemm_fp32(a, b)) - want) <= 1.5e-4 * want


@pytest.mark.parametrize("t", [2, 3, 6, 7, 8])
def test_reassoc_tol_covers_split_epilogue(O, t):
    """oracle.reassoc_tol (the MFMA prefill's bar) holds for a numpy emulation of that kernel's
    arithmetic — d_w*d_a formed exactly, times sumi rounded once per block, the offset parts summed
    on their own, 8 K-split partials added in order, combined at the end — at the small K where
    summation_tol (which assumes bit-identical per-block terms) is too tight for it."""
    m, n, k = 24, 40, 128
    a, b = O.fill_uniform_step4(m, n, k, 3 + t)
    aq, bq = O.quantize(a, O.Q8_1), O.quantize(b, t)
    c_ref, s = O.gemm_w4a8(aq, bq, t, want_sumi=True)
    dot, off = O.block_parts(aq, bq, s, t)
    f32 = np.float32
    p = dot.astype(f32)                                   # one rounding per block (exact dd * sumi)
    nb = p.shape[-1]
    waves = 8
    acc = np.zeros(p.shape[:2], f32)
    comp = np.zeros(p.shape[:2], f32)
    for w in range(waves):                                # K split over waves, partials in order
        pa = np.zeros(p.shape[:2], f32)
        pc = np.zeros(p.shape[:2], f32)
        for bi in range(w, nb, waves):
            pa = (pa + p[..., bi]).astype(f32)
            pc = (pc + off[..., bi].astype(f32)).astype(f32)
        acc = (acc + pa).astype(f32)
        comp = (comp + pc).astype(f32)
    got = (acc + comp).astype(f32).astype(np.float64)
    assert (np.abs(got - c_ref) <= O.reassoc_tol(aq, bq, s, t)).all()
    assert (O.reassoc_tol(aq, bq, s, t) >= O.summation_tol(aq, bq, s, t)).all()
