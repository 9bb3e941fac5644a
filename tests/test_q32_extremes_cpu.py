"""What can be settled without a GPU about tests/q32_extremes.py: the classes sit where the docstring says, the
reference stays finite, the bounds of the GPU tests (tests/test_gpu_q32_extremes.py) have teeth on these inputs — a
kernel that flushed f16 subnormal scales, or dropped the sign of d_a, would leave them — and the host twins hold.
"""
import ctypes
import functools

import numpy as np
import pytest

import q32_extremes as QE

M, N = 8, 19  # six token classes + two random tokens; thirteen row classes + six random rows
KS = (128, 1056)


@functools.lru_cache(maxsize=None)
def case(t, k):
    """(aq, bq, c_ref float32 [M, N], sumi), read-only."""
    import oracle as O
    aq, bq = QE.extremes(np.random.default_rng([t, k]), t, M, N, k)
    c, s = O.gemm_w4a8(aq, bq, t, want_sumi=True)
    for x in (aq, bq, c, s):
        x.setflags(write=False)
    return aq, bq, c, s


def is_sub(x):
    return (np.abs(x) >= 2.0 ** -24) & (np.abs(x) < 2.0 ** -14)


@pytest.mark.parametrize("t", QE.TYPES)
@pytest.mark.parametrize("k", KS)
def test_classes_sit_where_the_docstring_says(O, t, k):
    """Read back with the oracle's own decoding: oracle._h for the f16 fields, oracle.dequantize (on a copy with d = 1,
    m = 0) for the codes."""
    aq, bq, _, _ = case(t, k)
    nb = k // 32
    assert aq.shape == (M, nb, 36) and bq.shape == (N, nb, QE.BB[t])
    d = O._h(bq[..., 0:2]).astype(np.float64)
    da, sa = O._h(aq[..., 0:2]).astype(np.float64), O._h(aq[..., 2:4]).astype(np.float64)
    qa = aq[..., 4:36].view(np.int8).astype(np.int32)
    assert np.isfinite(d).all() and np.isfinite(da).all() and np.isfinite(sa).all()
    unit = bq.copy()
    unit[..., 0:2] = QE.f16_bytes(np.ones((N, nb)))
    if t in QE.HAS_M:
        unit[..., 2:4] = 0
    q = O.dequantize(unit, t).reshape(N, nb, 32).astype(np.int32) + {2: 8, 6: 16}.get(t, 0)
    assert np.array_equal(q, QE.codes(t, bq))
    lo, hi = QE.code_range(t)

    assert (d[QE.ROW_SUB_POS] == 2.0 ** -24).all() and (d[QE.ROW_SUB_NEG] == -2.0 ** -24).all()
    c = d[QE.ROW_SUB_CYCLE]
    assert is_sub(c).all() and (c > 0).any() and (c < 0).any()
    assert np.abs(c).min() == 2.0 ** -24 and np.abs(c).max() == (1023 * 2.0 ** -24 if nb >= 5 else 2.0 ** -15)
    assert (np.abs(d[QE.ROW_MIN_NORMAL]) == 2.0 ** -14).all()
    assert (d[QE.ROW_MAX_POS] == 65504).all() and (q[QE.ROW_MAX_POS] == hi).all()
    assert (d[QE.ROW_MAX_NEG] == -65504).all() and (q[QE.ROW_MAX_NEG] == hi).all()
    assert (d[QE.ROW_MAX_CODE_MIN] == 65504).all() and (q[QE.ROW_MAX_CODE_MIN] == lo).all()
    if t in QE.QH_OFF:
        qh = bq[..., QE.QH_OFF[t]:QE.QH_OFF[t] + 4]
        assert (qh[QE.ROW_MAX_POS] == 0xFF).all() and (qh[QE.ROW_MAX_CODE_MIN] == 0).all()
    for r, sign in ((QE.ROW_ZERO_POS, False), (QE.ROW_ZERO_NEG, True)):
        assert (d[r] == 0).all() and (np.signbit(d[r]) == sign).all()
    if t in QE.HAS_M:
        mw = O._h(bq[..., 2:4]).astype(np.float64)
        assert np.isfinite(mw).all()
        assert is_sub(mw[list(QE.SUBNORMAL_ROWS)]).all() and (np.abs(mw[QE.ROW_MIN_NORMAL]) == 2.0 ** -14).all()
        assert (np.abs(mw[[QE.ROW_MAX_POS, QE.ROW_MAX_NEG, QE.ROW_MAX_CODE_MIN]]) == 65504).all()
        assert is_sub(mw[QE.ROW_M_SUB]).all() and (np.abs(d[QE.ROW_M_SUB]) == 2.0 ** -13).all()
        assert (mw[QE.ROW_M_SUB] > 0).any() and (mw[QE.ROW_M_SUB] < 0).any()
        assert (q[QE.ROW_M_SUB, :, 0] == 1).all() and (q[QE.ROW_M_SUB, :, 1:] == 0).all()
        assert (mw[QE.ROW_M_MAX_POS] == 65504).all() and (mw[QE.ROW_M_MAX_NEG] == -65504).all()
        assert is_sub(d[[QE.ROW_M_MAX_POS, QE.ROW_M_MAX_NEG]]).all()
        assert (mw[QE.ROW_M_ZERO] == 0).all() and (d[QE.ROW_M_ZERO] != 0).any()
    # the rows past the classes keep random_blocks' band
    rest = d[QE.row_classes(t):]
    assert rest.shape[0] >= N - QE.EXTREME_ROWS and (np.abs(rest) <= 0.1).all() and not is_sub(rest).all()

    assert (da[QE.TOK_SUB] == 2.0 ** -24).all() and (sa[QE.TOK_SUB] == 2.0 ** -24).all()
    assert is_sub(da[QE.TOK_SUB_CYCLE]).all() and is_sub(sa[QE.TOK_SUB_CYCLE]).all()
    assert (sa[QE.TOK_SUB_CYCLE] < 0).any() and (sa[QE.TOK_SUB_CYCLE] > 0).any()
    for tok, s, qv in ((QE.TOK_MAX_NEG, -65504, -128), (QE.TOK_MAX_POS, 65504, 127)):
        assert (da[tok] == 65504).all() and (sa[tok] == s).all() and (qa[tok] == qv).all()
    neg = da[QE.TOK_NEG_D]
    assert (neg <= -1e-3 + 1e-6).all() and (neg >= -2e-2 - 1e-4).all() and not is_sub(neg).any()
    assert (da[QE.TOK_NEG_ZERO] == 0).all() and np.signbit(da[QE.TOK_NEG_ZERO]).all()
    assert (da[QE.TOKEN_CLASSES:] >= 1e-3 - 1e-6).all() and (np.abs(sa[QE.TOKEN_CLASSES:]) <= 5).all()


def test_tokens_argument_selects_the_classes():
    """tokens= puts the chosen classes into the first tokens (what the M = 1 and M = 2 GPU cases rotate through)."""
    t, k = 2, 128
    full, _ = QE.extremes(np.random.default_rng(1), t, 6, N, k)
    for sel in ((4,), (5, 0), (1, 3), (2,)):
        aq, bq = QE.extremes(np.random.default_rng(1), t, len(sel), N, k, tokens=sel)
        for i, c in enumerate(sel):
            if c in (QE.TOK_NEG_D, QE.TOK_NEG_ZERO):  # built on the call's own random bytes
                h = aq[i, :, 0:2].copy().view(np.float16)[:, 0]
                assert np.signbit(h).all() and ((h == 0).all() if c == QE.TOK_NEG_ZERO else (h <= -1e-3 + 1e-6).all())
            else:
                assert np.array_equal(aq[i, :, 0:4], full[c, :, 0:4])
    with pytest.raises(AssertionError):
        QE.extremes(np.random.default_rng(1), t, 1, N, k, tokens=(0, 1))
    with pytest.raises(AssertionError):
        QE.extremes(np.random.default_rng(1), t, 1, QE.EXTREME_ROWS - 1, k)


@pytest.mark.parametrize("t", QE.TYPES)
@pytest.mark.parametrize("k", KS)
def test_reference_is_finite_and_no_class_vanishes(O, t, k):
    aq, bq, c, s = case(t, k)
    assert np.isfinite(c).all()
    terms = O.block_terms(aq, bq, s, t).astype(np.float64)
    assert np.isfinite(terms).all()
    mag = np.abs(terms).sum(-1)
    zero = QE.zero_outputs(t, M, N, range(QE.TOKEN_CLASSES))
    assert (mag[~zero] > 0).all() and (mag[zero] == 0).all() and (c[zero] == 0).all()
    # the largest |term| the docstring states (Q8_0 reaches it: -128 codes on qs = -128, d_w = d_a = 65504)
    assert np.abs(terms).max() <= QE.MAX_TERM < 2.3e15
    if t == 8:
        assert terms[QE.TOK_MAX_NEG, QE.ROW_MAX_CODE_MIN].max() == QE.MAX_TERM
    assert mag.max() * 256 / (k // 32) < 2.0 ** 60  # a K = 8192 row of such terms is still far inside fp32


@pytest.mark.parametrize("t", QE.TYPES)
@pytest.mark.parametrize("k", KS)
def test_bounds_have_teeth_against_flushed_subnormals(O, t, k):
    """With every f16 subnormal d_w, m_w, d_a and s_a replaced by zero, every output whose row or token class is
    subnormal leaves both bounds of the GPU tests (summation_tol; reassoc_tol with 8 waves, the widest the row-layout
    tests use, and with the tiled tests' 16)."""
    aq, bq, c, s = case(t, k)
    c_fl = O.gemm_w4a8(*QE.flush_subnormals(t, aq, bq), t)
    diff = np.abs(c_fl.astype(np.float64) - c)
    sel = np.zeros((M, N), bool)
    sel[list(QE.SUBNORMAL_TOKENS), :] = True
    sel[:, list(QE.subnormal_rows(t))] = True
    sel &= ~QE.zero_outputs(t, M, N, range(QE.TOKEN_CLASSES))
    assert sel.sum() >= 2 * N + 3 * (M - 2) - 8
    for tol in (O.summation_tol(aq, bq, s, t), O.reassoc_tol(aq, bq, s, t, waves=8), O.reassoc_tol(aq, bq, s, t, waves=16)):
        ratio = diff[sel] / tol[sel]
        print(f"t={t} k={k}: min |flushed - ref| / tol = {ratio.min():.3g}")
        assert (ratio > 1).all(), np.argwhere(sel & (diff <= tol))
    # nothing else moved, but the two rows of m = +-65504: their subnormal d is flushed too, and whether that shows
    # depends on the token (beyond the bound on the d_a = 65504 tokens, inside it on random ones) - why
    # q32_extremes.py counts them as range rows, not as subnormal ones
    if t in QE.HAS_M:
        sel[:, [QE.ROW_M_MAX_POS, QE.ROW_M_MAX_NEG]] = True
    assert (diff[~sel] == 0).all()


@pytest.mark.parametrize("t", QE.TYPES)
@pytest.mark.parametrize("k", KS)
def test_bounds_have_teeth_against_a_dropped_sign_of_d_a(O, t, k):
    """|d_a| in place of the negative d_a moves that token's outputs out of both bounds, on every row whose d part is
    there to be seen: not the rows of d = +-0, nor the row of unsigned codes 0, whose sumi is 0 (Q8_0's -128 codes
    keep it), nor (Q4_1 / Q5_1) the two rows whose m = +-65504 stands next to a subnormal d."""
    aq, bq, c, s = case(t, k)
    c_abs = O.gemm_w4a8(QE.abs_d_a(aq), bq, t)
    diff = np.abs(c_abs.astype(np.float64) - c)
    rows = np.ones(N, bool)
    rows[[QE.ROW_ZERO_POS, QE.ROW_ZERO_NEG]] = False
    if t != QE.Q8_0:
        rows[QE.ROW_MAX_CODE_MIN] = False
    if t in QE.HAS_M:
        rows[[QE.ROW_M_MAX_POS, QE.ROW_M_MAX_NEG]] = False
    for tol in (O.summation_tol(aq, bq, s, t), O.reassoc_tol(aq, bq, s, t, waves=8), O.reassoc_tol(aq, bq, s, t, waves=16)):
        ratio = diff[QE.TOK_NEG_D, rows] / tol[QE.TOK_NEG_D, rows]
        print(f"t={t} k={k}: min |abs - ref| / tol = {ratio.min():.3g}")
        assert (ratio > 1).all(), np.flatnonzero(rows)[ratio <= 1]
    other = np.ones(M, bool)
    other[[QE.TOK_NEG_D, QE.TOK_NEG_ZERO]] = False
    assert (diff[other] == 0).all()


@pytest.mark.parametrize("t", QE.TYPES)
@pytest.mark.parametrize("k", KS)
def test_host_twins_on_the_extremes(O, t, k):
    """qg_gemm_w4a8_cpu_mt and the single-format twins of tests/test_host_twins.py, through their own half_to_float."""
    import quant_gemm.host as H
    lib = H.load()
    aq, bq, c, s = case(t, k)
    tol = O.summation_tol(aq, bq, s, t)
    P = ctypes.c_void_p
    outs = [H.gemm_w4a8(aq, bq, M, N, k, t), H.gemm_w4a8(aq, bq, M, N, k, t, threads=5)]
    sym = {2: lib.qg_gemm_w4a8_q4_0_cpu, 8: lib.qg_gemm_w8a8_cpu}.get(t)
    if sym is not None:
        o = np.empty((M, N), np.float32)
        assert sym(P(aq.ctypes.data), P(bq.ctypes.data), P(o.ctypes.data), M, N, k) == 0
        outs.append(o)
        dot = lib.qg_vec_dot_q4_0_q8_1_cpu if t == 2 else lib.qg_vec_dot_q8_0_q8_1_cpu
        o = np.empty((M, N), np.float32)
        for i in range(M):
            for r in range(N):
                v = ctypes.c_float()
                dot(k, ctypes.byref(v), P(bq[r].ctypes.data), P(aq[i].ctypes.data))
                o[i, r] = v.value
        outs.append(o)
    for o in outs:
        assert np.isfinite(o).all()
        err = np.abs(o.astype(np.float64) - c)
        assert (err <= tol).all(), (err / tol).max()


@pytest.mark.parametrize("t", [2, 8])
@pytest.mark.parametrize("k", KS)
def test_w16_on_the_extreme_rows(O, t, k):
    """W4A16 / W8A16: the extreme weight rows on N(0, 1) activations stay finite, and flushing the subnormal d_w moves
    the subnormal rows by more than oracle.w16_tol."""
    _, bq, _, _ = case(t, k)
    a = np.random.default_rng([16, t, k]).standard_normal((5, k)).astype(np.float32)
    gemm = O.gemm_w4a16 if t == 2 else O.gemm_w8a16
    c = gemm(a, bq)
    assert np.isfinite(c).all()
    _, bqf = QE.flush_subnormals(t, np.zeros((1, k // 32, 36), np.uint8), bq)
    diff = np.abs(gemm(a, bqf).astype(np.float64) - c)
    tol = O.w16_tol(a, bq, t)
    rows = list(QE.SUBNORMAL_ROWS)
    assert (diff[:, rows] > tol[:, rows]).all(), (diff[:, rows] / tol[:, rows]).min()
    rest = np.ones(N, bool)
    rest[rows] = False
    assert (diff[:, rest] == 0).all()
