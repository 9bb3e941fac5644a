"""Q8_1 activations and Q4_0 / Q4_1 / Q5_0 / Q5_1 / Q8_0 weights at the ends of their f16 scale formats, for the
32-element product kernels (tests/test_q32_extremes_cpu.py, tests/test_gpu_q32_extremes.py). NumPy only.

The pattern of tests/kquant_ref.py:extremes: one class per weight row and one per activation token, so every output
(token class x row class) is homogeneous in magnitude and a bound relative to the output's own sum |term| cannot hide
one class under another. Finite values only: Inf and NaN scales are out of scope (the contract of include/qg/qg.h says
nothing about them).
"""
from __future__ import annotations

import numpy as np

from kquant_ref import F16_MAX, F16_MIN_NORMAL, F16_SUBNORMALS

Q4_0, Q4_1, Q5_0, Q5_1, Q8_0 = 2, 3, 6, 7, 8
TYPES = (Q4_0, Q4_1, Q5_0, Q5_1, Q8_0)
BB = {Q4_0: 18, Q4_1: 20, Q5_0: 22, Q5_1: 24, Q8_0: 34}
HAS_M = (Q4_1, Q5_1)
QS_OFF = {Q4_0: 2, Q4_1: 4, Q5_0: 6, Q5_1: 8, Q8_0: 2}
QH_OFF = {Q5_0: 2, Q5_1: 4}

# Weight row classes (the row index is the class). Rows 9..12 exist for Q4_1 / Q5_1 only; for the other formats, and
# from EXTREME_ROWS on for every format, rows are random_blocks rows.
ROW_SUB_POS, ROW_SUB_NEG, ROW_SUB_CYCLE, ROW_MIN_NORMAL, ROW_MAX_POS, ROW_MAX_NEG, ROW_MAX_CODE_MIN, ROW_ZERO_POS, \
    ROW_ZERO_NEG, ROW_M_SUB, ROW_M_MAX_POS, ROW_M_MAX_NEG, ROW_M_ZERO = range(13)
EXTREME_ROWS = 13
# Activation token classes
TOK_SUB, TOK_SUB_CYCLE, TOK_MAX_NEG, TOK_MAX_POS, TOK_NEG_D, TOK_NEG_ZERO = range(6)
TOKEN_CLASSES = 6

# rows / tokens whose every d (or, ROW_M_SUB, every m) is an f16 subnormal that the output depends on visibly: with
# these fields flushed to zero the output must leave the bound (test_q32_extremes_cpu.py, "teeth")
SUBNORMAL_ROWS = (ROW_SUB_POS, ROW_SUB_NEG, ROW_SUB_CYCLE)
SUBNORMAL_TOKENS = (TOK_SUB, TOK_SUB_CYCLE)
# the largest |term| extremes() can produce: d_w = d_a = 65504 and a Q8_0 block of -128 codes on qs = -128
MAX_TERM = 65504.0 * 65504.0 * (128 * 128 * 32)  # 2.25e15


def row_classes(t: int) -> int:
    """The number of weight row classes of format t: 13 with an m field, 9 without."""
    return EXTREME_ROWS if t in HAS_M else ROW_M_SUB


def subnormal_rows(t: int):
    return SUBNORMAL_ROWS + ((ROW_M_SUB,) if t in HAS_M else ())


def f16_bytes(x) -> np.ndarray:
    x = np.asarray(x, np.float64)
    return np.ascontiguousarray(x.astype(np.float16)).view(np.uint8).reshape(x.shape + (2,))


def f16_field(b: np.ndarray, off: int) -> np.ndarray:
    """The f16 at byte `off` of every block, as float64 (signs of zero kept)."""
    return np.ascontiguousarray(b[..., off:off + 2]).view(np.float16)[..., 0].astype(np.float64)


def set_codes(t: int, row: np.ndarray, code: int) -> None:
    """Every element of the blocks `row` [..., BB] to the unsigned code (Q4: 0..15, Q5: 0..31) or, Q8_0, to the signed
    byte `code`."""
    o = QS_OFF[t]
    if t == Q8_0:
        row[..., o:o + 32] = np.uint8(code & 0xFF)
        return
    row[..., o:o + 16] = np.uint8((code & 15) * 0x11)
    if t in QH_OFF:
        row[..., QH_OFF[t]:QH_OFF[t] + 4] = 0xFF if code & 16 else 0


def codes(t: int, b: np.ndarray) -> np.ndarray:
    """int32 [..., 32]: the stored code of every element (unsigned for Q4 / Q5, signed for Q8_0), elements 0..15 in the
    low nibbles, 16..31 in the high ones, bit 4 of element e at bit e of qh."""
    o = QS_OFF[t]
    if t == Q8_0:
        return np.ascontiguousarray(b[..., o:o + 32]).view(np.int8).astype(np.int32)
    qs = b[..., o:o + 16].astype(np.int32)
    q = np.concatenate([qs & 15, qs >> 4], axis=-1)
    if t in QH_OFF:
        qh = np.ascontiguousarray(b[..., QH_OFF[t]:QH_OFF[t] + 4]).view(np.uint32)[..., 0].astype(np.int64)
        q = q | ((((qh[..., None] >> np.arange(32)) & 1) << 4).astype(np.int32))
    return q


def code_range(t: int):
    """(minimum, maximum) stored code."""
    return (-128, 127) if t == Q8_0 else (0, 31) if t in QH_OFF else (0, 15)


def extremes(rng, t: int, m: int, n: int, k: int, tokens=None):
    """Q8_1 [m, k/32, 36] and weights of format t [n, k/32, BB[t]] at the ends of the f16 scale formats. Finite values
    only (no Inf, no NaN). The largest |term| is MAX_TERM = 65504^2 * 128 * 128 * 32 = 2.25e15 (Q8_0), far inside fp32.
    `sub` below is kquant_ref.F16_SUBNORMALS (2^-24, 3 2^-24, 2^-20, 2^-15, 1023 2^-24) cycled along the blocks and
    `alt` a sign that alternates along them.

    Weight rows (n >= EXTREME_ROWS; codes random unless stated; m is the second f16 of Q4_1 / Q5_1):
      0  d = +2^-24 in every block, m = +2^-24        1  d = -2^-24, m = +2^-24
      2  d = sub * alt, m = sub (two blocks on) * -alt
      3  d = 2^-14 * alt, m = -2^-14 * alt
      4  d = +65504, every code at its maximum (nibble 15 / Q5 31 with all qh bits / Q8_0 +127), m = +65504
      5  d = -65504, maximum codes, m = +65504
      6  d = +65504, every code at its minimum (nibble 0 / Q5 0 / Q8_0 -128), m = -65504
      7  d = +0, m random                             8  d = -0, m random
    and, Q4_1 / Q5_1 only (rows of the other formats from 9 on are random):
      9  m = sub, negative in every third block (so its sum does not cancel), with the normal d = 2^-13 * alt;
         element 0 of every block has code 1 and every other element code 0, so sumi is one activation byte and
         neither part of the term hides the other for any token class
     10  m = +65504 with d = sub * alt               11  m = -65504 with d = sub * -alt
         (range rows, not among subnormal_rows(): next to such an m the part of the subnormal d is inside the bounds
         for most tokens)
     12  m = +0, d random
    Rows from EXTREME_ROWS on are random_blocks rows (d in +-0.1, m in +-0.5).

    Activation tokens; token i of the result is class tokens[i] (default 0, 1, 2, ...), tokens past len(tokens) are
    random_blocks tokens (d_a in [1e-3, 2e-2], s_a in +-5); qs random unless stated:
      0  d_a = s_a = 2^-24 in every block
      1  d_a = sub, s_a = sub (three blocks on), negative in every third block
      2  d_a = 65504, qs = -128, s_a = -65504         3  d_a = 65504, qs = +127, s_a = +65504
      4  d_a = -(a random normal f16 in [1e-3, 2e-2]), s_a random in +-5
      5  d_a = -0, s_a random in +-5
    """
    from test_gpu_product import random_blocks
    assert t in TYPES and n >= EXTREME_ROWS and k % 32 == 0
    tokens = tuple(range(min(m, TOKEN_CLASSES))) if tokens is None else tuple(tokens)
    assert len(tokens) <= m and all(0 <= c < TOKEN_CLASSES for c in tokens)
    nb = k // 32
    aq, bq = random_blocks(rng, m, n, k, t)
    j = np.arange(nb)
    sub = np.array(F16_SUBNORMALS)
    alt = np.where(j % 2 == 0, 1.0, -1.0)
    lo, hi = code_range(t)

    def put(r, d, mw=None):
        bq[r, :, 0:2] = f16_bytes(np.broadcast_to(d, (nb,)))
        if t in HAS_M and mw is not None:
            bq[r, :, 2:4] = f16_bytes(np.broadcast_to(mw, (nb,)))

    put(ROW_SUB_POS, 2.0 ** -24, 2.0 ** -24)
    put(ROW_SUB_NEG, -2.0 ** -24, 2.0 ** -24)
    put(ROW_SUB_CYCLE, sub[j % 5] * alt, -sub[(j + 2) % 5] * alt)
    put(ROW_MIN_NORMAL, F16_MIN_NORMAL * alt, -F16_MIN_NORMAL * alt)
    put(ROW_MAX_POS, F16_MAX, F16_MAX)
    put(ROW_MAX_NEG, -F16_MAX, F16_MAX)
    put(ROW_MAX_CODE_MIN, F16_MAX, -F16_MAX)
    set_codes(t, bq[ROW_MAX_POS], hi)
    set_codes(t, bq[ROW_MAX_NEG], hi)
    set_codes(t, bq[ROW_MAX_CODE_MIN], lo)
    put(ROW_ZERO_POS, 0.0)
    put(ROW_ZERO_NEG, -0.0)
    if t in HAS_M:
        put(ROW_M_SUB, 2.0 ** -13 * alt, sub[j % 5] * np.where(j % 3 == 0, -1.0, 1.0))
        set_codes(t, bq[ROW_M_SUB], 0)
        bq[ROW_M_SUB, :, QS_OFF[t]] = 1  # element 0: code 1
        put(ROW_M_MAX_POS, sub[j % 5] * alt, F16_MAX)
        put(ROW_M_MAX_NEG, -sub[(j + 1) % 5] * alt, -F16_MAX)
        bq[ROW_M_ZERO, :, 2:4] = f16_bytes(np.zeros(nb))

    for i, c in enumerate(tokens):
        if c == TOK_SUB:
            aq[i, :, 0:2] = aq[i, :, 2:4] = f16_bytes(np.full(nb, 2.0 ** -24))
        elif c == TOK_SUB_CYCLE:
            aq[i, :, 0:2] = f16_bytes(sub[j % 5])
            aq[i, :, 2:4] = f16_bytes(sub[(j + 2) % 5] * np.where(j % 3 == 0, -1.0, 1.0))
        elif c in (TOK_MAX_NEG, TOK_MAX_POS):
            s = -1.0 if c == TOK_MAX_NEG else 1.0
            aq[i, :, 0:2] = f16_bytes(np.full(nb, F16_MAX))
            aq[i, :, 2:4] = f16_bytes(np.full(nb, s * F16_MAX))
            aq[i, :, 4:36] = 0x80 if c == TOK_MAX_NEG else 0x7F
        elif c == TOK_NEG_D:
            aq[i, :, 1] |= 0x80  # the sign bit of d_a; random_blocks drew a normal |d_a|
        else:
            aq[i, :, 0:2] = f16_bytes(np.full(nb, -0.0))
    return aq, bq


def flush_subnormals(t: int, aq: np.ndarray, bq: np.ndarray):
    """Copies of (aq, bq) with every f16 subnormal d_w, m_w, d_a and s_a replaced by a zero of its sign: what a kernel
    that flushed subnormal f16 inputs would compute on."""
    aq, bq = aq.copy(), bq.copy()
    for b, offs in ((aq, (0, 2)), (bq, (0, 2) if t in HAS_M else (0,))):
        for o in offs:
            h = np.ascontiguousarray(b[..., o:o + 2]).view(np.uint16)[..., 0]
            sub = (h & 0x7C00) == 0
            b[..., o][sub] = 0
            b[..., o + 1][sub] &= 0x80
    return aq, bq


def abs_d_a(aq: np.ndarray) -> np.ndarray:
    """A copy of aq with |d_a| in place of d_a: what a kernel that dropped the sign of d_a would compute on."""
    aq = aq.copy()
    aq[..., 1] &= 0x7F
    return aq


def zero_outputs(t: int, m: int, n: int, tokens) -> np.ndarray:
    """bool [m, n]: the outputs of extremes() that are zero by construction (every term is): a row of d = +-0 without
    an m field; for Q8_0 the token of d_a = -0; for Q4_1 / Q5_1 that token on the row of m = 0."""
    z = np.zeros((m, n), bool)
    if t not in HAS_M:
        z[:, [ROW_ZERO_POS, ROW_ZERO_NEG]] = True
    for i, c in enumerate(tokens):
        if c == TOK_NEG_ZERO:
            if t == Q8_0:
                z[i, :] = True
            if t in HAS_M:
                z[i, ROW_M_ZERO] = True
    return z
