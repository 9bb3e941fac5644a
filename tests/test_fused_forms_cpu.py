"""The shape lists of tests/test_gpu_fused_forms.py against the kernel forms they are there for, without a GPU (the
pattern of tests/test_w16_shapes_cpu.py): the lists are imported, not copied, so a retune that moves a case to another
form, or an edit that moves a case to another K, fails here instead of leaving the GPU test to check less than it says.

The fused launch has no describe hook; every launch of a list is asked of qg_debug_config(..., algo = 1) as its Q8_1
twin, the same rows at the test's N. That names the fused kernel's form because the dispatch depends on the activation
input (AIN) in two places only:
  * gemv_form, csrc/qg_gemv_impl.hpp:58-59: the N >= 16384 rule (M = 1, K < 8192 to 512-thread workgroups) is
    `if constexpr (NRULE && MT == 1 && AIN == AIN_Q8_1)`; the fused variants fall through to W1 (line 64-65). No N of
    these lists but F32_MANY_ROWS' reaches it, and there the fused form is asked as the twin at N = 16383;
  * gemv_pick, csrc/qg_gemv_kernel.hpp:744-745: the grouped branch is `if constexpr (... AIN == AIN_Q8_1 ...) if
    (g.group)`, which a fused call never enters (run_fused sets no group; gemv_launch, line 822, refuses one).
Everything else of gemv_pick (the M = 1 entry, the short entry, the strided batch's half-size workgroups, ONEU) reads
M, K, N, batch and the output strides alone. (gemv_shape_ok, lines 643-646, asks 16-B aligned rows of a fused call and
refuses the parity hook; neither moves a form.)

Also here: run_fused's chunk rule restated (chunk_rows, from gemv_shape_ok's LDS test) picks the chunk sizes the GPU
tests name, and the generated activations keep to the quantizer's domain (finite, no block whose 1 / d overflows)."""
import numpy as np
import pytest

import test_gpu_fused_forms as F
from test_gemv_pick_cpu import bind
from test_gpu_q32_extremes import field, gemv_form

TYPES = F.TYPES
SMALL = {(2, 8, 256), (4, 4, 256), (2, 16, 256), (2, 32, 512)}  # the K < 4096 forms of M <= 4 (launch_staged)
FORMS = SMALL | {(2, 64, 512), (2, 64, 1024), (4, 32, 512)}


@pytest.fixture(scope="module")
def so():
    import quant_gemm._lib as L
    return bind(L.load())


def twin(so, t, m, n, k):
    """(MT, BPL, LPR, WGS, loop-free, ONEU) of the Q8_1 GEMV on m rows; the restated gemv_form must agree"""
    import ctypes
    buf = ctypes.create_string_buffer(256)
    assert so.qg_debug_config(m, n, k, t, 1, 0, buf, 256) == 0, (t, m, n, k)
    cfg = buf.value.decode()
    assert cfg.startswith("gemv ") and " AIN=0 " in cfg, cfg
    got = tuple(int(field(cfg, x)) for x in ("MT", "BPL", "LPR", "WGS")) + (field(cfg, "ONEU") != "0",)
    assert got == gemv_form(t, m, n, k), (cfg, gemv_form(t, m, n, k))
    return got + (int(field(cfg, "ONEU")),)


def f32_launches():
    """(t, rows, n, k) of every fused GEMV launch the FP32 tests make"""
    out = set()
    for t in TYPES:
        for m, k in F.F32_SINGLE:
            for ws in (False, True):
                out |= {(t, r1 - r0, F.n_of(t, k), k) for r0, r1 in F.fused_launches(m, k, ws) or []}
    for t, m, n, k, rows in F.F32_CHUNKED:
        out |= {(t, r1 - r0, n, k) for r0, r1 in F.fused_launches(m, k, False)}
    return out


def f16_launches():
    out = set()
    for cases, wss in ((F.F16_SINGLE, (False, True)), (F.F16_CHUNKED, (False,))):
        for ntok, k in cases:
            for ws in wss:
                out |= {(F.Q4_0, r1 - r0, F.n_of(F.Q4_0, k), k) for r0, r1 in F.fused_launches(ntok, k, ws) or []}
    return out


def test_fp32_lists_meet_every_form(so):
    seen = {(t,) + twin(so, t, m, n, k) for t, m, n, k in f32_launches()}
    assert {x[1] for x in seen} == {1, 2, 4, 8}
    assert {x[2:5] for x in seen} == FORMS
    assert {x[2:6] for x in seen} == {f + (lf,) for f in FORMS for lf in (True, False)}
    for t in TYPES:
        for mt in (1, 2, 4):  # every form of the M tile, loop-free and with the unit loop, in every format
            mine = {x[2:6] for x in seen if x[0] == t and x[1] == mt}
            # (Q4_0 at M = 1 has no unit loop below K = 16384: two or four units a lane run loop-free, ONEU = 2 / 4)
            lfs = (True,) if (t, mt) == (F.Q4_0, 1) else (True, False)
            assert {x for x in mine if x[:3] in SMALL} == {f + (lf,) for f in SMALL for lf in lfs}, (t, mt)
            assert {x[:2] + x[3:] for x in mine if x[:3] not in SMALL} == {(2, 64, True), (2, 64, False)}, (t, mt)
        # MT = 8 (K = 192, 1024, 6144): (2, 8, 256) is loop-free only (K <= 512), (4, 4, 256) at K = 1024 has the loop;
        # the loop-free (4, 32, 512) is K = 4096, the strided batch of M = 16 (and test_f32_fused_bit_identical_to_two_step)
        assert {x[2:6] for x in seen if x[0] == t and x[1] == 8} - {(4, 32, 512, True)} == \
            {(2, 8, 256, True), (4, 4, 256, False), (4, 32, 512, False)}, t
    assert {x[0] for x in seen if x[1:6] == (8, 4, 32, 512, True)} == {F.Q4_0, F.Q5_1}
    # FP32 prologue in gemv1_kernel's multi-unit forms (Q4_0, M = 1)
    assert {x[6] for x in seen if x[0] == F.Q4_0 and x[1] == 1} == {0, 1, 2, 4}
    # K > 4096 with the unit loop at M >= 2: the 512-thread workgroups of the byte-decode formats, whose staging loop runs
    # more than once there (K = 8192, M = 2: 512 blocks), and Q4_1's 1024-thread ones
    for t in TYPES[1:]:
        assert {x[4] for x in seen if x[0] == t and x[1] in (2, 4) and x[2:4] == (2, 64) and not x[5]} == \
            {1024 if t == F.Q4_1 else 512}


def test_fp16_lists_meet_every_form(so):
    seen = {twin(so, t, m, n, k) for t, m, n, k in f16_launches()}
    assert {x[0] for x in seen} == {1, 2, 4, 8}
    assert {x[5] for x in seen if x[0] == 1} == {0, 1, 2, 4}
    for mt in (1, 2, 4):
        assert {x[1:3] for x in seen if x[0] == mt} == {f[:2] for f in SMALL} | {(2, 64)}
        assert {x[4] for x in seen if x[0] == mt and x[1:3] == (2, 64)} == {True, False}
    for mt in (2, 4):
        assert all(not x[4] for x in seen if x[0] == mt and x[1:4] in SMALL)  # K = 576 .. 3072: the unit loop
    assert {x[1:5] for x in seen if x[0] == 8} == {(4, 4, 256, False), (4, 32, 512, False)}
    assert any(k > 2048 and not twin(so, t, m, n, k)[4] for t, m, n, k in f16_launches())


def test_named_cases_are_where_they_say(so):
    units = lambda k, bpl, lpr: -(-(k // 32 // bpl) // lpr)
    assert (1, 4160) in F.F32_SINGLE and 4160 // 64 == 65 and units(4160, 2, 64) == 2
    assert twin(so, F.Q4_0, 1, 19, 4160)[1:] == (2, 64, 1024, True, 2)
    assert all(twin(so, t, 1, 19, 4160)[1:3] + twin(so, t, 1, 19, 4160)[4:] == (2, 64, False, 0) for t in TYPES[1:])
    # the published decode K = 14336: 224 units on 64 lanes, a partial last round
    assert {(1, 14336), (2, 14336), (3, 576), (2, 3072)} <= set(F.F32_SINGLE) and 14336 // 64 % 64 == 32
    assert twin(so, F.Q4_0, 1, 19, 8192)[5] == 2 and twin(so, F.Q4_0, 1, 19, 14336)[5] == 4
    assert twin(so, F.Q4_0, 1, 19, 32768)[5] == 0
    assert twin(so, F.Q4_1, 3, 19, 576) == (4, 2, 8, 256, False, 0)
    assert twin(so, F.Q5_0, 2, 19, 3072) == (2, 2, 32, 512, False, 0)
    assert twin(so, F.Q8_0, 2, 19, 14336) == (2, 2, 64, 512, False, 0)
    # (3, 32768): three rows of records exceed 96 KiB
    assert (3, 32768) in F.F32_SINGLE and not F.gemv_shape_ok(3, 32768) and F.gemv_shape_ok(2, 32768)
    assert F.fused_launches(3, 32768, False) == [(0, 2), (2, 3)] and F.fused_launches(3, 32768, True) is None
    for m, k in F.F32_SINGLE:
        assert m <= 4 and ((m, k) == (3, 32768) or F.fused_launches(m, k, False) == F.fused_launches(m, k, True) == [(0, m)])
    assert all(19 <= F.n_of(t, k) <= 33 for t in TYPES for _, k in F.F32_SINGLE)  # test_row_gemv's rule


def test_many_rows_twin_and_fused_form_differ_as_said(so):
    for t, m, n, k in F.F32_MANY_ROWS:
        assert (m, n >= 16384, k < 8192) == (1, True, True)
        assert twin(so, t, m, n, k)[:5] == (1, 2, 64, 512, True)                      # the N >= 16384 rule
        w1 = twin(so, t, m, n - 1, k)[:5]                                              # one row fewer: W1
        assert w1 == F.fused_form(t, m, k) == (1, 2, 64, 1024 if t == F.Q4_0 else 512, True)
    assert {t for t, *_ in F.F32_MANY_ROWS} == {F.Q4_0, F.Q5_0}  # one format whose W1 differs from the rule's 512, one not


def test_chunk_rule_picks_the_named_chunks(so):
    """gemv_shape_ok restated: M > 2 and M * units * REC_DW * 4 > 96 KiB, the unit size from K/32 % 4 as ok_f."""
    assert F.REC_DW == {2: 12 * 2 + 4, 4: 12 * 4 + 4} and F.LDS_LIMIT == 98304
    assert F.gemv_shape_ok(8, 7168) and not F.gemv_shape_ok(8, 7680)     # "M = 8 from K = 7680 on"
    assert F.gemv_shape_ok(4, 14336) and not F.gemv_shape_ok(4, 16384)   # M = 4 at K = 16384
    assert not F.gemv_shape_ok(9, 1024) and not F.gemv_shape_ok(1, 96) and F.gemv_shape_ok(2, 1 << 20)
    for t, m, n, k, rows in F.F32_CHUNKED:
        assert F.chunk_rows(m, k) == rows, (m, k)
        assert m > 4 or not F.gemv_shape_ok(m, k)  # a chunk test, not the single launch
        # the library agrees on what is eligible: the forced GEMV takes `rows` rows and refuses the next larger chunk
        import ctypes
        buf = ctypes.create_string_buffer(256)
        assert so.qg_debug_config(min(rows, m), n, k, t, 1, 0, buf, 256) == 0
        if rows < 8 and m >= 2 * rows:
            assert so.qg_debug_config(min(2 * rows, m), n, k, t, 1, 0, buf, 256) == -3
    by = lambda m, k: [r1 - r0 for r0, r1 in F.fused_launches(m, k, False)]
    assert by(13, 8192) == [4, 4, 4, 1] and by(4, 16384) == [2, 2] and by(7, 16384) == [2, 2, 2, 1]
    assert by(16, 4096) == [8, 8] and by(16, 1024) == [8, 8] and by(6, 6144) == [6] and by(5, 192) == [5]
    assert {(m, k) for _, m, _, k, r in F.F32_CHUNKED if r == 8 and m <= 8} == {(m, k) for m in (5, 6, 8) for k in (192, 1024, 6144)}
    assert {r for *_, r in F.F32_CHUNKED} == {8, 4, 2}
    # M = 16, N = 4112: more row tiles than one round of full-size workgroups (256 compute units), so the batch runs the
    # full-size form; the small-N batch of M = 16 the half-size two-tile one
    rpb = lambda f: (f[3] // 64) * (64 // f[2])
    big = [c for c in F.F32_CHUNKED if c[2] == 4112]
    assert {c[0] for c in big} == {F.Q4_0, F.Q5_1}
    for t, m, n, k, rows in big:
        f = twin(so, t, rows, n, k)
        assert f[:5] == (8, 4, 32, 512, True) and -(-n // rpb(f)) > 256
    t, m, n, k, rows = F.F32_CHUNKED[-1]
    assert (t, m, k) == (F.Q4_0, 16, 1024) and -(-n // rpb(twin(so, t, rows, n, k))) <= 256
    # FP16
    assert [by(13, k) for k in (1024, 6144, 8192)] == [[8, 5], [8, 5], [4, 4, 4, 1]]
    assert all(by(6, k) == [6] for k in (1024, 6144, 8192))
    assert by(3, 32768) == [2, 1] and by(4, 32768) == [2, 2]


def test_fp16_single_launches_have_the_gemv_as_two_step_twin(so):
    """test_f16_single_launch compares an eligible N_tok <= 4 with the reference's two-step entry, whose auto dispatch
    must then be the row GEMV."""
    for ntok, k in F.F16_SINGLE:
        if F.fused_launches(ntok, k, True) is not None:
            assert so.qg_select_algo(ntok, F.n_of(F.Q4_0, k), k, F.Q4_0) == 1, (ntok, k)
    assert [c for c in F.F16_SINGLE if F.fused_launches(*c, True) is None] == [(3, 32768), (4, 32768)]


def test_generated_activations_keep_to_the_quantizers_domain(O):
    """Finite, and no block whose 1 / d overflows (0 < amax < ~3.7e-37): there the reference converts NaN to int, which
    C leaves undefined — the exclusion of test_q8_1_quantizer_extreme_scales. Every source really is in every list."""
    cases = {(m, k, F.start_of(t, i)) for t in TYPES for i, (m, k) in enumerate(F.F32_SINGLE)}
    cases |= {(m, k, F.start_of(t, 3)) for t, m, n, k in F.F32_MANY_ROWS}
    cases |= {(m, k, F.start_of(t, i)) for i, (t, m, n, k, r) in enumerate(F.F32_CHUNKED)}
    f16 = {(m, k, i) for i, (m, k) in enumerate(F.F16_SINGLE)} | {(m, k, 2 + i) for i, (m, k) in enumerate(F.F16_CHUNKED)}
    for m, k, start in sorted(cases | f16):
        x = F.activation_rows(m, k, start)
        assert x.shape == (m, k) and x.dtype == np.float32 and np.isfinite(x).all()
        amax = np.abs(x.reshape(-1, 32)).max(axis=1)
        assert ((amax > 3.7e-37) | (amax == 0)).all()
        if (m, k, start) in f16:
            h = x.astype(np.float16)
            assert np.isfinite(h).all() and np.isfinite(h.astype(np.float32).reshape(-1, 32).sum(axis=1, dtype=np.float32)).all()
    for i, (m, k) in enumerate(F.F32_SINGLE):  # at M = 1 every case meets every source across the five formats
        if m == 1:
            assert {F.start_of(t, i) % 5 for t in TYPES} == set(range(5))
    # the sources are what they say: the scaled rows emit subnormal, zero and large d, the edge row holds a zero block
    aq = O.quantize(np.stack([F.activation_rows(1, 1024, s)[0] for s in range(5)]), O.Q8_1)
    d = np.ascontiguousarray(aq[..., 0:2]).view(np.float16)[..., 0].astype(np.float64)
    assert ((d[1] > 0) & (d[1] < 2.0 ** -14)).all() and (d[2] == 0).all() and (d[3] > 100).all()
    assert (d[4] == 0).any() and (d[4] > 1).any() and F.SOURCES == ("step4", "sub_d", "zero_d", "large_d", "edge")
