"""Every 32-element kernel family at the ends of the f16 scale formats (tests/q32_extremes.py): subnormal, smallest
normal, +-65504 and zero d_w / m_w / d_a / s_a, negative d_a — the scale epilogues that the band of random_blocks
(d_a in [1e-3, 2e-2], |d_w| <= 0.1) never exercises.

One harness for every case: the product is launched into the interior of a sentinel-filled buffer (every sentinel must
survive), twice (identical bits), the family is read from the qg_debug_config* string, and the result is compared with
the oracle under the bound that family's own test file uses (oracle.summation_tol for the GEMV, ragged, generic and
tiled decode GEMV kernels, whose per-block terms are the oracle's bit for bit; oracle.reassoc_tol for the MFMA
families). tests/test_q32_extremes_cpu.py shows that a kernel flushing the subnormal scales, or dropping the sign of
d_a, leaves those bounds on these inputs. Each case prints its max err / tol (profiles/q32_extremes/README.md).
"""
import ctypes
import functools
import re

import numpy as np
import pytest

import q32_extremes as QE
from test_gpu_product import dev, host

pytestmark = pytest.mark.gpu

TYPES = list(QE.TYPES)
SENT = -7.0   # sentinel around every output
PAD = 5       # columns (ldc entries) ...
GUARD = 64    # ... or floats on either side (dense entries) that must keep it
P = ctypes.c_void_p


@functools.lru_cache(maxsize=24)
def operands(t, m, n, k, tokens=None, both_ends=False, salt=0):
    """(aq, bq, c_ref, sumi) of one case, read-only. both_ends: the class rows again as the last rows of N."""
    import oracle as O
    aq, bq = QE.extremes(np.random.default_rng([t, m, n, k, salt]), t, m, n, k, tokens=tokens)
    if both_ends:
        bq[n - QE.EXTREME_ROWS:] = bq[:QE.EXTREME_ROWS]
    c, s = O.gemm_w4a8(aq, bq, t, want_sumi=True)
    for x in (aq, bq, c, s):
        x.setflags(write=False)
    return aq, bq, c, s


def rotate(m, rot):
    """The token classes of an M < 6 case: m consecutive classes starting at rot."""
    return None if m >= QE.TOKEN_CLASSES else tuple((rot + i) % QE.TOKEN_CLASSES for i in range(m))


def stream():
    import torch
    return P(torch.cuda.current_stream().cuda_stream)


def guarded_run(m, n, launch, dense=False):
    """launch(view, ldc) twice, each into the interior of a fresh sentinel-filled buffer: [1:m+1, :n] of [m+2, n+PAD]
    floats, or (dense: the entry takes no row stride) floats GUARD .. GUARD + m n of a flat one. Every sentinel
    survives, the two results are the same bits; returns the result [m, n]."""
    import torch
    outs = []
    for _ in range(2):
        if dense:
            big = torch.full((2 * GUARD + m * n,), SENT, dtype=torch.float32, device="cuda")
            view, ldc = big[GUARD:GUARD + m * n].view(m, n), n
        else:
            big = torch.full((m + 2, n + PAD), SENT, dtype=torch.float32, device="cuda")
            view, ldc = big[1:m + 1, :n], n + PAD
        try:
            launch(view, ldc)
            g = host(big).copy()
        except RuntimeError as e:  # a HIP error poisons the context: end the run, launch nothing more
            if "HIP" in str(e) or "hip" in str(e):
                pytest.exit(f"HIP error, run ended: {e}", returncode=3)
            raise
        inner = g[GUARD:GUARD + m * n] if dense else g[1:m + 1, :n]
        outs.append(inner.reshape(m, n).copy())
        inner[...] = SENT
        assert (g == SENT).all(), f"{int((g != SENT).sum())} sentinels overwritten"
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "two launches differ"
    return outs[0]


def report(label, c, c_ref, tol):
    assert np.isfinite(c).all(), f"{label}: non-finite output at {np.argwhere(~np.isfinite(c))[:8].tolist()}"
    err = np.abs(c.astype(np.float64) - c_ref)
    ratio = err / tol
    print(f"q32x {label}: max err/tol = {ratio.max():.3g}")
    bad = np.argwhere(err > tol)
    assert bad.size == 0, f"{label}: max err/tol {ratio.max():.3g}; (token, row) {bad[:12].tolist()} of {len(bad)}"


def bound(O, kind, aq, bq, s, t):
    return O.summation_tol(aq, bq, s, t) if kind == "sum" else O.reassoc_tol(aq, bq, s, t, waves=kind)


def via_gemm_w4a8(qg, a, b, m, n, k, t, algo):
    return guarded_run(m, n, lambda view, ldc: qg.gemm_w4a8(a, b, m, n, k, t, algo=algo, out=view))


def field(cfg, name):
    return re.search(rf"\b{name}=(\w+)", cfg).group(1)


# ------------------------------------------------------------------------------------------------ row GEMV (algo = 1)
def gemv_form(t, m, n, k):
    """(MT, BPL, LPR, WGS, loop-free) of launch_staged (csrc/qg_gemv_impl.hpp), restated."""
    nb = k // 32
    mt = 1 if m <= 1 else 2 if m <= 2 else 4 if m <= 4 else 8
    byte_fmt = t in (6, 7, 8)
    if mt <= 4 and nb % 2 == 0 and nb // 2 >= 64:
        if mt == 1 and n >= 16384 and k < 8192:
            f = (2, 64, 512)
        elif mt == 1 and nb // 2 <= 64:
            f = (2, 64, 512 if t in (6, 7) else 1024)
        elif mt == 1:
            f = (2, 64, 512 if t == 8 else 1024)
        else:
            f = (2, 64, 512 if byte_fmt else 1024)
    elif mt <= 4 and nb % 2 == 0 and nb // 2 >= 32:
        f = (2, 32, 512)
    elif mt <= 4 and nb % 2 == 0 and nb // 2 >= 16:
        f = (2, 16, 256)
    elif nb % 4 == 0:
        f = (4, 32, 512) if nb // 4 >= 32 else (4, 4, 256)
    else:
        f = (2, 8, 256)
    units = -(-(nb // f[0]) // f[1])  # units per lane
    # more than one unit per lane: the unit loop, but Q4_0 at M = 1 unrolls 2 or 4 units (ONEU = 2 / 4)
    loop_free = units == 1 or (t == 2 and mt == 1 and units <= 4)
    return (mt,) + f + (loop_free,)


# the issue's list (M = 1 at six K, M = 2..4 at K = 1024 and 4096, M = 8 at K = 4096) and, so that every form meets its
# unit loop too, M = 1 at K = 576 / 640 / 1536 / 3072 / 32768, M = 2..4 at K = 8192 and M = 8 at K = 192 / 1024 / 6144
GEMV_CASES = [(1, k) for k in (192, 512, 576, 640, 1024, 1536, 2048, 3072, 4096, 8192, 32768)] + \
             [(m, k) for m in (2, 3, 4) for k in (1024, 4096, 8192)] + [(8, k) for k in (192, 1024, 4096, 6144)]


def gemv_case(O, qg, t, m, n, k, rot, both_ends=False):
    cfg = qg.debug_config(m, n, k, t, algo=1)
    mt, bpl, lpr, wgs, loop_free = gemv_form(t, m, n, k)
    assert cfg.startswith(f"gemv F={t} MT={mt} BPL={bpl} LPR={lpr} WGS={wgs} AIN=0 "), cfg
    assert (field(cfg, "ONEU") != "0") == loop_free, cfg
    aq, bq, c_ref, s = operands(t, m, n, k, rotate(m, rot), both_ends)
    c = via_gemm_w4a8(qg, dev(aq), dev(bq), m, n, k, t, 1)
    report(f"gemv t={t} ({m},{n},{k}) MT={mt} BPL={bpl} LPR={lpr} WGS={wgs} ONEU={field(cfg, 'ONEU')}", c, c_ref,
           bound(O, "sum", aq, bq, s, t))
    return cfg


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("m,k", GEMV_CASES)
def test_row_gemv(O, qg, t, m, k):
    n = 19 + (t + k // 32) % 15  # 19 <= N <= 33
    gemv_case(O, qg, t, m, n, k, rot=t + GEMV_CASES.index((m, k)))


def test_row_gemv_many_rows(O, qg):
    """Q4_0, M = 1, N = 16384: the N >= 16384 form (512-thread workgroups), the class rows at both ends of N."""
    cfg = gemv_case(O, qg, 2, 1, 16384, 4096, rot=1, both_ends=True)
    assert " WGS=512 " in cfg and "grid=2048x1" in cfg, cfg


def test_row_gemv_cases_meet_every_form(qg):
    """Between them the cases name every unit size, lanes per row and workgroup size of launch_staged, each loop-free
    and with the unit loop, at every M tile."""
    seen = set()
    for t in TYPES:
        for m, k in GEMV_CASES + [(1, 4096)]:
            n = 16384 if (m, k) == (1, 4096) and t == 2 else 19
            cfg = qg.debug_config(m, n, k, t, algo=1)
            seen.add((int(field(cfg, "MT")), int(field(cfg, "BPL")), int(field(cfg, "LPR")), int(field(cfg, "WGS")),
                      field(cfg, "ONEU") != "0"))
    assert {x[0] for x in seen} == {1, 2, 4, 8}
    forms = {(2, 8, 256), (4, 4, 256), (2, 16, 256), (2, 32, 512), (2, 64, 512), (2, 64, 1024), (4, 32, 512)}
    assert {x[1:4] for x in seen} == forms
    assert {x[1:] for x in seen} == {f + (lf,) for f in forms for lf in (True, False)}
    for mt in (1, 2, 4):  # MT <= 4 takes the 2-block forms from K = 1024 on; MT = 8 never does
        assert {x[1:4] for x in seen if x[0] == mt} >= {(2, 16, 256), (2, 64, 512), (2, 64, 1024)}
    assert {x[1:] for x in seen if x[0] == 8} == {(2, 8, 256, True), (4, 4, 256, False), (4, 32, 512, True), (4, 32, 512, False)}


# ------------------------------------------------------------------------------------------------ MFMA rows (algo = 2)
def mmq_expect(t, m, n, k):
    """What the qg_debug_config string must hold for the MFMA row cases."""
    if (m, n, k) == (9, 33, 128):  # the 4-B DMA variant, where a stage's row segment (4 blocks) is no multiple of 16 B;
        return [f"P16={int(t in (3, 7))} "]  # Q4_1 / Q5_1 segments (80 / 96 B) always are: they keep 16-B pieces
    return {(9, 33, 1024): ["BN=16 TT=1 ", "P16=1 "], (32, 4096, 256): ["BN=32 TT=1 W=12 "],
            (33, 64, 256): ["BN=32 TT=2 W=8 "], (96, 4096, 256): ["BN=32 TT=2 W=4 "]}[(m, n, k)]


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("m,n,k", [(9, 33, 128), (9, 33, 1024), (32, 4096, 256), (33, 64, 256), (96, 4096, 256)])
def test_mfma_rows(O, qg, t, m, n, k):
    cfg = qg.debug_config(m, n, k, t, algo=2)
    assert cfg.startswith(f"mmq F={t} ") and " LAY=0 " in cfg and all(x in cfg for x in mmq_expect(t, m, n, k)), cfg
    aq, bq, c_ref, s = operands(t, m, n, k, None, n >= 64)
    c = via_gemm_w4a8(qg, dev(aq), dev(bq), m, n, k, t, 2)
    report(f"mmq t={t} ({m},{n},{k}) {cfg.split(' LAY')[0]}", c, c_ref, bound(O, 8, aq, bq, s, t))


@pytest.mark.parametrize("t", TYPES)
def test_mmql_rows_and_tiled(O, qg, t):
    """(520, 4010, 256): the large-M kernel on both weight layouts (one K slice per output: waves = 1)."""
    m, n, k = 520, 4010, 256
    aq, bq = QE.extremes(np.random.default_rng([t, m, n, k]), t, m, n, k)
    bq[n - QE.EXTREME_ROWS:] = bq[:QE.EXTREME_ROWS]
    c_ref, s = O.gemm_w4a8(aq, bq, t, want_sumi=True)
    tol = bound(O, 1, aq, bq, s, t)
    del s
    a, b = dev(aq), dev(bq)
    cfg = qg.debug_config(m, n, k, t, algo=2)
    assert cfg.startswith(f"mmql F={t} ") and " LAY=0 " in cfg, cfg
    report(f"mmql t={t} ({m},{n},{k}) LAY=0", via_gemm_w4a8(qg, a, b, m, n, k, t, 2), c_ref, tol)
    cfg = qg.debug_config_tiled(m, n, k, t)
    assert cfg.startswith(f"mmql F={t} ") and " LAY=1 " in cfg, cfg
    lib, bt = qg._lib.load(), qg.tile_weights(b, n, k, t)
    c = guarded_run(m, n, lambda view, ldc: qg._lib.check(lib.qg_gemm_w4a8_tiled_ldc(
        P(a.data_ptr()), P(bt.data_ptr()), P(view.data_ptr()), m, n, k, ldc, t, stream()), "tiled_ldc"))
    report(f"tiled_mmql t={t} ({m},{n},{k}) LAY=1", c, c_ref, tol)


# ------------------------------------------------------------------------------------------------ the other row families
@pytest.mark.parametrize("t", TYPES)
def test_repack_mfma(O, qg, t):
    """(32, 1024, 96): odd K/32 at a prefill size, the MFMA kernel on a zero-padded copy (qg_repack.hip)."""
    m, n, k = 32, 1024, 96
    assert qg.select_algo(m, n, k, t) == 2
    cfg = qg.debug_config(m, n, k, t)
    assert cfg.startswith(f"mmq F={t} ") and (k // 32) % 2 == 1, cfg
    aq, bq, c_ref, s = operands(t, m, n, k, None, True)
    c = via_gemm_w4a8(qg, dev(aq), dev(bq), m, n, k, t, 0)
    report(f"repack t={t} ({m},{n},{k})", c, c_ref, bound(O, 8, aq, bq, s, t))


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("m,n,k", [(3, 19, 96), (9, 19, 1056)])
def test_ragged(O, qg, t, m, n, k):
    assert qg.select_algo(m, n, k, t) == 4
    cfg = qg.debug_config(m, n, k, t)
    assert cfg.startswith(f"ragged F={t} MT={4 if m <= 4 else 8} "), cfg
    aq, bq, c_ref, s = operands(t, m, n, k, rotate(m, t))
    c = via_gemm_w4a8(qg, dev(aq), dev(bq), m, n, k, t, 0)
    report(f"ragged t={t} ({m},{n},{k})", c, c_ref, bound(O, "sum", aq, bq, s, t))


@pytest.mark.parametrize("t", TYPES)
def test_ragged_two_byte_aligned_weights(O, qg, t):
    """(4, 19, 1024) with the weights 2 B off a dword: the GEMV declines them and the ragged kernel serves the call
    (the same bits as algo = 4 on aligned bytes; qg_debug_config speaks of aligned buffers only)."""
    import torch
    m, n, k = 4, 19, 1024
    assert qg.debug_config(m, n, k, t, algo=4).startswith(f"ragged F={t} MT=4 ")
    aq, bq, c_ref, s = operands(t, m, n, k, rotate(m, t + 2))
    raw = torch.zeros(bq.size + 2, dtype=torch.uint8, device="cuda")
    raw[2:] = dev(bq.ravel())
    bmis = raw[2:].view(bq.shape)
    assert bmis.data_ptr() % 4 == 2
    a = dev(aq)
    c = via_gemm_w4a8(qg, a, bmis, m, n, k, t, 0)
    assert np.array_equal(c.view(np.uint32), via_gemm_w4a8(qg, a, dev(bq), m, n, k, t, 4).view(np.uint32))
    report(f"ragged t={t} ({m},{n},{k}) B%4=2", c, c_ref, bound(O, "sum", aq, bq, s, t))


@pytest.mark.parametrize("t", TYPES)
def test_generic(O, qg, t):
    m, n, k = 3, 19, 64
    assert qg.debug_config(m, n, k, t, algo=3).startswith(f"generic F={t} ")
    aq, bq, c_ref, s = operands(t, m, n, k, rotate(m, t + 3))
    c = via_gemm_w4a8(qg, dev(aq), dev(bq), m, n, k, t, 3)
    report(f"generic t={t} ({m},{n},{k})", c, c_ref, bound(O, "sum", aq, bq, s, t))


# ------------------------------------------------------------------------------------------------ tiled layout
TILED = [(1, 33, 1024, "gemvt", "sum"), (2, 33, 1024, "gemvt", "sum"), (3, 33, 1024, "gemvm", 16),
         (4, 33, 1024, "gemvm", 16), (16, 64, 256, "mmq", 16)]


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("m,n,k,fam,kind", TILED)
def test_tiled(O, qg, t, m, n, k, fam, kind):
    cfg = qg.debug_config_tiled(m, n, k, t)
    assert cfg.startswith(f"{fam} F={t} ") and (" LAY=1 " in cfg if fam == "mmq" else " TA=0 " in cfg), cfg
    aq, bq, c_ref, s = operands(t, m, n, k, rotate(m, t + m))
    lib, a, bt = qg._lib.load(), dev(aq), qg.tile_weights(dev(bq), n, k, t)
    c = guarded_run(m, n, lambda view, ldc: qg._lib.check(lib.qg_gemm_w4a8_tiled_ldc(
        P(a.data_ptr()), P(bt.data_ptr()), P(view.data_ptr()), m, n, k, ldc, t, stream()), "tiled_ldc"))
    report(f"{'tiled_mmq' if fam == 'mmq' else fam} t={t} ({m},{n},{k})", c, c_ref, bound(O, kind, aq, bq, s, t))


@pytest.mark.parametrize("t", TYPES)
def test_tiled_act(O, qg, t):
    """(5, 64, 256): the activations in the tiled layout too (LAY = 2)."""
    m, n, k = 5, 64, 256
    cfg = qg.debug_config_tiled_act(m, n, k, t)
    assert cfg.startswith(f"mmq F={t} ") and " LAY=2 " in cfg, cfg
    aq, bq, c_ref, s = operands(t, m, n, k, rotate(m, t))
    lib, at, bt = qg._lib.load(), qg.tile_activations(dev(aq), m, k), qg.tile_weights(dev(bq), n, k, t)
    c = guarded_run(m, n, lambda view, ldc: qg._lib.check(lib.qg_gemm_w4a8_tiled_act_ldc(
        P(at.data_ptr()), P(bt.data_ptr()), P(view.data_ptr()), m, n, k, ldc, t, stream()), "tiled_act_ldc"))
    report(f"tiled_act t={t} ({m},{n},{k})", c, c_ref, bound(O, 16, aq, bq, s, t))


# ------------------------------------------------------------------------------------------------ other entries
@pytest.mark.parametrize("t,sym", [(2, "qg_gemm_q4_0_q8_1"), (3, "qg_gemm_q4_1_q8_1"), (6, "qg_gemm_q5_0_q8_1"),
                                   (7, "qg_gemm_q5_1_q8_1"), (8, "qg_gemm_q8_0_q8_1")])
def test_weight_major(O, qg, t, sym):
    """gemm_q*_q8_1(W [19 rows], A [2 tokens], K = 1024) -> out[M_w][N_tok], dense: the C symbol, into a flat buffer."""
    mw, ntok, k = 19, 2, 1024
    assert qg.debug_config(ntok, mw, k, t).startswith(f"gemv F={t} MT=2 ")
    aq, bq, c_ref, s = operands(t, ntok, mw, k, rotate(ntok, t))
    lib, a, w = qg._lib.load(), dev(aq), dev(bq)
    out = guarded_run(mw, ntok, lambda view, ldc: qg._lib.check(getattr(lib, sym)(
        P(w.data_ptr()), P(a.data_ptr()), P(view.data_ptr()), mw, ntok, k, stream()), sym), dense=True)
    report(f"weight_major t={t} ({mw},{ntok},{k})", np.ascontiguousarray(out.T), c_ref, bound(O, "sum", aq, bq, s, t))


@pytest.mark.parametrize("t", TYPES)
def test_strided_batch(O, qg, t):
    """Three items at M = 1, K = 4096 in one launch, each with its own token class and its own weights."""
    n, k, nbatch = 19, 4096, 3
    assert qg.debug_config(1, n, k, t, algo=1).startswith(f"gemv F={t} MT=1 BPL=2 LPR=64 ")
    items = [operands(t, 1, n, k, ((2 * i + t) % QE.TOKEN_CLASSES,), salt=i) for i in range(nbatch)]
    a = dev(np.stack([it[0] for it in items]))
    w = dev(np.stack([it[1] for it in items]))
    lib = qg._lib.load()
    out = guarded_run(nbatch, n, lambda view, ldc: qg._lib.check(lib.qg_gemm_w4a8_strided_batched(
        P(a.data_ptr()), a[0].numel(), P(w.data_ptr()), w[0].numel(), P(view.data_ptr()), n, nbatch, 1, n, k, t,
        stream()), "strided_batched"), dense=True)
    for i, (aq, bq, c_ref, s) in enumerate(items):
        report(f"batched t={t} item {i} (1,{n},{k})", out[i:i + 1], c_ref, bound(O, "sum", aq, bq, s, t))


# ------------------------------------------------------------------------------------------------ FP32 / FP16 activations
SCALES = (1e-4, 1e-6, 3e4)


def scaled_rows(m, k, shift, seed):
    """float32 [m, k]: row i = SCALES[(i + shift) % 3] times values in [-1, 1] whose every block holds 15 pairs
    (v, -v) and two free values, shuffled: |sum of a block| <= 2 scale, so s_a = 6e4 at most stays finite in f16 at
    scale 3e4, where d_a = amax / 127 is large (about 236); at 1e-4 the quantizer emits subnormal d_a, and at 1e-6
    d_a = +0 (amax / 127 < 2^-25) next to subnormal s_a."""
    rng = np.random.default_rng([seed, m, k])
    v = rng.uniform(-1, 1, (m, k // 32, 15))
    blk = np.concatenate([v, -v, rng.uniform(-1, 1, (m, k // 32, 2))], axis=-1)
    blk = rng.permuted(blk, axis=-1)
    sc = np.array([SCALES[(i + shift) % 3] for i in range(m)])
    return (blk.reshape(m, k) * sc[:, None]).astype(np.float32)


def check_emitted_scales(aq, m, shift):
    da = QE.f16_field(aq, 0)
    sa = QE.f16_field(aq, 2)
    assert np.isfinite(da).all() and np.isfinite(sa).all()
    for i in range(m):
        sc = SCALES[(i + shift) % 3]
        if sc == 3e4:
            assert (da[i] > 100).all() and np.abs(sa[i]).max() > 1e4
        elif sc == 1e-4:
            assert ((da[i] > 0) & (da[i] < 2.0 ** -14)).all()
        else:
            assert (da[i] == 0).all() and ((sa[i] != 0) & (np.abs(sa[i]) < 2.0 ** -14)).any()


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("m,shift", [(1, 0), (1, 1), (1, 2), (4, 0), (12, 1)])
def test_f32_activations(O, qg, t, m, shift):
    """gemm_w4a8_f32 on rows whose device-side quantization emits subnormal and large d_a: M = 1 and 4 quantize in the
    GEMV prologue, M = 12 through the workspace. Bit-identical to quantize-then-product (tests/test_gpu_fused.py);
    the two-step result within the oracle's bound for the bytes the device quantizer wrote, which are the oracle's."""
    n, k = 19, 1024
    x = scaled_rows(m, k, shift, t)
    _, bq, _, _ = operands(t, 6, n, k)
    x_d, w_d = dev(x), dev(bq)
    aq_d = qg.quantize_q8_1(x_d)
    aq = host(aq_d)
    assert np.array_equal(aq, O.quantize(x, O.Q8_1))
    check_emitted_scales(aq, m, shift)
    two = via_gemm_w4a8(qg, aq_d, w_d, m, n, k, t, 0)
    lib = qg._lib.load()
    wsb = lib.qg_gemm_w4a8_f32_workspace_size(m, k)
    import torch
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    fused = guarded_run(m, n, lambda view, ldc: qg._lib.check(lib.qg_gemm_w4a8_f32(
        P(x_d.data_ptr()), P(w_d.data_ptr()), P(view.data_ptr()), m, n, k, t, P(ws.data_ptr()), wsb, stream()),
        "gemm_w4a8_f32"), dense=True)
    assert np.array_equal(fused.view(np.uint32), two.view(np.uint32))
    c_ref, s = O.gemm_w4a8(aq, bq, t, want_sumi=True)
    mfma = qg.select_algo(m, n, k, t) == 2
    assert mfma == (m == 12)
    report(f"f32_fused t={t} ({m},{n},{k}) shift={shift}", two, c_ref, bound(O, 8 if mfma else "sum", aq, bq, s, t))


@pytest.mark.parametrize("ntok,shift", [(1, 0), (1, 1), (1, 2), (4, 0), (12, 1)])
def test_f16_fused_activations(O, qg, ntok, shift):
    """The Q4_0 fp16_fused entry (weight-major) on the same rows as f16, with the fused kernel's quantizer."""
    import torch
    t, mw, k = 2, 19, 1024
    x = scaled_rows(ntok, k, shift, 16).astype(np.float16)
    assert np.isfinite(x).all()
    _, wq, _, _ = operands(t, 6, mw, k)
    x_d, w_d = dev(x), dev(wq)
    aq_d = qg.quantize_q8_1_f16_fused(x_d)
    aq = host(aq_d)
    assert np.array_equal(aq, O.quantize_q8_1_fused_f16(x))
    check_emitted_scales(aq, ntok, shift)
    lib = qg._lib.load()
    two = guarded_run(mw, ntok, lambda view, ldc: qg._lib.check(lib.qg_gemm_q4_0_q8_1(
        P(w_d.data_ptr()), P(aq_d.data_ptr()), P(view.data_ptr()), mw, ntok, k, stream()), "gemm_q4_0_q8_1"), dense=True)
    wsb = lib.qg_gemm_w4a8_f32_workspace_size(ntok, k)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    fused = guarded_run(mw, ntok, lambda view, ldc: qg._lib.check(lib.qg_gemm_q4_0_fp16_fused_ws(
        P(w_d.data_ptr()), P(x_d.data_ptr()), P(view.data_ptr()), mw, ntok, k, P(ws.data_ptr()), wsb, stream()),
        "fp16_fused"), dense=True)
    assert np.array_equal(fused.view(np.uint32), two.view(np.uint32))
    c_ref, s = O.gemm_w4a8(aq, wq, t, want_sumi=True)
    mfma = qg.select_algo(ntok, mw, k, t) == 2
    report(f"f16_fused t={t} ({mw},{ntok},{k}) shift={shift}", np.ascontiguousarray(two.T), c_ref,
           bound(O, 8 if mfma else "sum", aq, wq, s, t))


# ------------------------------------------------------------------------------------------------ W4A16 / W8A16
@pytest.mark.parametrize("t", [2, 8])
@pytest.mark.parametrize("m", [1, 4, 16, 40])
@pytest.mark.parametrize("k", [256, 1024])
def test_w16(O, qg, t, m, k):
    """The extreme weight rows on N(0, 1) activations, within the W16 tests' bound (oracle.w16_tol)."""
    n = 19
    _, bq, _, _ = operands(t, 6, n, k)
    a = np.random.default_rng([16, t, m, k]).standard_normal((m, k)).astype(np.float32)
    lib, a_d, w_d = qg._lib.load(), dev(a), dev(bq)
    sym = "qg_gemm_w4a16" if t == 2 else "qg_gemm_w8a16"
    c = guarded_run(m, n, lambda view, ldc: qg._lib.check(getattr(lib, sym)(
        P(a_d.data_ptr()), P(w_d.data_ptr()), P(view.data_ptr()), m, n, k, stream()), sym), dense=True)
    ref = O.gemm_w4a16(a, bq) if t == 2 else O.gemm_w8a16(a, bq)
    report(f"w16 t={t} ({m},{n},{k})", c, ref.astype(np.float64), O.w16_tol(a, bq, t))
