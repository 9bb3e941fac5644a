"""The quantizing prologue of the row GEMV (gemv_body, csrc/qg_gemv_kernel.hpp, AIN_F32 and AIN_F16_FUSED) in every
kernel form the Q8_1 variant is tested in (GEMV_CASES of tests/test_gpu_q32_extremes.py), and the host path that launches
it (run_fused, csrc/qg_api.hip): the single launch at M <= 4, the chunks of 8 / 4 / 2 rows without a workspace with
their strided batch and remainder launch, and the fall-backs where the LDS records of a chunk exceed 96 KiB.

Bars, the project's own: the device quantizer's bytes are the oracle's; every fused launch is
bit-identical (uint32 views) to the two-step GEMV (algo = 1) on the same rows, every output element compared; the result
lies within oracle.summation_tol of oracle.gemm_w4a8 on those bytes, and that reference is finite. Every fused launch
goes into the interior of a sentinel-filled buffer, twice (guarded_run).

Activation rows cycle through five sources (activation_rows): the step-4 uniform recipe, the three scales of
scaled_rows (subnormal f16 d, d = +0, large d) and the edge_rows set (all-zero block, exact rounding ties, the f16-tie
sum), so a prologue whose quantizer parted from the stand-alone one shows in the bits. No NaN, no Inf, no block whose
1 / d overflows (tests/test_fused_forms_cpu.py checks the inputs, and holds these lists to the kernel forms).

The fused FP32 entry takes dense output rows only (qg_gemm_w4a8_f32 has no row stride), so "strided out" here is the
FP16 entry's weight-major output (token stride 1, row stride N_tok) and, for FP32, the guard floats on either side.
Each case prints its max err / tol (profiles/fused_forms/README.md).
"""
import functools

import numpy as np
import pytest

from test_gpu_parity import dev, edge_rows, host
from test_gpu_q32_extremes import GEMV_CASES, P, TYPES, bound, field, gemv_form, guarded_run, operands, report, \
    scaled_rows, stream

pytestmark = pytest.mark.gpu

Q4_0, Q4_1, Q5_0, Q5_1, Q8_0 = TYPES
SOURCES = ("step4", "sub_d", "zero_d", "large_d", "edge")  # sub_d .. large_d: scaled_rows' SCALES 1e-4, 1e-6, 3e4
REC_DW = {2: 28, 4: 52}  # gemv_geom::REC_DW = 12 BPL + 4
LDS_LIMIT = 96 * 1024


def n_of(t, k):
    """test_row_gemv's rule: 19 <= N <= 33, no multiple of the rows per workgroup"""
    return 19 + (t + k // 32) % 15


# ------------------------------------------------------------------------------------------------ the lists
# 1. one launch (M <= 4): the M <= 4 cases of GEMV_CASES; (1, 4160): 65 units on 64 lanes; the published decode K at
#    M = 1 and 2; M = 3 and 2 in two unit-loop forms of K < 4096; (3, 32768): the records of 3 rows exceed 96 KiB, so two
#    rows and one (no workspace) or the two-step product (workspace). The last two lines: so that the M tiles of 2 and
#    of 4 meet every K < 4096 form loop-free and with its unit loop, as M = 1 does through GEMV_CASES
F32_SINGLE = [c for c in GEMV_CASES if c[0] <= 4] + [(1, 4160), (1, 14336), (2, 14336), (3, 576), (2, 3072), (3, 32768)] + \
             [(2, k) for k in (192, 512, 576, 640, 1536, 2048)] + \
             [(4, 192), (3, 512), (4, 640), (3, 1536), (4, 2048), (3, 3072)]
# 3. (t, M, N, K): the Q8_1 twin takes the N >= 16384 form, the fused launch keeps its own workgroup size
F32_MANY_ROWS = [(Q4_0, 1, 16384, 4096), (Q5_0, 1, 16384, 4096)]
# 4. (t, M, N, K, rows per chunk), workspace=False
F32_CHUNKED = [(t, m, n_of(t, k), k, 8) for t in TYPES for m in (5, 6, 8) for k in (192, 1024, 6144)] + \
              [(t, 13, n_of(t, 8192), 8192, 4) for t in (Q4_0, Q8_0)] + \
              [(Q4_1, 4, n_of(Q4_1, 16384), 16384, 2), (Q4_1, 7, n_of(Q4_1, 16384), 16384, 2)] + \
              [(Q4_0, 16, 4112, 4096, 8), (Q5_1, 16, 4112, 4096, 8)] + \
              [(Q4_0, 16, n_of(Q4_0, 1024), 1024, 8)]
# 5. FP16 (Q4_0): (N_tok, K), both workspace settings; (N_tok, K) without a workspace
F16_SINGLE = [(ntok, k) for ntok in (1, 2, 3, 4) for k in (576, 640, 1536, 3072, 4096, 4160, 8192, 14336, 32768)]
F16_CHUNKED = [(ntok, k) for ntok in (6, 13) for k in (1024, 6144, 8192)]


# ------------------------------------------------------------------------------------------------ run_fused, restated
def gemv_shape_ok(m, k):
    """gemv_shape_ok behind ok_f (csrc/qg_gemv_kernel.hpp, qg_gemv_impl.hpp) for aligned operands: the unit size from
    K/32 % 4, whole units, and the LDS test M > 2 and M * units * REC_DW * 4 > 96 KiB."""
    nb = k // 32
    bpl = 4 if nb % 4 == 0 else 2
    if not 1 <= m <= 8 or k % (32 * bpl) != 0:
        return False
    return not (m > 2 and m * (nb // bpl) * REC_DW[bpl] * 4 > LDS_LIMIT)


def chunk_rows(m, k):
    """run_fused's chunk without a workspace: the first of 8, 4, 2, 1 that gemv_shape_ok takes (with at most M rows)"""
    for rows in (8, 4, 2, 1):
        if gemv_shape_ok(min(rows, m), k):
            return rows
    return 0


def fused_launches(m, k, workspace):
    """The row ranges [(r0, r1)] of the fused GEMV launches of run_fused (csrc/qg_api.hip) — one launch at an eligible
    M <= 4, otherwise without a workspace a strided batch of whole chunks and a remainder launch — or None: quantized
    into the workspace, then the Q8_1 product of the auto dispatch."""
    if m <= 4 and gemv_shape_ok(m, k):
        return [(0, m)]
    if workspace:
        return None
    c = min(chunk_rows(m, k), m)
    assert c, (m, k)
    return [(r, min(r + c, m)) for r in range(0, m, c)]


def fused_form(t, m, k):
    """gemv_form of a fused launch: the Q8_1 rule without its N >= 16384 exception (qg_gemv_impl.hpp:58)"""
    return gemv_form(t, m, 0, k)


# ------------------------------------------------------------------------------------------------ activations
@functools.lru_cache(maxsize=None)
def activation_rows(m, k, start):
    """float32 [m, k], read-only: row i from SOURCES[(start + i) % 5], tiled to K. The edge source is the seven edge_rows
    (64 values each) one after another, begun at row (start + i) % 7, so one row holds every edge block."""
    import oracle as O
    rows = []
    for i in range(m):
        src = SOURCES[(start + i) % len(SOURCES)]
        if src == "step4":
            rows.append(O.fill_uniform_step4(1, 1, k, 50 + start + i)[0][0])
        elif src == "edge":
            e = np.roll(edge_rows(), -((start + i) % 7), axis=0).ravel()
            rows.append(np.tile(e, -(-k // e.size))[:k])
        else:
            rows.append(scaled_rows(1, k, SOURCES.index(src) - 1, start + i)[0])
    x = np.stack(rows).astype(np.float32)
    x.setflags(write=False)
    return x


def start_of(t, index):
    """the first row's source: by case index and format, so a case meets every source across the five formats"""
    return index + TYPES.index(t)


def bits(c):
    return np.ascontiguousarray(c).view(np.uint32)


def assert_same_bits(got, twin, what):
    diff = np.argwhere(bits(got) != bits(twin))
    assert diff.size == 0, f"{what}: {len(diff)} outputs differ from two-step, {diff[:8].tolist()}"


# ------------------------------------------------------------------------------------------------ FP32
def f32_case(O, qg, t, m, n, k, start, workspaces, both_ends=False):
    x = activation_rows(m, k, start)
    bq = operands(t, 1, n, k, (1,), both_ends)[1]
    x_d, w_d = dev(x), dev(bq)
    aq_d = qg.quantize_q8_1(x_d)
    aq = host(aq_d)
    assert np.array_equal(aq, O.quantize(x, O.Q8_1)), "device quantizer bytes"
    c_ref, s = O.gemm_w4a8(aq, bq, t, want_sumi=True)
    assert np.isfinite(c_ref).all()
    for ws in workspaces:
        label = f"f32 t={t} ({m},{n},{k}) ws={int(ws)} src={SOURCES[start % 5]}"
        got = guarded_run(m, n, lambda view, ldc: qg.gemm_w4a8_f32(x_d, w_d, t, workspace=ws, out=view), dense=True)
        launches = fused_launches(m, k, ws)
        if launches is None:  # the two-step product of the auto dispatch on the workspace
            two = host(qg.gemm_w4a8(aq_d, w_d, m, n, k, t))
            assert_same_bits(got, two, label)
            kind = 8 if qg.select_algo(m, n, k, t) == 2 else "sum"
        else:
            for r0, r1 in launches:
                twin = host(qg.gemm_w4a8(aq_d[r0:r1].contiguous(), w_d, r1 - r0, n, k, t, algo=1))
                assert_same_bits(got[r0:r1], twin, f"{label} rows {r0}:{r1}")
            kind = "sum"
        report(label, got, c_ref, bound(O, kind, aq, bq, s, t))
    return launches


@pytest.mark.parametrize("t", TYPES)
@pytest.mark.parametrize("m,k", F32_SINGLE)
def test_f32_single_launch(O, qg, t, m, k):
    """With and without a workspace the one fused launch wherever M rows are eligible (every case but (3, 32768))."""
    launches = f32_case(O, qg, t, m, n_of(t, k), k, start_of(t, F32_SINGLE.index((m, k))), (False, True))
    assert (launches == [(0, m)]) == ((m, k) != (3, 32768))


@pytest.mark.parametrize("t,m,n,k", F32_MANY_ROWS)
def test_f32_many_rows(O, qg, t, m, n, k):
    """N >= 16384: gemv_form sends the Q8_1 launch to 512-thread workgroups, the fused one keeps W1 (1024 threads for
    Q4_0, 512 for Q5_0); a wave sums one row in the same order either way, so the same bits. The class rows at both ends
    of N."""
    cfg = qg.debug_config(m, n, k, t, algo=1)
    assert cfg.startswith(f"gemv F={t} MT=1 BPL=2 LPR=64 WGS=512 AIN=0 "), cfg
    assert gemv_form(t, m, n, k)[1:4] == (2, 64, 512)
    assert fused_form(t, m, k)[1:4] == (2, 64, 1024 if t == Q4_0 else 512)
    assert f32_case(O, qg, t, m, n, k, start_of(t, 3), (False,), both_ends=True) == [(0, 1)]


@pytest.mark.parametrize("t,m,n,k,rows", F32_CHUNKED)
def test_f32_chunks(O, qg, t, m, n, k, rows):
    """workspace=False: chunk by chunk the two-step GEMV on the same rows (a strided batch of whole chunks, then the
    remainder launch)."""
    assert chunk_rows(m, k) == rows
    launches = f32_case(O, qg, t, m, n, k, start_of(t, F32_CHUNKED.index((t, m, n, k, rows))), (False,))
    assert launches == [(r, min(r + rows, m)) for r in range(0, m, rows)]
    mt, bpl, lpr, wgs, loop_free = gemv_form(t, min(rows, m), n, k)  # the Q8_1 twin of a whole chunk
    cfg = qg.debug_config(min(rows, m), n, k, t, algo=1)
    assert cfg.startswith(f"gemv F={t} MT={mt} BPL={bpl} LPR={lpr} WGS={wgs} AIN=0 "), cfg
    assert (field(cfg, "ONEU") != "0") == loop_free, cfg


# ------------------------------------------------------------------------------------------------ FP16 (Q4_0)
def f16_case(O, qg, ntok, k, start, workspaces):
    import torch
    t = Q4_0
    mw = n_of(t, k)
    x = activation_rows(ntok, k, start).astype(np.float16)
    assert np.isfinite(x).all()
    wq = operands(t, 1, mw, k, (1,))[1]
    x_d, w_d = dev(x), dev(wq)
    aq_d = qg.quantize_q8_1_f16_fused(x_d)
    aq = host(aq_d)
    assert np.array_equal(aq, O.quantize_q8_1_fused_f16(x)), "device quantizer bytes"
    c_ref, s = O.gemm_w4a8(aq, wq, t, want_sumi=True)  # [ntok, mw]: the transposed view
    assert np.isfinite(c_ref).all()
    lib = qg._lib.load()
    for ws in workspaces:
        label = f"f16 ({mw},{ntok},{k}) ws={int(ws)} src={SOURCES[start % 5]}"
        wsb = lib.qg_gemm_w4a8_f32_workspace_size(ntok, k) if ws else 0
        buf = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
        out = guarded_run(mw, ntok, lambda view, ldc: qg._lib.check(lib.qg_gemm_q4_0_fp16_fused_ws(
            P(w_d.data_ptr()), P(x_d.data_ptr()), P(view.data_ptr()), mw, ntok, k, P(buf.data_ptr()) if ws else None, wsb,
            stream()), "fp16_fused"), dense=True)
        launches = fused_launches(ntok, k, ws)
        kind = "sum"
        if launches is None or (ntok <= 4 and launches == [(0, ntok)]):  # the reference's two-step entry, auto dispatch
            two = host(qg.gemm_q4_0_q8_1(w_d, aq_d, mw, ntok, k))
            assert_same_bits(out, two, label)
            if launches is None and qg.select_algo(ntok, mw, k, t) == 2:
                kind = 8
        if launches is not None:
            for r0, r1 in launches:
                twin = host(qg.gemm_w4a8(aq_d[r0:r1].contiguous(), w_d, r1 - r0, mw, k, t, algo=1))
                assert_same_bits(out[:, r0:r1].T, twin, f"{label} tokens {r0}:{r1}")
        report(label, np.ascontiguousarray(out.T), c_ref, bound(O, kind, aq, wq, s, t))


@pytest.mark.parametrize("ntok,k", F16_SINGLE)
def test_f16_single_launch(O, qg, ntok, k):
    f16_case(O, qg, ntok, k, F16_SINGLE.index((ntok, k)), (False, True))


@pytest.mark.parametrize("ntok,k", F16_CHUNKED)
def test_f16_chunks(O, qg, ntok, k):
    assert chunk_rows(ntok, k) == (4 if (ntok, k) == (13, 8192) else 8)
    f16_case(O, qg, ntok, k, 2 + F16_CHUNKED.index((ntok, k)), (False,))
