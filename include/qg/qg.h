/*
 * qg/qg.h — C-ABI of the MI355X (gfx950) W4A8 quantized GEMM/GEMV library `libqg_hip.so`.
 *
 * Plain C: raw device pointers, sizes, an opaque HIP stream. Every call is stream-ordered and
 * asynchronous (no host sync — the one exception is the one-time growth of a workspace the library
 * keeps for a stream, see qg_gemm_w4a8_ws / qg_gemm_w4a16_ws, which the _ws forms avoid), reentrant;
 * the caller owns all buffers
 * (destination-passing, schemas/docs/solution.md:27-42). Unlike the reference's `void` launch
 * wrappers (include/gemm_cuda_naive.cuh:285-292 — no error check), every entry point returns a
 * qg_status: 0 on success, a negative code otherwise; nothing is launched on a validation error.
 *
 * Conventions (the two-convention trap):
 *   activation-major  C[M][N] = A_q8_1[M][K] . B_w[N][K]^T   M = tokens, N = weight rows
 *                     (include/gemm_reference.h:7-13, 175-222; include/llama_adapter.h)
 *   weight-major      out[M][N] = W[M][K] . A_q8_1[N][K]^T   M = weight rows, N = tokens
 *                     (kernels/gemm/gemm_quant_formats.cuh:312-334, python/quant_gemm)
 * Block layouts: qg/blocks.h (byte-identical to include/quant_types.h / compat/ggml_types.h).
 */
#ifndef QG_QG_H
#define QG_QG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Binary-compatible with hipStream_t (NULL = the default stream). */
typedef struct ihipStream_t* qg_stream_t;

/* Quantization type ids = ggml_type ids (compat/ggml_types.h:199-215). */
typedef enum {
    QG_TYPE_F32 = 0,
    QG_TYPE_F16 = 1,
    QG_TYPE_Q4_0 = 2,
    QG_TYPE_Q4_1 = 3,
    QG_TYPE_Q5_0 = 6,
    QG_TYPE_Q5_1 = 7,
    QG_TYPE_Q8_0 = 8,
    QG_TYPE_Q8_1 = 9,
    QG_TYPE_Q4_K = 12, /* 256-element super-blocks of 144 B (qg/blocks.h); see "Q4_K weights" below */
    QG_TYPE_Q6_K = 14, /* 256-element super-blocks of 210 B (qg/blocks.h); see "Q6_K weights" below */
    QG_TYPE_I32 = 26,  /* int32 elements: the ids view of qg_mul_mat_id_from_view, nothing else */
    QG_TYPE_MXFP4 = 39 /* 32-element blocks of 17 B, E8M0 scale and E2M1 codes (qg/blocks.h); see "MXFP4 weights" below */
} qg_type;

typedef enum {
    QG_OK = 0,
    QG_ERR_INVALID_ARG = -1, /* null pointer, negative size, unknown kernel_type */
    QG_ERR_BAD_K = -2,       /* K (or element count) not a positive multiple of 32 */
    QG_ERR_UNSUPPORTED = -3, /* weight type / algorithm not available for this shape */
    QG_ERR_ALIGN = -4,       /* pointer alignment below what the block format allows */
    QG_ERR_HIP = -5          /* HIP launch error (see qg_last_hip_error) */
} qg_status;

/* Kernel family selection for qg_gemm_w4a8_ex (QG_ALGO_AUTO picks by shape). */
typedef enum {
    QG_ALGO_AUTO = 0,
    QG_ALGO_GEMV = 1,    /* M <= 8 (auto: M <= 4): register-resident weight units; Q4_0/Q4_1 nibble-plane
                            v_dot8_u32_u4 / v_dot8_i32_i4, Q5_x/Q8_0 byte decode + v_dot4 */
    QG_ALGO_MFMA = 2,    /* any M (auto: M >= 5), K % 128 == 0: v_mfma_i32_16x16x32_i8 per Q-block */
    QG_ALGO_GENERIC = 3, /* any K % 32 == 0, any alignment: byte loads, one wave per output (cross-check) */
    QG_ALGO_RAGGED = 4   /* any K % 32 == 0 (odd K / 32), 2-B aligned weights: one wave per weight row */
} qg_algo;

/* ---- W4A8 GEMM, activation-major ---------------------------------------------------------
 * Replaces gemm_w4a8_{naive,tiled,dp4a,tiled_dp4a,vectorized_dp4a}(A, B, C, M, N, K, stream)
 * (include/gemm_cuda_naive.cuh:285-292, gemm_cuda_tiled.cuh:293-300, gemm_cuda_dp4a.cuh:409-444)
 * and is the device twin of gemm_w4a8_reference (include/gemm_reference.h:175-222).
 * A: block_q8_1[M][K/32]; B: blocks of `wtype` (Q4_0/Q4_1/Q5_0/Q5_1, or Q8_0 = W8A8) [N][K/32];
 * C: float[M][N], overwritten. M == 0 or N == 0 is a no-op.
 *
 * Under stream capture (hipStreamBeginCapture, torch.cuda.graph) consecutive independent GEMVs become ONE
 * kernel node: a call with M <= 4 that AUTO (or QG_ALGO_GEMV) sends to the GEMV, whose only capture
 * dependency is the GEMV node the calling thread's previous qg_gemm_w4a8 / _ex / _ldc call created in the
 * same capture, with the same M, K and weight type, adds no node; that node is rewritten into the grouped
 * launch of qg_gemm_w4a8_grouped over all of them (up to 64 per node). "Independent": the call's output
 * overlaps no operand of the node's products and its inputs overlap none of their outputs (shared
 * activations or weights are fine); anything else, e.g. a GEMV that reads the previous one's output, stays
 * its own node, ordered as captured. Outputs are unchanged bit for bit, and a graph replays the same
 * dependencies towards everything else captured. Merged where it measured faster (csrc/qg_capture_fuse.hip,
 * fuse_class_enabled): every M <= 4 in the loop-free form (K <= 4096), M = 1 beyond; see
 * qg_set_capture_fusion. Eager (non-captured) calls are never merged. */
int qg_gemm_w4a8(const void* A_q8_1, const void* B, float* C, int M, int N, int K, int wtype, qg_stream_t stream);
int qg_gemm_w4a8_ex(const void* A_q8_1, const void* B, float* C, int M, int N, int K, int wtype, int algo,
                    qg_stream_t stream);
/* As qg_gemm_w4a8_ex with an output row stride: C[m * ldc + n], ldc >= N floats (e.g. a rank's
 * column slice of a wider buffer in the row-sharded multi-GPU path, quant_gemm/sharded.py). */
int qg_gemm_w4a8_ldc(const void* A_q8_1, const void* B, float* C, int M, int N, int K, int64_t ldc, int wtype,
                     int algo, qg_stream_t stream);

/* ---- Q4_K weights (wtype == QG_TYPE_Q4_K) --------------------------------------------------
 * B: block_q4_K[N][K/256], ggml's bytes (qg/blocks.h). Sub-block j of super-block sb meets activation
 * block 8 sb + j:
 *   C(m, n) = sum_sb [ d * sum_j d_a * float(sc_j * sumi_j)  -  dmin * sum_j float(m_j) * s_a ]
 * with sumi the exact int32 dot of the 4-bit codes and the Q8_1 bytes, and s_a the Q8_1 block's stored sum
 * (as the Q4_1 / Q5_1 min terms). The order of the fp32 operations is the kernel's; each output is within
 * 2 * (K/32 + W + 2) * 2^-24 * sum(|terms|) of the exact value, W = 0 for the decode GEMV and 16 for the
 * MFMA prefill, and two launches give identical bits.
 * Taken by: qg_gemm_w4a8, qg_gemm_w4a8_ex, qg_gemm_w4a8_ldc, qg_debug_sumi (per-sub-block sumi[M][N][K/32]
 * from the product's own instantiation), qg_debug_config, qg_select_algo, qg_dequantize,
 * qg_gemm_w4a8_from_view (weights view: nb[0] = 144, ne[0] = K) and qg_gemm_w4a8_f32 with a workspace
 * (quantize into it, then the product). QG_ALGO_AUTO: the decode GEMV ("q4k_gemv") for M <= 8, the MFMA
 * prefill ("q4k_mmq") from M = 9 on; both may be forced (the GEMV only for M <= 8 and while its LDS
 * records, 336 B per token and super-block, fit 160 KiB).
 * Validation: K not a positive multiple of 256 -> QG_ERR_BAD_K; B not 16-B aligned or A not 4-B aligned ->
 * QG_ERR_ALIGN; QG_ALGO_RAGGED / QG_ALGO_GENERIC -> QG_ERR_UNSUPPORTED; qg_gemm_w4a8_f32 without a
 * workspace of qg_gemm_w4a8_f32_workspace_size(M, K) bytes -> QG_ERR_UNSUPPORTED.
 * Every other entry that takes a wtype (tiled, repacked, prepacked, padded, grouped, strided-batched, _ws,
 * qg_quantize) returns QG_ERR_UNSUPPORTED for it and launches nothing. */

/* ---- Q6_K weights (wtype == QG_TYPE_Q6_K) --------------------------------------------------
 * B: block_q6_K[N][K/256], ggml's bytes (qg/blocks.h), rows dense. Q8_1 block b (0..7) of super-block sb is
 * activation block 8 sb + b; it covers elements 32b .. 32b + 31, exactly the scale groups 2b (first 16
 * elements) and 2b + 1 (last 16). With s0, s1 the exact int32 dots of the signed codes q (-32..31) with the
 * Q8_1 bytes over those two halves:
 *   isum(m, n, 8 sb + b) = scales[2b] * s0 + scales[2b + 1] * s1          (int32, exact; |isum| <= 2^24)
 *   C(m, n) = sum_sb d * sum_b d_a(8 sb + b) * float(isum)
 * The Q8_1 block's stored sum s_a is not used (the -32 is in the signed codes). The order of the fp32
 * operations is the kernel's; each output is within 2 * (K/32 + W + 2) * 2^-24 * sum(|d d_a isum|) of the
 * exact value, W = 0 for the decode GEMV and 8 for the MFMA prefill, and two launches give identical bits.
 * Taken by the same entries as Q4_K: qg_gemm_w4a8, qg_gemm_w4a8_ex, qg_gemm_w4a8_ldc, qg_debug_sumi
 * (isum[M][N][K/32] from the product's own instantiation), qg_debug_config, qg_select_algo, qg_dequantize
 * ((d * float(scale)) * float(q), each product rounded to fp32), qg_gemm_w4a8_from_view (weights view:
 * nb[0] = 210, ne[0] = K, dense rows) and qg_gemm_w4a8_f32 with a workspace. QG_ALGO_AUTO: the decode GEMV
 * ("q6k_gemv") for M <= 8, the MFMA prefill ("q6k_mmq") from M = 9 on; both may be forced (the GEMV only for
 * M <= 8 and while its LDS records, 304 B per token and super-block, fit 160 KiB). A Q6_K GEMV captured into
 * a graph is a plain kernel node: the capture-time merge never considers it.
 * Validation: K not a positive multiple of 256 -> QG_ERR_BAD_K; A not 4-B aligned or B not 2-B aligned ->
 * QG_ERR_ALIGN (a 210-B super-block guarantees no more than 2 B inside a row, so the kernels take both
 * parities); QG_ALGO_RAGGED / QG_ALGO_GENERIC -> QG_ERR_UNSUPPORTED; qg_gemm_w4a8_f32 without a workspace ->
 * QG_ERR_UNSUPPORTED. Every other entry that takes a wtype returns QG_ERR_UNSUPPORTED for it, as for Q4_K,
 * and qg_tile_weights_bytes / qg_repack_weights_bytes return 0. */

/* ---- MXFP4 weights (wtype == QG_TYPE_MXFP4) -------------------------------------------------
 * B: block_mxfp4[N][K/32], ggml's bytes (qg/blocks.h), rows dense: 17 bytes per 32 elements, one E8M0 scale byte e
 * and 16 bytes of 4-bit codes in the Q4_0 nibble order. A code indexes
 *   kv[16] = {0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12}     (the doubled E2M1 values; code 8 is 0)
 * and scale(e) is the fp32 with bits e < 2 ? 0x00200000 << e : (e - 1) << 23, i.e. 2^(e - 128) for all 256 values of
 * e (e = 0, 1: the subnormals 2^-128, 2^-127; e = 255: 2^127; there is no NaN code). qg_dequantize gives
 * float(kv[code]) * scale(e): exact for every (code, e), +0.0f for code 8.
 * The product of block b of a weight row with Q8_1 block b of the activation row:
 *   sumi(m, n, b) = sum_j kv[code_j] * a_j                       (int32, exact; |sumi| <= 32 * 12 * 128 < 2^24)
 *   C(m, n) = sum_b (d_a * scale(e)) * float(sumi)               (the multiplications in that order, each rounded)
 * The Q8_1 block's stored sum s_a is not used. The order of the additions is the kernel's; each output is within
 * 2 * (K/32 + W + 2) * 2^-24 * sum_b |term| of the exact value, W = 0 for the decode GEMV and the host twin and
 * W = 8 for the MFMA prefill (the K-slice partials it chains per output; MXFP4_MMQ_W in csrc/qg_mxfp4.hpp), and two
 * launches give identical bits. fp32 subnormals are kept: where a term or d_a * scale(e) lies below 2^-126 the
 * bound gains 2^-149 per term. Overflow (large e with large d_a * sumi) gives what fp32 gives.
 * Taken by: qg_gemm_w4a8, qg_gemm_w4a8_ex, qg_gemm_w4a8_ldc, qg_debug_sumi (sumi[M][N][K/32] from the product's own
 * instantiation), qg_debug_config, qg_select_algo, qg_dequantize, qg_gemm_w4a8_from_view (weights view:
 * nb[0] = 17, ne[0] = K, dense rows), qg_gemm_w4a8_f32 with a workspace, and qg_gemm_w4a8_moe /
 * qg_mul_mat_id_from_view (family "moe:mxfp4_gemv"; the expert stride N * K/32 * 17 is any number of bytes).
 * QG_ALGO_AUTO: the decode GEMV ("mxfp4_gemv") for M <= 8, the MFMA prefill ("mxfp4_mmq") from M = 9 on; both may
 * be forced (the GEMV only for M <= 8 and while its LDS records, 48 B per token and block, fit 160 KiB:
 * M * K <= 109216 elements). A captured MXFP4 GEMV is a plain kernel node: the capture-time merge never considers it.
 * Validation: K not a positive multiple of 32 -> QG_ERR_BAD_K; A not 4-B aligned -> QG_ERR_ALIGN; B has NO alignment
 * requirement (17-B blocks start at any byte: the kernels read aligned dwords and realign them, and read nothing
 * outside the tensor); QG_ALGO_RAGGED / QG_ALGO_GENERIC -> QG_ERR_UNSUPPORTED; qg_gemm_w4a8_f32 without a workspace
 * -> QG_ERR_UNSUPPORTED. Every other entry that takes a wtype (tiled, repacked, prepacked, padded, grouped,
 * strided-batched, _ws, qg_quantize, the weight-major qg_gemm_q*, qg_gemm_w4a8_moe_prefill, _batch, _glu, _down)
 * returns QG_ERR_UNSUPPORTED for it and launches nothing. There is no MXFP4 quantizer. */

/* The Solution entry point of the definition gemm_q4_0_q8_1_w4a8
 * (schemas/definitions/gemm/gemm_q4_0_q8_1_w4a8.json:35-53: inputs A_q8_1[M][K/32], B_q4_0[N][K/32],
 * output C[M][N]; destination-passing, schemas/docs/solution.md:27-42), in definition order —
 * the role include/gemm_cuda_dp4a.cuh::gemm_q4_0_q8_1_dp4a plays for the reference's CUDA
 * solutions (schemas/solutions/gemm_q4_0_q8_1_cuda_dp4a.json:15). == qg_gemm_w4a8(..., QG_TYPE_Q4_0).
 * Registered by integration/solutions/gemm_q4_0_q8_1_hip_gfx950.json. */
int qg_gemm_q4_0_q8_1_w4a8(const void* A_q8_1, const void* B_q4_0, float* C, int M, int N, int K,
                           qg_stream_t stream);

/* As qg_gemm_w4a8 (QG_ALGO_AUTO) with a caller workspace for the odd-K/32 prefill route (K/32 not a
 * multiple of 8, or 2-B aligned weights, at M >= 32 and N >= 1024): weights and activations are
 * copied into zero-padded rows inside `workspace` (>= qg_gemm_w4a8_workspace_size(M, N, K, wtype)
 * bytes, 256-B aligned; 0 for shapes that never take that route) and the MFMA kernel runs on the
 * copy. Capture-safe (a graph keeps the caller's pointer). Without a workspace, qg_gemm_w4a8 uses
 * a buffer the library keeps per (device, stream) — it grows to the largest N*K'/32*bb +
 * M*K'/32*36 bytes seen on that stream (K' = K rounded up to 256), is held until
 * qg_release_workspaces(), and growing it synchronizes that stream once; during stream capture
 * that buffer is never used and such shapes run the ragged kernel instead (same results to the
 * summation-order bound, not bit for bit). Weights used many times: repack once with
 * qg_repack_weights and call qg_gemm_w4a8_prepacked. */
size_t qg_gemm_w4a8_workspace_size(int M, int N, int K, int wtype);
int qg_gemm_w4a8_ws(const void* A_q8_1, const void* B, float* C, int M, int N, int K, int wtype, void* workspace,
                    size_t workspace_bytes, qg_stream_t stream);

/* (Round 5: for weights reused across calls the tiled layout below — qg_tile_weights +
 * qg_gemm_w4a8_tiled, or qg_gemm_w4a8_tiled_act with tiled activations — is the faster route for odd K/32
 * as well: M = 32, K = 4128 6.1-6.2 us against 7.4 us here and 7.2 us for qg_gemm_w4a8_padded; DESIGN.md §6.
 * The padded rows below stay for callers that keep the reference row layout.)
 * Load-time weight layout for K/32 not a multiple of 8 (e.g. K = 4128): rows of K'/32 blocks,
 * K'/32 = round_up(K/32, 8), the real blocks first and then zero blocks (d = 0: every padded term is
 * an exact +0 of the reference's sum). qg_repack_weights writes B_packed (16-B aligned,
 * qg_repack_weights_bytes(N, K, wtype) bytes) from B [N][K/32]; one streaming kernel.
 * qg_gemm_w4a8_prepacked then computes the SAME product as qg_gemm_w4a8(A, B, ...) (within the
 * summation-order bound; K is the logical K) from B_packed: the activations are padded into
 * `workspace` (>= qg_gemm_w4a8_prepacked_workspace_size(M, K) bytes, 16-B aligned; 0 when K/32 is
 * already a multiple of 8) and the QG_ALGO_AUTO kernel runs on K' — no per-call weight copy. From M = 5
 * (the MFMA kernel) the activations are read in place instead (round 5: one launch, the workspace
 * is not touched). Capture-safe. */
size_t qg_repack_weights_bytes(int N, int K, int wtype);
int qg_repack_weights(const void* B, void* B_packed, int N, int K, int wtype, qg_stream_t stream);
size_t qg_gemm_w4a8_prepacked_workspace_size(int M, int K);
/* The activation side of the same layout, written by the quantizer itself so the product is ONE
 * launch: qg_quantize_q8_1_padded quantizes M rows of K floats (as qg_quantize_q8_1) into rows of
 * K'/32 Q8_1 blocks, zero blocks after the real ones; qg_gemm_w4a8_padded(A_padded, B_packed, ...)
 * then runs the QG_ALGO_AUTO kernel on K' directly (K is the logical K). */
int qg_quantize_q8_1_padded(const float* x, void* y, int M, int K, qg_stream_t stream);
int qg_gemm_w4a8_padded(const void* A_padded, const void* B_packed, float* C, int M, int N, int K, int wtype,
                        qg_stream_t stream);
int qg_gemm_w4a8_prepacked(const void* A_q8_1, const void* B_packed, float* C, int M, int N, int K, int wtype,
                           void* workspace, size_t workspace_bytes, qg_stream_t stream);

/* Load-time TILED weight layout (round 5) — the fast form for weights used many times, any K % 32 == 0.
 * qg_tile_weights writes B_tiled (16-B aligned, qg_tile_weights_bytes(N, K, wtype) bytes) from B
 * [N][K/32]: rows in tiles of 32, K/32 in stages of 4 blocks, each (tile, stage) one contiguous run of
 * 128 * block_bytes bytes whose fields are arranged in the prefill kernel's operand order (qs by MFMA
 * k-slot, then qh, then the f16 scales); rows past N and blocks past K/32 are zero (d = 0: an exact +0
 * term). The layout is specified in llama.cpp-quant-gemm_amd/csrc/qg_mmq_kernel.hpp (tiled_fmt) and
 * restated in oracle/oracle.py (tile_weights); one streaming kernel.
 * qg_gemm_w4a8_tiled then computes the same product as qg_gemm_w4a8(A, B, ...) (activation-major,
 * A: block_q8_1 [M][K/32], 16-B aligned; within the reassociation bound of the MFMA kernel, DESIGN.md
 * §5; for M = 1..2 the tiled decode GEMV, whose per-block terms are the reference's bit for bit, summed in
 * a fixed order; for M = 3..4, and M = 2 at K/32 > 256, the MFMA small-batch decode, within the same
 * reassociation bound) from B_tiled in ONE launch for every M — the prefill's weight stages are one linear
 * stream instead of 32 row segments. K/32 need not be a multiple of 4 or 8 (the kernel windows the plain
 * activation rows). _ldc: output row stride (>= N floats). qg_debug_sumi_tiled / qg_debug_config_tiled
 * are the parity hook and the configuration query of the same instantiation (as qg_debug_sumi /
 * qg_debug_config below). Replaces the tiled-GEMM role of include/gemm_cuda_tiled.cuh:293-300 and the
 * cp.async-staged kernels/gemm/gemm_async_copy.cuh:65-232 for reused weights.
 * DECODE ON THE TILED LAYOUT (measured, one MI355X, N = 4096, profiles/r06_tuning/r6o_ab_tiled_decode_final.txt):
 * at K = 14336 (the reference's published decode shapes) Q4_0 M = 1 / 2 / 3 / 4 / 8 run 7.77 / 8.27 / 9.10 /
 * 9.39 / 9.82 us against 7.65 / 8.84 / 10.45 / 11.31 / 10.11 on the reference rows (Q8_0 M = 4 13.49 vs 18.32)
 * — one tiled copy serves decode and prefill; at N = K = 4096 M = 1 / 2 / 3 / 4 run 3.94 / 4.18 / 4.30 / 4.38
 * against 3.39 / 3.75 / 4.21 / 4.50: a caller bound by single-token decode at such K keeps the rows for M <= 2
 * (qg_gemm_w4a8) and tiles a second copy only if its batched decode or prefill needs it.
 * Limits (QG_ERR_UNSUPPORTED, nothing launched; the tiled layout has no generic kernel): output strides
 * past INT32_MAX; M <= 4 with K > 16384 whose shape the MFMA kernel rejects too; tiled weights of a
 * (tile, stage) run count past 2^31 bytes; plain activation rows of 2 GiB or more under the windowed
 * (odd K/32) MFMA path. */
size_t qg_tile_weights_bytes(int N, int K, int wtype);
int qg_tile_weights(const void* B, void* B_tiled, int N, int K, int wtype, qg_stream_t stream);
int qg_gemm_w4a8_tiled(const void* A_q8_1, const void* B_tiled, float* C, int M, int N, int K, int wtype,
                       qg_stream_t stream);
int qg_gemm_w4a8_tiled_ldc(const void* A_q8_1, const void* B_tiled, float* C, int M, int N, int K, int64_t ldc,
                           int wtype, qg_stream_t stream);
int qg_debug_sumi_tiled(const void* A_q8_1, const void* B_tiled, int32_t* sumi, int M, int N, int K, int wtype,
                        qg_stream_t stream);
int qg_debug_config_tiled(int M, int N, int K, int wtype, int sumi, char* buf, size_t len);

/* TILED ACTIVATIONS (round 5) — the activation side of the tiled layout, for the prefill on tiled weights:
 * tokens in tiles of 16, K/32 in stages of 4 blocks, each (token tile, stage) one contiguous run of 2304 bytes
 * holding the 16 tokens' 4 block_q8_1 (token-major: token t's blocks at t * 144 + j * 36); tiles follow each
 * other tile-major, stages within a tile in order; tokens past M (to a multiple of 16) and blocks past K/32 (to
 * a multiple of 4) are zero blocks. qg_activations_tiled_bytes(M, K) sizes it. qg_quantize_q8_1_tiled writes it
 * straight from FP32 rows (16-B aligned x and A_tiled; each real block's bytes are qg_quantize_q8_1's);
 * qg_tile_activations rearranges existing Q8_1 rows into it. qg_gemm_w4a8_tiled_act(A_tiled, B_tiled, ...)
 * then computes the same product as qg_gemm_w4a8_tiled(A_q8_1, B_tiled, ...) (the same kernels and tile
 * configurations, so the same bits) with every stage of BOTH operands one linear DMA stream. _ldc, the parity
 * hook and the configuration query as for qg_gemm_w4a8_tiled. */
size_t qg_activations_tiled_bytes(int M, int K);
int qg_quantize_q8_1_tiled(const float* x, void* A_tiled, int M, int K, qg_stream_t stream);
int qg_tile_activations(const void* A_q8_1, void* A_tiled, int M, int K, qg_stream_t stream);
int qg_gemm_w4a8_tiled_act(const void* A_tiled, const void* B_tiled, float* C, int M, int N, int K, int wtype,
                           qg_stream_t stream);
int qg_gemm_w4a8_tiled_act_ldc(const void* A_tiled, const void* B_tiled, float* C, int M, int N, int K, int64_t ldc,
                               int wtype, qg_stream_t stream);
int qg_debug_sumi_tiled_act(const void* A_tiled, const void* B_tiled, int32_t* sumi, int M, int N, int K, int wtype,
                            qg_stream_t stream);
int qg_debug_config_tiled_act(int M, int N, int K, int wtype, int sumi, char* buf, size_t len);

/* W8A8: Q8_0 weights x Q8_1 activations, term sumi * d_a * d_w. Replaces gemm_w8a8_{naive,dp4a}
 * (include/gemm_cuda_naive.cuh:294-301, gemm_cuda_dp4a.cuh:418-425); device twin of
 * gemm_w8a8_reference (include/gemm_reference.h:233-267). Same as qg_gemm_w4a8(..., QG_TYPE_Q8_0). */
int qg_gemm_w8a8(const void* A_q8_1, const void* B_q8_0, float* C, int M, int N, int K, qg_stream_t stream);

/* ---- W4A16 / W8A16: FP32 activations, fp32 arithmetic -----------------
 * C[M][N] = A_f32[M][K] . dequant(B)[N][K]^T, activation-major. Replaces gemm_w4a16_{naive,tiled}
 * (include/gemm_cuda_naive.cuh:267-274, gemm_cuda_tiled.cuh:284-291) and gemm_w8a16_naive
 * (gemm_cuda_naive.cuh:276-283); device twin of gemm_w4a16_reference (gemm_reference.h:73-112).
 * Results agree with the reference to fp32 summation order (each block's products are summed,
 * then scaled by d once); the bf16-MFMA prefill (M > 8, K % 256 == 0) represents each activation
 * exactly (three bf16 parts) below K = 1024 and as two round-to-nearest bf16 parts from K = 1024
 * (added error <= 2^-16 sum_k |a_k w_k|, an eighth or less of the fp32 K-term bound
 * 2 (K + 2) 2^-24 sum_k |a_k w_k|; the high part is clamped to the largest finite bf16, so
 * activations up to FLT_MAX keep that bound and an infinite activation gives an infinite, not a NaN,
 * product). A: 4-B aligned floats (16-B for the fast path), any K % 32 == 0.
 * 8 < M <= 32 with 16-B aligned A and B, K % 256 == 0, K <= 8192 and a grid of at most one workgroup
 * per CU runs without split-K and without any workspace (round 4: each workgroup owns all of K; outputs
 * deterministic); qg_gemm_w16_workspace_size still sizes the split-K route those shapes take when the
 * operands are not 16-B aligned.
 * Prefill (M > 8, K % 256 == 0) otherwise splits K across workgroups when that fills the GPU; the partial
 * tiles live in a workspace the library allocates once per (device, stream), on the first such
 * call outside stream capture. Calls made during stream capture never use the library's
 * workspace: they run without split-K (same results to fp32 summation order), so a graph holds
 * no pointer the library may free. qg_release_workspaces() frees them (after a device synchronize;
 * call it when no other thread is inside the library, e.g. at teardown).
 * The _ws forms take the caller's workspace instead (for graphs and multi-stream callers):
 * >= qg_gemm_w16_workspace_size(M, N, K) bytes (0: no split-K for this shape), 256-B aligned,
 * zeroed once before its first use. Its layout is shape-independent: a counter region that every
 * call leaves zeroed again, then scratch partial tiles — so one workspace serves calls of any
 * shapes on one stream. Calls that may run concurrently need distinct workspaces. A smaller or
 * misaligned workspace is not used. */
void qg_release_workspaces(void);
size_t qg_gemm_w16_workspace_size(int M, int N, int K);
int qg_gemm_w4a16_ws(const float* A, const void* B_q4_0, float* C, int M, int N, int K, void* workspace,
                     size_t workspace_bytes, qg_stream_t stream);
int qg_gemm_w8a16_ws(const float* A, const void* B_q8_0, float* C, int M, int N, int K, void* workspace,
                     size_t workspace_bytes, qg_stream_t stream);
int qg_gemm_w4a16(const float* A, const void* B_q4_0, float* C, int M, int N, int K, qg_stream_t stream);
int qg_gemm_w8a16(const float* A, const void* B_q8_0, float* C, int M, int N, int K, qg_stream_t stream);
/* The kernel qg_gemm_w4a16 (wtype = QG_TYPE_Q4_0) or qg_gemm_w8a16 (QG_TYPE_Q8_0) would launch, as text like
 * qg_debug_config's (NUL-terminated, truncated to len); nothing is launched and no pointer is dereferenced. The
 * operands are the stand-in addresses A = 256 + a_off and B = 256 + b_off (the alignment rules are part of the
 * dispatch), the workspace a caller's of ws_bytes bytes as the _ws forms take it (0: none can be had, as during
 * stream capture). One line per family word — "w16d", "w16s", "w16sk", "w16mfma", "w16gemv" (SIG=m1|full: the
 * argument list), "w16gemv1r", "w16generic" — with the kernel's template arguments, grid=XxYxZ, wg= (threads per
 * workgroup), lds= (dynamic LDS bytes) and, for the split-K families, ks= (K slices), ns= or kbs= (stages or blocks
 * per slice) and ws= (workspace bytes the launch needs). Returns what the call would return before launching; an
 * empty call (M or N of 0) is QG_OK with an empty line. */
int qg_w16_config(int M, int N, int K, int wtype, int a_off, int b_off, size_t ws_bytes, char* buf, size_t len);
/* python/quant_gemm/csrc/gemm_ops.cu:431-466 gemm_q4_0_fp32_cuda(weight_q [N][K/32], activation
 * [M][K], M, N, K) -> out[M][N]: the same product, weight-first argument order. */
int qg_gemm_q4_0_fp32(const void* weight_q4_0, const float* activation, float* out, int M, int N, int K,
                      qg_stream_t stream);

/* Strided batch of independent products (e.g. the experts of an MoE layer, or several projections
 * sharing nothing): item i uses A + i*strideA, B + i*strideB (bytes) and C + i*strideC (floats).
 * One launch on the GEMV path (M <= 8), so the per-launch cost is paid once for the batch. */
int qg_gemm_w4a8_strided_batched(const void* A_q8_1, int64_t strideA, const void* B, int64_t strideB, float* C,
                                 int64_t strideC, int batch, int M, int N, int K, int wtype, qg_stream_t stream);

/* Grouped products with independent pointers and row counts (a decoder layer's Q / K / V or
 * gate / up projections; the experts an MoE step selects, when the HOST knows them -- ids that live on the
 * device: qg_gemm_w4a8_moe below): item i computes
 * C_i[m * ldc_i + n] = A_i[M][K] . B_i[N_i][K]^T (ldc_i = 0 means N_i). One M, K and weight type for
 * the group. Where QG_ALGO_AUTO picks the GEMV for every item (M <= 4 at aligned shapes), up to 64
 * items go out in ONE launch (the descriptor travels in the kernel arguments: no device
 * allocation, capture-safe, host `items` array read before return); otherwise the items are
 * enqueued one by one. Either way each C_i is bit-identical to qg_gemm_w4a8_ldc(A_i, B_i, C_i, M,
 * N_i, K, ldc_i, wtype, QG_ALGO_AUTO). Items with N_i == 0 are skipped. Replaces a host loop over
 * gemm_q4_0_q8_1_warp-style launches (kernels/gemm/gemm_warp_optimized.cuh:933-1070). */
typedef struct {
    const void* A_q8_1;  /* block_q8_1 [M][K/32] (items may share it) */
    const void* B;       /* weight blocks [N][K/32] of the group's wtype */
    float* C;            /* [M][ldc] */
    int N;
    int ldc;             /* output row stride in floats, 0 = N */
} qg_gemv_item;
int qg_gemm_w4a8_grouped(const qg_gemv_item* items, int count, int M, int K, int wtype, qg_stream_t stream);

/* Affine groups. A group of two or more items that share N and ldc and whose A, B and C pointers each advance
 * by one constant byte stride from item to item (zero or negative strides included; the A stride a multiple
 * of 4 bytes, the B stride of 16) is a strided batch, and is launched as qg_gemm_w4a8_strided_batched would
 * launch it: same kernel body, same bits, no per-item descriptor in front of the weight stream. This holds
 * for qg_gemm_w4a8_grouped and for the grouped nodes of the capture-time merge (a merged node follows the
 * calls: the strided form while they keep the progression, the general grouped kernel from the first call
 * that breaks it). mode: 0 off, 1 the shape classes measured faster (the default), 2 every class. The
 * default is read once from the environment variable QG_GROUP_AFFINE (0, 1 or 2). */
void qg_set_group_affine(int mode);

/* The route qg_gemm_w4a8_grouped(items, count, M, K, wtype) would take for its first launch, written to buf
 * (NUL-terminated, truncated to len) like qg_debug_config; nothing is enqueued and no pointer is
 * dereferenced. "gemvg ..." the grouped kernel, "gemvb ..." the strided batch's kernel (an affine group),
 * each with its template parameters and grid; "items: ..." when the items are enqueued one by one; "none"
 * when there is nothing to launch. Returns what qg_gemm_w4a8_grouped would return for the same arguments
 * before launching. */
int qg_group_config(const qg_gemv_item* items, int count, int M, int K, int wtype, char* buf, size_t len);

/* ---- expert-indexed decode GEMV: ggml_mul_mat_id for a decode step, ids read on the device ----
 * Slot s = t * n_used + u (t < T, u < n_used):
 *   e = ids[t * ids_stride + u]
 *   C[s * ldc + n] = sum_k B_experts[e][n][k] * A[t * a_rows + (u % a_rows)][k]      (n < N)
 * B_experts: n_expert dense matrices [N][K/bs] of `wtype`, one after another (ggml's [K, N, n_expert]); any of
 *    Q4_0, Q4_1, Q5_0, Q5_1, Q8_0 (bs = 32), Q4_K, Q6_K (bs = 256), MXFP4 (bs = 32, 17-byte blocks: experts at any byte).
 * A: block_q8_1 [T][a_rows][K/32], a_rows == 1 (gate / up: one row per token, shared by its slots) or
 *    a_rows == n_used (down: one row per slot).
 * ids: int32 in DEVICE memory, read by the kernel; ids_stride >= n_used elements between tokens (ggml's top-k
 *    result is a view with row stride n_expert).
 * C: float, ldc floats between slots, 0 = N.
 * A slot whose id is outside [0, n_expert) reads no weight byte and writes N times +0.0f (an expert-parallel rank
 * passes ids - first_local_expert and sums the ranks' outputs).
 * ONE launch for all T * n_used slots (the slot is a grid dimension), one workgroup-uniform load of the id per
 * workgroup. The host never reads ids; no device allocation, no synchronisation: capture-safe, and a captured
 * graph follows the ids its replay finds in the buffer. Captured, the call is a plain kernel node: the
 * capture-time merge of qg_gemm_w4a8 neither absorbs it nor merges across it.
 * Bits: each slot's N outputs are bit-identical to qg_gemm_w4a8(A_row, B_experts + e * N * K/bs * block_bytes,
 * C_row, 1, N, K, wtype, stream) called eagerly, so each inherits that product's documented bound; two launches
 * give identical bits.
 * Served shapes: those where QG_ALGO_AUTO at M = 1 picks the decode GEMV of the type ("gemv", "q4k_gemv",
 * "q6k_gemv", "mxfp4_gemv"), up to 65535 slots. QG_ERR_UNSUPPORTED, nothing launched: odd K/32 (the five 32-element types;
 * MXFP4 takes any K/32); LDS records of the activation
 * row beyond 160 KiB (Q4_K: K > 124672, Q6_K: K > 137728, MXFP4: K > 109216, the 32-element types: K > 93568); an expert stride
 * N * K/bs * block_bytes off the kernel's weight alignment; more than 65535 slots.
 * Validation, in the order of every entry: a negative T, n_used or N -> QG_ERR_INVALID_ARG; K not a positive
 * multiple of bs -> QG_ERR_BAD_K; wtype -> QG_ERR_UNSUPPORTED; T, n_used or N equal to 0 -> QG_OK, nothing touched;
 * a null pointer -> QG_ERR_INVALID_ARG; alignment -> QG_ERR_ALIGN (A and ids 4 B; B 4 B for the 32-element types,
 * 16 B for Q4_K, 2 B for Q6_K, none for MXFP4). Then a_rows not in {1, n_used}, ids_stride < n_used, n_expert < 1, ldc < 0 or
 * 0 < ldc < N -> QG_ERR_INVALID_ARG (after the precheck: an empty call is a no-op whatever they are), then the
 * unsupported shapes above.
 * qg_moe_config names the kernel the call would launch (family after "moe:", template parameters, grid) for
 * 256-B aligned buffers, launch-free; the same status codes for the shape.
 * Prefill-size T of Q4_K / Q6_K experts: qg_gemm_w4a8_moe_prefill below (this entry streams the slot's whole
 * expert matrix for every slot); slots of different tokens sharing one pass over an expert they both chose, at decode
 * sizes: qg_gemm_w4a8_moe_batch below.
 * The gate and the up product of a Q4_K / Q6_K FFN block with their GLU in one launch: qg_gemm_w4a8_moe_glu below; the
 * down product with the router-weighted sum over the token's experts in one launch: qg_gemm_w4a8_moe_down below.
 * Not built: prefill-size T and shared passes for the five 32-element types, tiled-layout experts,
 * FP32 activations. */
int qg_gemm_w4a8_moe(const void* A_q8_1, int a_rows, const void* B_experts, int n_expert, const int32_t* ids,
                     int64_t ids_stride, float* C, int64_t ldc, int T, int n_used, int N, int K, int wtype,
                     qg_stream_t stream);
int qg_moe_config(int T, int n_used, int N, int K, int wtype, char* buf, size_t len);

/* ---- expert-grouped MFMA prefill: ggml_mul_mat_id at prompt sizes, ids sorted on the device ----
 * The operands, the slot numbering s = t * n_used + u, a_rows, ids_stride and ldc (0 = N) are those of
 * qg_gemm_w4a8_moe above, and so is the result:
 *   C[s * ldc + n] = sum_k B_experts[e][n][k] * A[t * a_rows + (u % a_rows)][k],   e = ids[t * ids_stride + u]
 * and a slot whose id is outside [0, n_expert) reads no weight byte and gets N times +0.0f.
 * Two launches: a plan kernel counting-sorts the slots by expert id into `workspace` (counts, the slots in expert
 * order, one record per tile of R = 16, 32 or 64 rows of one expert), then one MFMA launch runs the Q4_K / Q6_K
 * prefill body on every tile, its activation rows gathered and its output rows scattered through the sorted list:
 * an expert's matrix is read once per tile of R slots instead of once per slot. The MFMA launch's grid is the
 * host's upper bound floor(slots / R) + min(n_expert + 1, slots) on the number of tiles; workgroups past the true
 * number return at once.
 * The host never reads ids; no allocation, no synchronisation: capture-safe (two kernel nodes), and a replayed graph
 * follows the ids it finds, with another number of rows per expert and of tiles on every replay.
 * Bits: an output's arithmetic is that of the "q4k_mmq" / "q6k_mmq" family at the call's RG (qg_moe_prefill_config)
 * on its own activation row and weight row; it does not depend on the tile's size or on where the sort put the
 * slot, so two launches give identical bits and each output inherits the MFMA prefill's documented bound.
 * Served: wtype QG_TYPE_Q4_K or QG_TYPE_Q6_K (the five 32-element types: QG_ERR_UNSUPPORTED), K % 256 == 0,
 * n_expert <= 4096, at most 65535 slots, any N. QG_ERR_UNSUPPORTED beyond, and for an expert stride
 * N * K/256 * block_bytes off the kernel's weight alignment (16 B for Q4_K, never for Q6_K).
 * workspace: device memory, 16-B aligned, at least qg_gemm_w4a8_moe_prefill_workspace_size(T, n_used, n_expert)
 * bytes (a function of these three alone, monotone in each; 0 where one of them is <= 0). It holds only what the
 * plan writes: the call reads nothing from it that the same call has not written, so its previous content is
 * arbitrary. In use until the call's kernels finish: calls on one stream may share it, concurrent streams need one
 * each.
 * Validation: the order of qg_gemm_w4a8_moe (precheck with the type check -- here Q4_K / Q6_K only -- then a_rows /
 * ids_stride / n_expert / ldc), then workspace == NULL -> QG_ERR_INVALID_ARG, workspace off 16 B -> QG_ERR_ALIGN,
 * workspace_bytes below the size function -> QG_ERR_INVALID_ARG, then the unsupported shapes. An empty call (T,
 * n_used or N equal to 0) is QG_OK and touches nothing, whatever the later arguments are.
 * qg_moe_prefill_config names the launch ("moe:q4k_mmq" / "moe:q6k_mmq", TT, RG, KS, R = 16 TT rows per tile, grid =
 * row tiles x the upper bound above), launch-free, the same status codes for the shape. (TT, RG) is chosen from
 * (T, n_used, n_expert, N, K, wtype, CU count): slots / n_expert (rounded up) <= 16 -> (1, 1), <= 32 -> (2, 1),
 * beyond (4, 4) once ceil(N / 64) * ceil(slots / 64) fills the CUs, else (4, 1); Q6_K at K <= 1024 always (4, 4).
 * Which entry for which T (measured on an MI355X with a uniform router): with 8 experts, 2 used
 * (Mixtral, N x K = 14336 x 4096 and 4096 x 14336) this entry is below qg_gemm_w4a8_moe from T = 16 on (the smallest
 * T measured; 0.67 .. 0.87 of it there, 0.09 .. 0.16 at T = 1024); with 128 experts, 8 used (Qwen3-MoE, 768 x 2048 and
 * 2048 x 768) from T = 256 on (at T = 64 it takes 1.1 .. 2.2 times as long: two slots per expert leave nothing to
 * share). As a rule: this entry once slots / n_expert reaches 16, qg_gemm_w4a8_moe below 4; between them it depends on
 * the expert's size (ahead at 4 with Mixtral's 33 MB Q4_K experts, behind at 4 with Qwen3-MoE's 0.9 MB ones).
 * qg_debug_moe_prefill_plan runs the plan alone for the tile size the product would use and copies the n_expert + 1
 * counts (the last: the invalid bin) and the T * n_used sorted slots (the invalid bin's last) to caller device
 * buffers; for tests, no stable layout promise.
 * Not built: the five 32-element types (their MFMA kernel stages through LDS-DMA from linear bases), tiled-layout
 * experts, FP32 activations, an automatic choice between the entries, the plan fused into the router. */
size_t qg_gemm_w4a8_moe_prefill_workspace_size(int T, int n_used, int n_expert);
int qg_gemm_w4a8_moe_prefill(const void* A_q8_1, int a_rows, const void* B_experts, int n_expert, const int32_t* ids,
                             int64_t ids_stride, float* C, int64_t ldc, int T, int n_used, int N, int K, int wtype,
                             void* workspace, size_t workspace_bytes, qg_stream_t stream);
int qg_moe_prefill_config(int T, int n_used, int n_expert, int N, int K, int wtype, char* buf, size_t len);
int qg_debug_moe_prefill_plan(const int32_t* ids, int64_t ids_stride, int T, int n_used, int n_expert, int a_rows, int N,
                              int K, int wtype, int32_t* counts, int32_t* sorted, void* workspace,
                              size_t workspace_bytes, qg_stream_t stream);

/* ---- expert-grouped decode GEMV: ggml_mul_mat_id for batched decode, ids sorted on the device ----
 * The operands, the slot numbering s = t * n_used + u, a_rows, ids_stride and ldc (0 = N) are those of
 * qg_gemm_w4a8_moe above, and so is the result:
 *   C[s * ldc + n] = sum_k B_experts[e][n][k] * A[t * a_rows + (u % a_rows)][k],   e = ids[t * ids_stride + u]
 * and a slot whose id is outside [0, n_expert) reads no weight byte and gets N times +0.0f.
 * Two launches: the plan kernel of qg_gemm_w4a8_moe_prefill counting-sorts the slots by expert id into `workspace`,
 * here with tiles of R = 2, 4 or 8 rows of one expert; then one launch runs the Q4_K / Q6_K decode GEMV body on every
 * tile (MT = R activation rows per weight pass), its activation rows gathered into the LDS records and its output rows
 * scattered through the sorted list: slots of different tokens that chose the same expert share one pass over its
 * matrix. The GEMV launch's grid is row tiles x the host's upper bound floor(slots / R) + min(n_expert + 1, slots) on
 * the number of tiles; workgroups past the true number return at once.
 * The host never reads ids; no allocation, no synchronisation: capture-safe (two kernel nodes), and a replayed graph
 * follows the ids it finds, with another number of rows per expert and of tiles on every replay.
 * Bits: every slot's N outputs are bit-identical to qg_gemm_w4a8_moe on the same operands, so also to the eager M = 1
 * qg_gemm_w4a8: the arithmetic is that of the "q4k_gemv" / "q6k_gemv" family at the single call's LPR, WGS and ONE, a
 * token's accumulation chain is its own, and nothing depends on R, on the tile or on where the sort put the slot. Each
 * output inherits the decode GEMV's documented bound.
 * R is a function of (T, n_used, n_expert, K, wtype) alone: per = ceil(slots / n_expert) <= 2 -> 2, <= 4 -> 4, else 8,
 * then halved until R * K/256 records (336 B for Q4_K, 304 B for Q6_K) fit 160 KiB of LDS: Q4_K takes R = 8 up to
 * K = 15360 and R = 4 up to K = 30976, Q6_K R = 8 up to K = 17152 and R = 4 up to K = 34304.
 * Served: wtype QG_TYPE_Q4_K or QG_TYPE_Q6_K (the five 32-element types: QG_ERR_UNSUPPORTED), K % 256 == 0,
 * n_expert <= 4096, at most 65535 slots, any N. QG_ERR_UNSUPPORTED, nothing launched: beyond these; the shapes
 * qg_gemm_w4a8_moe refuses; K whose records of two rows exceed the LDS (Q4_K: K > 62208, Q6_K: K > 68864); an expert
 * stride N * K/256 * block_bytes off the kernel's weight alignment (16 B for Q4_K, never for Q6_K); a tile bound
 * beyond 65535 (not reachable within the bounds above).
 * workspace: device memory, 16-B aligned, at least qg_gemm_w4a8_moe_batch_workspace_size(T, n_used, n_expert) bytes (a
 * function of these three alone, monotone in each; 0 where one of them is <= 0; larger than the prefill's, whose
 * tile records are sized for R = 16: 4 + bins + 2 slots + 4 max_tiles(R = 2) int32, each region rounded up to 16 B).
 * It holds only what the plan writes; its previous content is arbitrary. In use until the call's kernels finish:
 * calls on one stream may share it, concurrent streams need one each.
 * Validation: the order of qg_gemm_w4a8_moe_prefill: the precheck with the type check (Q4_K / Q6_K only), a_rows /
 * ids_stride / n_expert / ldc -> QG_ERR_INVALID_ARG, workspace == NULL -> QG_ERR_INVALID_ARG, workspace off 16 B ->
 * QG_ERR_ALIGN, workspace_bytes below the size function -> QG_ERR_INVALID_ARG, then the unsupported shapes. An empty
 * call (T, n_used or N equal to 0) is QG_OK and touches nothing, whatever the later arguments are.
 * qg_moe_batch_config names the launch ("moeb:q4k_gemv" / "moeb:q6k_gemv", R, LPR, WGS, ONE, grid, lds), launch-free,
 * the same status codes for the shape.
 * Which of the three entries for which T: measured on an MI355X with a uniform router (DESIGN.md 3e,
 * profiles/moe_batch/ab_moe_batch.txt; per = slots / n_expert). per <= 1: qg_gemm_w4a8_moe (this entry takes 1.05 ..
 * 1.6 times as long with Qwen3-MoE's 128 experts, 0.95 .. 1.08 with Mixtral's 8). per = 2 .. 4: this entry, in all 16
 * measured classes (0.58 .. 0.97 of the better of the two others). per = 8 .. 16: this entry where experts are small
 * (Qwen3-MoE, 0.9 .. 1.3 MB: 0.38 .. 0.85), qg_gemm_w4a8_moe_prefill where they are large (Mixtral, 33 .. 48 MB: this
 * entry at 1.03 .. 1.56 of it, below it only for Q6_K gate/up, 0.79 and 0.97). per >= 32: qg_gemm_w4a8_moe_prefill
 * (this entry at 1.1 .. 2.4 of it on Mixtral; not measured on Qwen3-MoE, T > 256).
 * Not built: the five 32-element types (their GEMV body is a function shared by many shipped kernels), one plan shared
 * by the gate / up / down products of a layer, an automatic choice between the three entries, tiled-layout experts,
 * FP32 activations. */
size_t qg_gemm_w4a8_moe_batch_workspace_size(int T, int n_used, int n_expert);
int qg_gemm_w4a8_moe_batch(const void* A_q8_1, int a_rows, const void* B_experts, int n_expert, const int32_t* ids,
                           int64_t ids_stride, float* C, int64_t ldc, int T, int n_used, int N, int K, int wtype,
                           void* workspace, size_t workspace_bytes, qg_stream_t stream);
int qg_moe_batch_config(int T, int n_used, int n_expert, int N, int K, int wtype, char* buf, size_t len);

/* ---- fused gate / up mul_mat_id with its GLU: the first half of an MoE FFN block in one launch ----
 * down(act(gate(x)) * up(x)) starts with two mul_mat_id on the same ids, the same activation row and the same shape,
 * and an elementwise GLU on their results. This entry replaces those three kernels (qg_gemm_w4a8_moe on the gate
 * experts, qg_gemm_w4a8_moe on the up experts, the caller's activation kernel) for Q4_K / Q6_K experts.
 * Slot s = t * n_used + u (t < T, u < n_used), e = ids[t * ids_stride + u]:
 *   g = sum_k B_gate[e][n][k] * A[t][k],   u = sum_k B_up[e][n][k] * A[t][k]
 *   C[s * ldc + n] = QG_GLU_REGLU:  (g > 0 ? g : 0.0f) * u
 *                    QG_GLU_SWIGLU: (g / (1.0f + expf(-g))) * u                         (n < N)
 * A: block_q8_1 [T][K/32], one row per token (there is no a_rows: gate and up always share the token's row).
 * B_gate, B_up: n_expert dense matrices [N][K/256] each, both of `wtype`, QG_TYPE_Q4_K or QG_TYPE_Q6_K; they may alias.
 * ids, ids_stride, C and ldc (0 = N) are those of qg_gemm_w4a8_moe.
 * Bits: g and u are the values qg_gemm_w4a8_moe gives for the slot on B_gate and on B_up, bit for bit (the kernel runs
 * the same decode GEMV body twice, at the same LPR, WGS and ONE); each operation of the op is then one rounded fp32
 * operation (no contraction), the division correctly rounded, expf the device library's (within 1 ulp; for g < -88.72
 * it overflows and the result is +-0 where the true |value| is below 2^-121). Two launches give identical bits.
 * A slot whose id is outside [0, n_expert) reads no weight byte and writes N times +0.0f, for either op.
 * ONE launch, a single kernel node when captured. The host never reads ids; no device allocation, no synchronisation:
 * capture-safe, and a replayed graph follows the ids it finds in the buffer.
 * Validation: the order of qg_gemm_w4a8_moe: a negative T, n_used or N -> QG_ERR_INVALID_ARG; K not a positive multiple
 * of 256 (32 where wtype is no super-block type) -> QG_ERR_BAD_K; wtype other than Q4_K / Q6_K (the five 32-element
 * types among them) -> QG_ERR_UNSUPPORTED; T, n_used or N equal to 0 -> QG_OK, nothing touched; a null pointer ->
 * QG_ERR_INVALID_ARG; alignment -> QG_ERR_ALIGN (A and ids 4 B; B_gate and B_up alike 16 B for Q4_K, 2 B for Q6_K).
 * Then ids_stride < n_used, n_expert < 1, ldc < 0 or 0 < ldc < N -> QG_ERR_INVALID_ARG; then more than 65535 slots or an
 * expert stride off the weight alignment -> QG_ERR_UNSUPPORTED; then the entry's own refusals, QG_ERR_UNSUPPORTED with
 * nothing launched: a glu_op other than QG_GLU_REGLU / QG_GLU_SWIGLU, a shape that QG_ALGO_AUTO at M = 1 does not send
 * to the type's decode GEMV (LDS records beyond 160 KiB: Q4_K K > 124672, Q6_K K > 137728).
 * qg_moe_glu_config names the launch ("moe_glu:q4k_gemv" / "moe_glu:q6k_gemv", LPR, WGS, ONE, grid, lds: those of
 * qg_moe_config for the same N, K and type; the op is no part of the launch's shape), launch-free; the same status
 * codes for the shape.
 * Standing against the three-kernel sequence (MI355X, uniform router): DESIGN.md 3f, profiles/moe_glu/.
 * Not built: the five 32-element types, a dense (no ids) GLU entry, GEGLU, a Q8_1-quantized output for the down
 * product, fused forms of the prefill and batch entries. (The weighted sum over experts after down:
 * qg_gemm_w4a8_moe_down below.) */
#define QG_GLU_REGLU  0   /* numbered as ggml's enum ggml_glu_op */
#define QG_GLU_SWIGLU 2
int qg_gemm_w4a8_moe_glu(const void* A_q8_1, const void* B_gate, const void* B_up, int n_expert, const int32_t* ids,
                         int64_t ids_stride, float* C, int64_t ldc, int T, int n_used, int N, int K, int wtype, int glu_op,
                         qg_stream_t stream);
int qg_moe_glu_config(int T, int n_used, int N, int K, int wtype, char* buf, size_t len);

/* ---- down mul_mat_id with the weighted expert sum: the second half of an MoE FFN block in one launch ----
 * sum_u w[t,u] * down_e(h[t,u]) is a mul_mat_id with one activation row per slot, the caller's multiply by the router
 * weights and the caller's sum over the token's n_used slots. This entry replaces those kernels (qg_gemm_w4a8_moe at
 * a_rows = n_used, which writes T * n_used * N floats that are read back once) for Q4_K / Q6_K experts. With
 * qg_gemm_w4a8_moe_glu an MoE FFN block at decode is four calls: quantize, moe_glu, quantize, moe_down.
 * Token t < T, slot u < n_used, e_u = ids[t * ids_stride + u]:
 *   d_u[n] = sum_k B_experts[e_u][n][k] * A[t * n_used + u][k]
 *   acc = +0.0f; for u = 0 .. n_used - 1 in ascending order, where 0 <= e_u < n_expert:
 *       acc = acc + weights[t * w_stride + u] * d_u[n]
 *   C[t * ldc + n] = acc                                                                      (n < N)
 * A: block_q8_1 [T][n_used][K/32], one row per slot (there is no a_rows: the a_rows = n_used case of qg_gemm_w4a8_moe).
 * B_experts, ids and ids_stride are those of qg_gemm_w4a8_moe; wtype QG_TYPE_Q4_K or QG_TYPE_Q6_K.
 * weights: float in DEVICE memory, 4-B aligned, w_stride >= n_used floats between tokens. NULL: every weight is 1.0f,
 *    the plain sum over the token's experts, bit-equal to passing ones (w_stride is then not looked at).
 * C: float [T][ldc], ONE row per token (not per slot), ldc = 0 means N.
 * Bits: d_u is the value qg_gemm_w4a8_moe(A, a_rows = n_used, ...) gives slot t * n_used + u at row n, bit for bit (the
 * kernel runs the same decode GEMV body at the same LPR and ONE); the multiplication and the addition of the fold are
 * each one rounded fp32 operation (no contraction), in ascending u as llama.cpp adds the experts. Two launches give
 * identical bits.
 * A slot whose id is outside [0, n_expert) reads no weight byte and contributes nothing: its weights value is not read,
 * so an inf or a NaN there does not reach the output. A token with no id in range gets N times +0.0f.
 * ONE launch, a single kernel node when captured. The host reads neither ids nor weights; no device allocation, no
 * synchronisation: capture-safe, and a replayed graph follows the ids and the weights it finds in the buffers.
 * Validation: the order of qg_gemm_w4a8_moe: a negative T, n_used or N -> QG_ERR_INVALID_ARG; K not a positive multiple
 * of 256 (32 where wtype is no super-block type) -> QG_ERR_BAD_K; wtype other than Q4_K / Q6_K (the five 32-element
 * types among them) -> QG_ERR_UNSUPPORTED; T, n_used or N equal to 0 -> QG_OK, nothing touched; a null A, B_experts,
 * ids or C -> QG_ERR_INVALID_ARG; alignment -> QG_ERR_ALIGN (A, ids and a non-null weights 4 B; B_experts 16 B for Q4_K,
 * 2 B for Q6_K). Then ids_stride < n_used, n_expert < 1, ldc < 0 or 0 < ldc < N, w_stride < n_used with non-null
 * weights -> QG_ERR_INVALID_ARG; then T > 65535 (the token is the grid's y; the number of slots is not bounded) or an
 * expert stride off the weight alignment -> QG_ERR_UNSUPPORTED; then the entry's own refusals, QG_ERR_UNSUPPORTED with
 * nothing launched: a shape that QG_ALGO_AUTO at M = 1 does not send to the type's decode GEMV; an LDS need beyond
 * 160 KiB. The workgroup keeps the records of all n_used activation rows (336 B per 256 elements for Q4_K, 304 B for
 * Q6_K) and n_used x RPB products: n_used * (K/256 * record + 4 RPB) bytes, RPB <= 64 the rows per workgroup
 * (qg_moe_down_config). The largest K served, by n_used:
 *   n_used      1       2      4      6      8     10     16     32
 *   Q4_K   124672   62208  30976  20736  15360  12288   7680   3840
 *   Q6_K   137728   68864  34304  22784  17152  13568   8448   4096
 * qg_moe_down_config names the launch ("moe_down:q4k_gemv" / "moe_down:q6k_gemv", LPR, WGS and ONE: those of
 * qg_moe_config for the same K and type; SW: the waves of a workgroup that stand side by side on the slots of one row
 * group, the largest power of two <= min(n_used, WGS / 64); grid = ceil(N / RPB) x T with RPB = (WGS / 64 / SW) *
 * (64 / LPR); lds), launch-free; the same status codes for the shape.
 * Which to use (measured on an MI355X with a uniform router against qg_gemm_w4a8_moe plus torch's multiply and sum,
 * DESIGN.md 3g, profiles/moe_down/ab_moe_down.txt): this entry at Qwen3-MoE's shape (N x K = 2048 x 768, 8 of 128
 * experts), both types, T = 1 and T = 8 (0.64 .. 0.78 of the sequence's time captured, 0.65 .. 0.78 eager), and at
 * Mixtral's (4096 x 14336, 2 of 8) at T = 1 (0.76 Q4_K, 0.89 Q6_K captured). It is NOT ahead at Mixtral's shape at
 * T = 8, where the weight stream and not the launch count is the time: 1.05 (Q4_K) and 1.17 (Q6_K) times the
 * sequence's time; keep qg_gemm_w4a8_moe and the caller's sum there. In all but one class the launch takes longer than
 * the sequence's product launch alone (1.01 .. 1.40 of it captured): what it saves is the two elementwise kernels and
 * the round trip of the T * n_used * N floats, not time in the product.
 * Not built: the five 32-element types, FP32 input quantized in the prologue, a Q8_1-writing GLU ahead of it, fused
 * forms of the prefill and batch entries. */
int qg_gemm_w4a8_moe_down(const void* A_q8_1, const void* B_experts, int n_expert, const int32_t* ids, int64_t ids_stride,
                          const float* weights, int64_t w_stride, float* C, int64_t ldc, int T, int n_used, int N, int K,
                          int wtype, qg_stream_t stream);
int qg_moe_down_config(int T, int n_used, int N, int K, int wtype, char* buf, size_t len);

/* ---- the two fused FFN entries with per-expert bias, gpt-oss's clamped SwiGLU and MXFP4 experts ----
 * A gpt-oss FFN block is g = gate_e(x) + bg[e], u = up_e(x) + bu[e], h = swiglu_oai(g, u), d = down_e(h) + bd[e],
 * y = sum_u w[t,u] * d_u. These two entries are qg_gemm_w4a8_moe_glu and qg_gemm_w4a8_moe_down above with the bias rows
 * and the third op, for wtype QG_TYPE_Q4_K, QG_TYPE_Q6_K or QG_TYPE_MXFP4 (which the two above refuse): the block at
 * decode is again four calls, quantize, moe_glu_bias, quantize, moe_down_bias. Everything not said here (operands, slot
 * numbering, ids, ldc, weights, an id outside [0, n_expert), capture, the host reading nothing) is as above.
 * Bias: float [n_expert][bias_stride] in DEVICE memory, 4-B aligned, bias_stride = 0 means N. Each bias pointer may be
 * NULL on its own: no add for that operand (not an add of 0.0f: -0.0f stays -0.0f).
 * qg_gemm_w4a8_moe_glu_bias, slot s = t * n_used + u, e = ids[t * ids_stride + u], g and u the two products:
 *   g = g + bias_gate[e * bias_stride + n]   (bias_gate != NULL)      u = u + bias_up[e * bias_stride + n]   (bias_up != NULL)
 *   C[s * ldc + n] = QG_GLU_REGLU, QG_GLU_SWIGLU: as qg_gemm_w4a8_moe_glu
 *                    QG_GLU_SWIGLU_OAI: x = fminf(g, limit); y = fminf(fmaxf(u, -limit), limit);
 *                                       (x / (1.0f + expf(alpha * (-x)))) * (y + 1.0f)
 *   alpha and limit are read for QG_GLU_SWIGLU_OAI alone (gpt-oss: 1.702f, 7.0f). Each step is one rounded fp32
 *   operation. An id outside [0, n_expert) stores +0.0f: no bias is read or applied.
 * qg_gemm_w4a8_moe_down_bias: d_u[n] = d_u[n] + bias[e_u * bias_stride + n] (one rounded add) ahead of the fold
 *   acc = acc + weights[t * w_stride + u] * d_u[n], which is unchanged. An id outside [0, n_expert) contributes nothing:
 *   neither its bias nor its weight is read.
 * Bits: g, u and d_u are those of qg_gemm_w4a8_moe on the same operands (MXFP4: the "moe:mxfp4_gemv" body at the
 * single call's LPR, WGS and ONE for K / 32 units). With Q4_K / Q6_K and null biases the outputs are bit-identical to
 * qg_gemm_w4a8_moe_glu / qg_gemm_w4a8_moe_down.
 * MXFP4 weights need no alignment: B_gate, B_up, B_experts and the expert stride N * K/32 * 17 are any number of bytes.
 * Validation: the order of the two entries above, with K a positive multiple of 32 for MXFP4; a non-null bias off 4 B
 * -> QG_ERR_ALIGN beside the other pointers; bias_stride < 0 or 0 < bias_stride < N -> QG_ERR_INVALID_ARG beside
 * ids_stride (whether or not a bias is given), and there too, for QG_GLU_SWIGLU_OAI, an alpha that is not finite or a
 * limit that is not finite and > 0; then the QG_ERR_UNSUPPORTED shapes of moe_front; then the entry's own refusals,
 * QG_ERR_UNSUPPORTED with nothing launched: a glu_op other than the three, a shape that QG_ALGO_AUTO at M = 1 does not
 * send to the type's decode GEMV, for down an LDS need beyond 160 KiB. MXFP4's need is
 * n_used * (K/32 * 48 + 4 RPB) bytes; the largest K served, by n_used:
 *   n_used        1       2       3       4       6       8      10      16      32
 *   MXFP4    109184   54592   36384   27296   18176   13632   10912    6816    3392
 * (Q4_K / Q6_K: the table of qg_gemm_w4a8_moe_down.)
 * qg_moe_glu_bias_config / qg_moe_down_bias_config: for Q4_K / Q6_K the strings of qg_moe_glu_config /
 * qg_moe_down_config (bias and op are no part of the launch's shape); for MXFP4 "moe_glu:mxfp4_gemv ..." and
 * "moe_down:mxfp4_gemv ... SW=...", LPR / WGS / ONE those of qg_moe_config for the same K, SW and RPB by the rule above.
 * Which to use (measured on an MI355X with a uniform router at gpt-oss's N = K = 2880, MXFP4, 4 of 32 and 4 of 128
 * experts, against the unfused sequence on the same operands -- qg_gemm_w4a8_moe twice, torch's two gathered bias adds
 * and a torch swiglu_oai for glu; qg_gemm_w4a8_moe at a_rows = n_used, torch's gathered bias add, multiply and sum for
 * down; DESIGN.md 3i, profiles/mxfp4_ffn/ab_mxfp4_ffn.txt): qg_gemm_w4a8_moe_glu_bias at T = 1 (0.38 of the sequence's
 * time captured, 0.26 eager) and at T = 8 (0.73 .. 0.75 both ways); qg_gemm_w4a8_moe_down_bias at T = 1 (0.51 captured,
 * 0.51 .. 0.52 eager). At T = 8 the down entry is NOT ahead beyond what a run resolves: 0.97 .. 1.00 of the sequence's
 * time with overlapping ranges; the weight stream is the time there, and either form serves. For Q4_K / Q6_K without
 * bias prefer qg_gemm_w4a8_moe_glu / qg_gemm_w4a8_moe_down: with null biases the new entries give the same bits in
 * 1.00 .. 1.01 of their time captured at Qwen3-MoE's shape (glu at T = 1: 7.10 against 7.03 us, outside that run's
 * spread of 0.02; the other three classes within it).
 * Not built: FP32-input or Q8_1-writing fused forms, GEGLU, a dense (no ids) GLU entry, an MXFP4 quantizer (MXFP4 in
 * the prefill and batch entries: the two _bias entries below). */
#define QG_GLU_SWIGLU_OAI 3   /* beside QG_GLU_REGLU 0 / QG_GLU_SWIGLU 2 */
int qg_gemm_w4a8_moe_glu_bias(const void* A_q8_1, const void* B_gate, const void* B_up, const float* bias_gate,
                              const float* bias_up, int64_t bias_stride, int n_expert, const int32_t* ids, int64_t ids_stride,
                              float* C, int64_t ldc, int T, int n_used, int N, int K, int wtype, int glu_op, float alpha,
                              float limit, qg_stream_t stream);
int qg_moe_glu_bias_config(int T, int n_used, int N, int K, int wtype, char* buf, size_t len);
int qg_gemm_w4a8_moe_down_bias(const void* A_q8_1, const void* B_experts, const float* bias, int64_t bias_stride, int n_expert,
                               const int32_t* ids, int64_t ids_stride, const float* weights, int64_t w_stride, float* C,
                               int64_t ldc, int T, int n_used, int N, int K, int wtype, qg_stream_t stream);
int qg_moe_down_bias_config(int T, int n_used, int N, int K, int wtype, char* buf, size_t len);

/* ---- the two expert-grouped entries with per-expert bias and MXFP4 experts ----
 * qg_gemm_w4a8_moe_prefill and qg_gemm_w4a8_moe_batch above with ggml's add_id folded in, for wtype QG_TYPE_Q4_K,
 * QG_TYPE_Q6_K or QG_TYPE_MXFP4 (which the two above refuse): what a gpt-oss FFN block needs beyond a handful of tokens,
 * where each of its three products is followed by a per-expert bias. With e = ids[t * ids_stride + u], s = t * n_used + u:
 *   C[s * ldc + n] = (sum_k B[e][n][k] * A[t * a_rows + u % a_rows][k]) + bias[e * bias_stride + n]
 * The add is one rounded fp32 addition on the finished product. bias: float [n_expert][bias_stride] in DEVICE memory,
 * 4-B aligned, bias_stride = 0 means N. bias == NULL: no addition at all (not an add of 0.0f: a -0.0f product stays
 * -0.0f). An id outside [0, n_expert) gives N times +0.0f: no weight byte and no bias is read.
 * Everything else is the contract of the entry each stands beside: slot numbering, a_rows, ids_stride, ldc, the limits
 * of 65535 slots and 4096 experts, the workspace (qg_gemm_w4a8_moe_prefill_workspace_size /
 * qg_gemm_w4a8_moe_batch_workspace_size serve these entries too, with the same rules), capture (the host never reads
 * ids; a replay follows the ids it finds), an empty call QG_OK.
 * MXFP4 weights need no alignment: B_experts and the expert stride N * K/32 * 17 are any number of bytes; K is a positive
 * multiple of 32 (Q4_K / Q6_K: of 256, with their alignment rules).
 * Validation: the order of the entry beside it; a non-null bias off 4 B -> QG_ERR_ALIGN beside the other pointers;
 * bias_stride < 0 or 0 < bias_stride < N -> QG_ERR_INVALID_ARG beside ids_stride (whether or not a bias is given); then
 * the workspace checks; then the QG_ERR_UNSUPPORTED shapes.
 * qg_gemm_w4a8_moe_prefill_bias, family "moe:mxfp4_mmq" for MXFP4: the plan, tiles and forms of
 *   qg_gemm_w4a8_moe_prefill; (TT, RG) by its general rule (not the Q6_K one), whose thresholds were measured for the
 *   K-quants. Bits: every product has the bits of the eager "mxfp4_mmq" product at the same RG on its own activation row
 *   and weight row, whatever TT, the tile and the slot's position; two launches give identical bits. Q4_K / Q6_K: the
 *   products of qg_gemm_w4a8_moe_prefill, bit for bit (with a null bias, its launch).
 * qg_gemm_w4a8_moe_batch_bias, family "moeb:mxfp4_gemv" for MXFP4: the plan and tiles of qg_gemm_w4a8_moe_batch; LPR, WGS
 *   and ONE those of qg_moe_config for the same K. An LDS record is one block, 48 B, so a tile needs R * K/32 * 48 bytes:
 *   R = 8 up to K = 13632, R = 4 up to K = 27296, R = 2 up to K = 54592, beyond that QG_ERR_UNSUPPORTED (Q4_K / Q6_K: the
 *   thresholds of qg_gemm_w4a8_moe_batch). Bits: every product is bit-identical to qg_gemm_w4a8_moe on the same operands.
 * qg_moe_prefill_bias_config / qg_moe_batch_bias_config: for Q4_K / Q6_K the strings of qg_moe_prefill_config /
 * qg_moe_batch_config (the bias is no part of the launch's shape); for MXFP4 "moe:mxfp4_mmq TT=.. RG=.. KS=.. R=..
 * grid=XxY" and "moeb:mxfp4_gemv R=.. LPR=.. WGS=.. ONE=.. grid=XxY lds=..".
 * A gpt-oss FFN block at prompt size: quantize, qg_gemm_w4a8_moe_prefill_bias twice (gate, up), the caller's clamped
 * SwiGLU, quantize, qg_gemm_w4a8_moe_prefill_bias (down, a_rows = n_used), the caller's weighted sum.
 * Which entry for which T (measured on an MI355X at gpt-oss's N = K = 2880, MXFP4, uniform router, captured, against
 * qg_gemm_w4a8_moe plus torch's gathered bias add on the same operands; DESIGN.md 3j,
 * profiles/moe_id_bias/ab_moe_id_bias.txt). 4 of 32 experts: qg_gemm_w4a8_moe_batch_bias from T = 8 (0.89 of the
 * sequence's time) through T = 64 (0.37), where qg_gemm_w4a8_moe_prefill_bias draws level (0.41) and then leads: 0.31 at
 * T = 256, 0.08 at T = 1024. 4 of 128 experts: the batch entry from T = 32 (0.91; 0.75 at T = 64), the prefill entry
 * from T = 256 (0.38; 0.30 at T = 1024). NOT ahead, keep qg_gemm_w4a8_moe and the caller's add: the prefill entry at
 * T = 16 (1.35 and 2.24 of the sequence's time) and at T = 64 with 128 experts (1.25); the batch entry with 128 experts
 * at T = 8 and 16 (1.07, 1.02). The prefill's (TT, RG) thresholds are the K-quants' and do not suit MXFP4 everywhere: at
 * T = 256 with 32 experts the rule's (2, 1) takes 2.1 times as long as a forced (4, 4). Q4_K / Q6_K with a bias cost a
 * third launch (an add kernel behind the unbiased entries' kernels): a convenience there, not a saving.
 * Not built: a fused GLU at prefill or batch size, one plan shared by the three products of a layer, an automatic choice
 * between the entries, the 32-element types in these entries, an MXFP4 quantizer. */
int qg_gemm_w4a8_moe_prefill_bias(const void* A_q8_1, int a_rows, const void* B_experts, const float* bias, int64_t bias_stride,
                                  int n_expert, const int32_t* ids, int64_t ids_stride, float* C, int64_t ldc, int T, int n_used,
                                  int N, int K, int wtype, void* workspace, size_t workspace_bytes, qg_stream_t stream);
int qg_moe_prefill_bias_config(int T, int n_used, int n_expert, int N, int K, int wtype, char* buf, size_t len);
int qg_gemm_w4a8_moe_batch_bias(const void* A_q8_1, int a_rows, const void* B_experts, const float* bias, int64_t bias_stride,
                                int n_expert, const int32_t* ids, int64_t ids_stride, float* C, int64_t ldc, int T, int n_used,
                                int N, int K, int wtype, void* workspace, size_t workspace_bytes, qg_stream_t stream);
int qg_moe_batch_bias_config(int T, int n_used, int n_expert, int N, int K, int wtype, char* buf, size_t len);

/* ---- weight-major twins (kernels/gemm/gemm_quant_formats.cuh:343-428) ---------------------
 * out[M][N] = W[M][K/32] . A[N][K/32]^T, M = weight rows, N = tokens. */
int qg_gemm_q4_0_q8_1(const void* W, const void* A_q8_1, float* out, int M, int N, int K, qg_stream_t stream);
int qg_gemm_q4_1_q8_1(const void* W, const void* A_q8_1, float* out, int M, int N, int K, qg_stream_t stream);
int qg_gemm_q5_0_q8_1(const void* W, const void* A_q8_1, float* out, int M, int N, int K, qg_stream_t stream);
int qg_gemm_q5_1_q8_1(const void* W, const void* A_q8_1, float* out, int M, int N, int K, qg_stream_t stream);
int qg_gemm_q8_0_q8_1(const void* W, const void* A_q8_1, float* out, int M, int N, int K, qg_stream_t stream);

/* ---- fused activation quantization --------------------------------------
 * Activation-major C[M][N] = Q8_1(X)[M][K] . B[N][K]^T for FP32 activations X[M][K] (dense rows),
 * quantized as quantize_row_q8_1_ref (include/quantize.h:165-193): the results are bit-identical to
 * qg_quantize_q8_1(X) followed by qg_gemm_w4a8 on the same stream.
 *   M <= 4 (X 16-B aligned): ONE launch, the quantization runs in the GEMV prologue (the Q8_1
 *     activations never go through HBM);
 *   otherwise (larger M, or a K the GEMV does not take), with workspace_bytes >=
 *     qg_gemm_w4a8_f32_workspace_size(M, K): quantize into the workspace (4-B aligned device
 *     memory), then the QG_ALGO_AUTO product;
 *   larger M without a workspace: the fused GEMV over 8-row chunks (weights streamed per chunk).
 * X only 4-B aligned is served through the workspace; without one it is QG_ERR_ALIGN. */
size_t qg_gemm_w4a8_f32_workspace_size(int M, int K);
int qg_gemm_w4a8_f32(const float* X, const void* B, float* C, int M, int N, int K, int wtype, void* workspace,
                     size_t workspace_bytes, qg_stream_t stream);

/* Replaces gemm_q4_0_fp16_fused(weight, fp16_activation, output, M, N, K, stream)
 * (kernels/gemm/gemm_fused.cuh:311-338), weight-major: out[M][N] = W_q4_0[M][K/32] .
 * Q8_1(act[N][K])^T, act IEEE half [N tokens][K], quantized with the fused kernel's semantics
 * (gemm_fused.cuh:76-143: tree-reduced amax/sum, id = 1/f16(d), q clamped to +-127) — race-free
 * here. Same dispatch as qg_gemm_w4a8_f32 with M <-> N (tokens); the _ws form
 * takes a workspace of qg_gemm_w4a8_f32_workspace_size(N, K) bytes. */
int qg_gemm_q4_0_fp16_fused(const void* W, const void* act_f16, float* out, int M, int N, int K, qg_stream_t stream);
int qg_gemm_q4_0_fp16_fused_ws(const void* W, const void* act_f16, float* out, int M, int N, int K, void* workspace,
                               size_t workspace_bytes, qg_stream_t stream);
/* The fused kernel's FP16 -> Q8_1 quantizer on its own (k halves, multiple of 32). */
int qg_quantize_q8_1_f16_fused(const void* x_f16, void* y, int64_t k, qg_stream_t stream);

/* ---- quantizers (include/quantize.h:343-368; python/quant_gemm/csrc/gemm_ops.cu:146-202) ----
 * x: float[k] (k = total elements, multiple of 32), y: k/32 blocks of the named type.
 * Bytes are identical to the reference CPU quantizers (quantize_row_*_ref, round half away). */
int qg_quantize_q8_1(const float* x, void* y, int64_t k, qg_stream_t stream);
int qg_quantize_q4_0(const float* x, void* y, int64_t k, qg_stream_t stream);
/* Any type; variant 0 = include/quantize.h semantics, variant 1 (Q8_1 only) =
 * tests/framework/test_framework.cuh:195-225 (s = d * sum(q), q clamped to +-127), variant 2
 * (QG_QVAR_DEFINITION, Q8_1 and Q4_0) = the Solution definitions below. Q4_1/Q5_0/Q5_1
 * follow tests/framework/test_framework.cuh:256-367. */
enum { QG_QVAR_REFERENCE = 0, QG_QVAR_FRAMEWORK = 1, QG_QVAR_DEFINITION = 2 };
int qg_quantize(int type, int variant, const float* x, void* y, int64_t k, qg_stream_t stream);
/* The Solution entry points of the definitions quantize_q8_1 / quantize_q4_0
 * (schemas/definitions/quantization/quantize_q8_1.json:26-33,58 and quantize_q4_0.json:25-32,55: input
 * x[num_elements] f32, output y[num_elements/32] blocks, destination-passing), in definition order,
 * with the definitions' semantics where they differ from include/quantize.h: an all-zero block stores
 * d = 1.0 (not 0); q = round-half-to-EVEN(x / d) (torch.round of a true division, not roundf(x * (1/d)));
 * the stored f16 d is the correctly rounded f16 of amax / 127 (/ 7), the definition's Python float
 * converted once. Q8_1 s = the fp32 sum in element order (the definition's torch.sum order is
 * unspecified). Registered by integration/solutions/quantize_q{8_1,4_0}_hip_gfx950.json. */
int qg_quantize_q8_1_definition(const float* x, void* y, int64_t num_elements, qg_stream_t stream);
int qg_quantize_q4_0_definition(const float* x, void* y, int64_t num_elements, qg_stream_t stream);
/* Dequantize k elements (include/quantize.h:84-102 and the per-format formulas). */
int qg_dequantize(int type, const void* x, float* y, int64_t k, qg_stream_t stream);
int qg_dequantize_q4_0(const void* x, float* y, int64_t k, qg_stream_t stream);

/* ---- parity hook: per-block int32 dots sumi[M][N][K/32] (the reference's inner loop,
 * include/gemm_reference.h:202-212), computed by the SAME kernel instantiation qg_gemm_w4a8_ex
 * launches for this shape and algo (same unit loads, operand records / MFMA fragments and integer
 * dot instructions); only the per-block fp32 epilogue is replaced by a store of the int32 dot.
 * The fp32 terms themselves are checked against the oracle to its summation-order bound (the
 * MFMA-assisted prefill epilogue rounds its scale products differently from the reference). */
int qg_debug_sumi(const void* A_q8_1, const void* B, int32_t* sumi, int M, int N, int K, int wtype, int algo,
                  qg_stream_t stream);
/* The kernel instantiation (family + template parameters + grid) that qg_gemm_w4a8_ex (sumi = 0)
 * or qg_debug_sumi (sumi = 1) would launch for this shape on 256-B aligned buffers, as text;
 * nothing is launched. The parity tests assert the two are the same kernel. */
int qg_debug_config(int M, int N, int K, int wtype, int algo, int sumi, char* buf, size_t len);

/* ---- ggml-facing adapter (include/llama_adapter.h:49-76, declared but never defined there) ----
 * A minimal ggml_tensor view: ne[0] = K (contiguous), ne[1] = rows; nb[] byte strides.
 * activation: Q8_1 [K, M]; weights: Q4_0/Q4_1/Q5_0/Q5_1 [K, N]; output: F32 [N, M] (ggml
 * ne-order), i.e. row-major C[M][N]. kernel_type: NULL or any of the reference's names
 * ("naive", "tiled", "dp4a", "tiled_dp4a", "vectorized_dp4a") or "auto"/"gemv"/"mfma"/"generic". */
typedef struct {
    void* data;
    int type;       /* qg_type */
    int64_t ne[4];  /* elements per dim, ne[0] innermost */
    size_t nb[4];   /* byte stride per dim */
} qg_tensor_view;

int qg_gemm_w4a8_from_view(const qg_tensor_view* activation, const qg_tensor_view* weights, qg_tensor_view* output,
                           const char* kernel_type, qg_stream_t stream);
/* gemm_w4a16_from_ggml (llama_adapter.h:78-90): activation F32 [K, M], weights Q4_0 or Q8_0
 * [K, N], output F32 [N, M]; kernel_type NULL / "naive" / "tiled" / "auto". */
int qg_gemm_w4a16_from_view(const qg_tensor_view* activation, const qg_tensor_view* weights, qg_tensor_view* output,
                            const char* kernel_type, qg_stream_t stream);
/* gemm_fp32_from_ggml (llama_adapter.h:92-103): all three F32. */
int qg_gemm_fp32_from_view(const qg_tensor_view* activation, const qg_tensor_view* weights, qg_tensor_view* output,
                           const char* kernel_type, qg_stream_t stream);
/* ggml_mul_mat_id(as, b, ids) -> out on views, mapped onto qg_gemm_w4a8_moe:
 *   as:  weights, ne = [K, N, n_expert], dense rows and nb[2] = N * row bytes (the dense expert stride);
 *   b:   Q8_1, ne = [K, a_rows, T], dense; a_rows 1 or n_used (ggml's wider broadcast is not served);
 *   ids: I32 (QG_TYPE_I32), ne = [n_used, T], nb[0] = 4, nb[1] a multiple of 4 (a strided top-k view is fine);
 *   out: F32, ne = [N, n_used, T], nb[0] = 4, nb[1] a multiple of 4 and >= 4 N, nb[2] = n_used * nb[1].
 * A view the entry cannot express (other strides, ne[3] > 1) is QG_ERR_UNSUPPORTED; mismatched dims are
 * QG_ERR_INVALID_ARG. */
int qg_mul_mat_id_from_view(const qg_tensor_view* as, const qg_tensor_view* b, const qg_tensor_view* ids,
                            qg_tensor_view* out, qg_stream_t stream);
/* The same views and the same refusals, always through qg_gemm_w4a8_moe_prefill with the caller's workspace (of
 * qg_gemm_w4a8_moe_prefill_workspace_size(T, n_used, n_expert) bytes): the entry for a prompt. */
int qg_mul_mat_id_from_view_ws(const qg_tensor_view* as, const qg_tensor_view* b, const qg_tensor_view* ids,
                               qg_tensor_view* out, void* workspace, size_t workspace_bytes, qg_stream_t stream);
/* The same views and the same refusals, always through qg_gemm_w4a8_moe_batch with the caller's workspace (of
 * qg_gemm_w4a8_moe_batch_workspace_size(T, n_used, n_expert) bytes): the entry for batched decode. */
int qg_mul_mat_id_from_view_batch(const qg_tensor_view* as, const qg_tensor_view* b, const qg_tensor_view* ids,
                                  qg_tensor_view* out, void* workspace, size_t workspace_bytes, qg_stream_t stream);
/* The fused gate / up pair of an MoE FFN block on views, mapped onto qg_gemm_w4a8_moe_glu: out = glu_op(as_gate x b)
 * * (as_up x b), both ggml_mul_mat_id on the same b and ids. The views and the refusals of qg_mul_mat_id_from_view, and
 * two more, both QG_ERR_UNSUPPORTED: b with ne[1] != 1 (gate and up take the token's one row), as_up differing from
 * as_gate in type, ne or nb. */
int qg_mul_mat_id_glu_from_view(const qg_tensor_view* as_gate, const qg_tensor_view* as_up, const qg_tensor_view* b,
                                const qg_tensor_view* ids, qg_tensor_view* out, int glu_op, qg_stream_t stream);
/* The down product of an MoE FFN block with the weighted sum over the token's experts on views, mapped onto
 * qg_gemm_w4a8_moe_down: out[t] = sum_u weights[t, u] * (as[ids[t, u]] x b[t, u]).
 *   as, ids: as in qg_mul_mat_id_from_view; b: Q8_1, ne = [K, n_used, T], dense;
 *   weights: NULL (every weight 1), or F32 with ne = [n_used, T] or [1, n_used, T] (ggml's router weights), the n_used
 *            floats of a token dense, the token stride a multiple of 4 B;
 *   out: F32, ne = [N, T], nb[0] = 4, nb[1] a multiple of 4 and >= 4 N.
 * The refusals of qg_mul_mat_id_from_view, and QG_ERR_UNSUPPORTED for b with ne[1] != n_used, weights of another type
 * or with strides the entry cannot express, out with ne[2] > 1; weights with other dims are QG_ERR_INVALID_ARG. */
int qg_mul_mat_id_down_from_view(const qg_tensor_view* as, const qg_tensor_view* b, const qg_tensor_view* ids,
                                 const qg_tensor_view* weights, qg_tensor_view* out, qg_stream_t stream);
/* The two views entries above with the bias views of qg_gemm_w4a8_moe_glu_bias / qg_gemm_w4a8_moe_down_bias, for Q4_K /
 * Q6_K / MXFP4 experts. A bias view is NULL (no add) or F32 with ne = [N, n_expert], nb[0] = 4, nb[1] a multiple of 4
 * and >= 4 N (the bias stride; two bias views must have the same): another type or such strides QG_ERR_UNSUPPORTED,
 * other dims or null data QG_ERR_INVALID_ARG. Everything else as in the two entries above; an MXFP4 as->nb[2] off the
 * dense expert size N * K/32 * 17 is QG_ERR_UNSUPPORTED, as in qg_mul_mat_id_from_view. */
int qg_mul_mat_id_glu_bias_from_view(const qg_tensor_view* as_gate, const qg_tensor_view* as_up, const qg_tensor_view* bias_gate,
                                     const qg_tensor_view* bias_up, const qg_tensor_view* b, const qg_tensor_view* ids,
                                     qg_tensor_view* out, int glu_op, float alpha, float limit, qg_stream_t stream);
int qg_mul_mat_id_down_bias_from_view(const qg_tensor_view* as, const qg_tensor_view* bias, const qg_tensor_view* b,
                                      const qg_tensor_view* ids, const qg_tensor_view* weights, qg_tensor_view* out,
                                      qg_stream_t stream);
/* qg_mul_mat_id_from_view_ws / qg_mul_mat_id_from_view_batch with the bias view of qg_gemm_w4a8_moe_prefill_bias /
 * qg_gemm_w4a8_moe_batch_bias, for Q4_K / Q6_K / MXFP4 experts: bias NULL (no add) or F32 with ne = [N, n_expert],
 * nb[0] = 4, nb[1] a multiple of 4 and >= 4 N; its refusals as in the two entries above. */
int qg_mul_mat_id_bias_from_view_ws(const qg_tensor_view* as, const qg_tensor_view* bias, const qg_tensor_view* b,
                                    const qg_tensor_view* ids, qg_tensor_view* out, void* workspace, size_t workspace_bytes,
                                    qg_stream_t stream);
int qg_mul_mat_id_bias_from_view_batch(const qg_tensor_view* as, const qg_tensor_view* bias, const qg_tensor_view* b,
                                       const qg_tensor_view* ids, qg_tensor_view* out, void* workspace, size_t workspace_bytes,
                                       qg_stream_t stream);
/* validate_tensor_types (llama_adapter.h:110-117): 1 if all three types match, else 0. */
int qg_validate_view_types(const qg_tensor_view* activation, const qg_tensor_view* weights,
                           const qg_tensor_view* output, int expected_activation_type, int expected_weight_type,
                           int expected_output_type);

/* ---- FP32 GEMM C[M][N] = A[M][K] . B[N][K]^T: the unquantized baseline the NMSE is quoted against
 * (gemm_fp32_naive, include/gemm_cuda_naive.cuh:258-265; gemm_fp32_reference,
 * gemm_reference.h:38-58). Any K >= 0, 4-B aligned floats. */
int qg_gemm_fp32(const float* A, const float* B, float* C, int M, int N, int K, qg_stream_t stream);

/* ---- GGUF weight files -------------------------------------------------
 * A read-only mapping of a GGUF v2/v3 file: metadata and tensor directory; Q4_0/Q4_1/Q5_0/Q5_1/
 * Q8_0/Q8_1/F16/F32 tensor data are the same bytes the kernels take. Host-side only, except
 * qg_gguf_upload_tensor (a stream-ordered copy, then a stream sync). Every length and offset is
 * checked against the file size; an unreadable or inconsistent file is QG_ERR_INVALID_ARG.
 * Tensor dims follow ggml: ne[0] = K (contiguous), ne[1] = rows; unused dims are 1. */
typedef struct qg_gguf qg_gguf;
int qg_gguf_open(const char* path, qg_gguf** out);
void qg_gguf_close(qg_gguf* file);
int qg_gguf_version(const qg_gguf* file);
int64_t qg_gguf_alignment(const qg_gguf* file);
int64_t qg_gguf_tensor_count(const qg_gguf* file);
int64_t qg_gguf_find_tensor(const qg_gguf* file, const char* name);   /* -1 if absent */
int qg_gguf_tensor_info(const qg_gguf* file, int64_t index, const char** name, int* type, int* n_dims,
                        int64_t ne[4], uint64_t* nbytes);               /* nbytes 0: type not supported */
const void* qg_gguf_tensor_data(const qg_gguf* file, int64_t index);   /* host pointer into the mapping */
int qg_gguf_upload_tensor(const qg_gguf* file, int64_t index, void* device_dst, size_t dst_bytes,
                          qg_stream_t stream);
/* a ggml-ordered view of the tensor's bytes at device_data, for the *_from_view entry points */
int qg_gguf_tensor_view(const qg_gguf* file, int64_t index, void* device_data, qg_tensor_view* out);
int64_t qg_gguf_kv_count(const qg_gguf* file);
int64_t qg_gguf_find_kv(const qg_gguf* file, const char* key);         /* -1 if absent */
/* GGUF value types: 0 u8, 1 i8, 2 u16, 3 i16, 4 u32, 5 i32, 6 f32, 7 bool, 8 string, 9 array,
 * 10 u64, 11 i64, 12 f64 (arrays: element type and count) */
int qg_gguf_kv_info(const qg_gguf* file, int64_t index, const char** key, int* type, uint64_t* array_count,
                    int* array_type);
int qg_gguf_kv_int(const qg_gguf* file, int64_t index, int64_t* value);
int qg_gguf_kv_float(const qg_gguf* file, int64_t index, double* value);
int qg_gguf_kv_string(const qg_gguf* file, int64_t index, const char** str, uint64_t* len);  /* not NUL-terminated */

/* ---- introspection ---- */
const char* qg_status_string(int status);
/* The capture-time GEMV merge (see qg_gemm_w4a8): 0 off, 1 on (the default; the environment variable
 * QG_CAPTURE_FUSE=0, read once, makes off the default), 2 on for every shape class, measured or not (A/B
 * runs). Process-wide; affects calls made after it. */
void qg_set_capture_fusion(int on);
/* Process-wide counters since load: captured GEMV calls merged into an existing node, and GEMV kernel
 * nodes those calls started (calls eligible for the merge only). Either pointer may be NULL. */
void qg_capture_fusion_stats(uint64_t* merged, uint64_t* nodes);
int qg_last_hip_error(void);                    /* hipError_t of the last QG_ERR_HIP on this thread */
int qg_select_algo(int M, int N, int K, int wtype); /* what QG_ALGO_AUTO dispatches to */
int qg_block_bytes(int type);                   /* 18/20/22/24/34/36, 144 for Q4_K, 210 for Q6_K, 17 for MXFP4, 0 if unknown */
int qg_block_elems(int type);                   /* 32 for the block types, 256 for Q4_K / Q6_K, 0 if unknown */
const char* qg_version(void);

#ifdef __cplusplus
}
#endif

#endif /* QG_QG_H */
