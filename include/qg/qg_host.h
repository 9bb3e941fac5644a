/*
 * qg/qg_host.h — host-only C-ABI twins of the reference's CPU entry points (`libqg_host.so`).
 *
 * SURVEY.md §8(b) "CPU API": the reference's ground-truth functions are inline host functions in
 * include/gemm_reference.h and include/quantize.h. A caller that links them today can link these
 * instead: same argument order, pointer types (as void*), layouts and results — bit-identical
 * outputs on x86-64 (IEEE fp32, no FMA contraction, the reference's operation order). This
 * library is independent of the GPU library (no HIP) and of the test oracle (oracle/), which
 * checks it.
 *
 * Differences, deliberate: the GEMMs return a status (0, or QG_ERR_BAD_K / QG_ERR_INVALID_ARG from
 * qg/qg.h) instead of void, since the reference never validates K % 32 (gemm_reference.h:181);
 * `_mt` forms partition output rows over threads (each output keeps the serial summation order,
 * so results are identical for any thread count).
 */
#ifndef QG_QG_HOST_H
#define QG_QG_HOST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* gemm_w4a8_reference(const block_q8_1* A, const block_q4_0* B, float* C, int M, int N, int K)
 * (include/gemm_reference.h:175-222): C[M][N] overwritten. */
int qg_gemm_w4a8_q4_0_cpu(const void* A_q8_1, const void* B_q4_0, float* C, int M, int N, int K);

/* vec_dot_q4_0_q8_1(int n, float* s, const void* vx, const void* vy)
 * (include/gemm_reference.h:276-306): *s = the dot of n elements, vx Q4_0, vy Q8_1. */
void qg_vec_dot_q4_0_q8_1_cpu(int n, float* s, const void* vx, const void* vy);

/* vec_dot_q8_0_q8_1 (include/gemm_reference.h:311-335) */
void qg_vec_dot_q8_0_q8_1_cpu(int n, float* s, const void* vx, const void* vy);

/* gemm_w8a8_reference (include/gemm_reference.h:233-267): Q8_0 weights. */
int qg_gemm_w8a8_cpu(const void* A_q8_1, const void* B_q8_0, float* C, int M, int N, int K);

/* Every weight format of qg_gemm_w4a8 (qg_type ids Q4_0/Q4_1/Q5_0/Q5_1/Q8_0), the same
 * per-block formulas as the GPU library (qg_common.hpp header), rows over `threads` threads
 * (<= 0: one). Also QG_TYPE_Q4_K (K % 256 == 0, else QG_ERR_BAD_K): the Q4_K product contract of qg.h,
 * one dot and one min accumulator per super-block in sub-block order, super-blocks summed in order.
 * And QG_TYPE_Q6_K (K % 256 == 0, else QG_ERR_BAD_K): the Q6_K product contract of qg.h, isum in int32, one
 * fp32 accumulator per super-block in block order, d applied once, super-blocks summed in order.
 * And QG_TYPE_MXFP4 (K % 32 == 0): the MXFP4 product contract of qg.h, sumi in int32, (d_a * scale(e)) * float(sumi)
 * per block, one fp32 accumulator per output, blocks in order (W = 0). Bits are
 * identical for every thread count (threads split the weight rows only). */
int qg_gemm_w4a8_cpu_mt(const void* A_q8_1, const void* B, float* C, int M, int N, int K, int wtype, int threads);

/* Host twin of qg_gemm_w4a8_moe (qg.h): the same arguments with `ids` in host memory, and `threads` as above.
 * Slot s = t * n_used + u takes expert e = ids[t * ids_stride + u]; its N outputs at C + s * ldc (0 = N) are
 * bit-identical to qg_gemm_w4a8_cpu_mt on (A row t * a_rows + u % a_rows, expert e) with M = 1, for every thread
 * count; an id outside [0, n_expert) gives N times +0.0f. The same validation codes; no shape is unsupported. */
int qg_gemm_w4a8_moe_cpu(const void* A_q8_1, int a_rows, const void* B_experts, int n_expert, const int32_t* ids,
                         int64_t ids_stride, float* C, int64_t ldc, int T, int n_used, int N, int K, int wtype,
                         int threads);

/* Host twin of qg_gemm_w4a8_moe_glu (qg.h): the same arguments with `ids` in host memory, and `threads` as above.
 * g and u of a slot have the bits of qg_gemm_w4a8_moe_cpu on B_gate and on B_up (a_rows = 1); the op is the same two
 * formulas, one rounded fp32 operation each, with libm's expf: QG_GLU_REGLU (g > 0 ? g : 0.0f) * u, QG_GLU_SWIGLU
 * (g / (1.0f + expf(-g))) * u. An id outside [0, n_expert) gives N times +0.0f. The same validation codes (wtype other
 * than Q4_K / Q6_K and a glu_op other than these two are QG_ERR_UNSUPPORTED; no alignment is asked); no shape is
 * unsupported. */
int qg_gemm_w4a8_moe_glu_cpu(const void* A_q8_1, const void* B_gate, const void* B_up, int n_expert, const int32_t* ids,
                             int64_t ids_stride, float* C, int64_t ldc, int T, int n_used, int N, int K, int wtype,
                             int glu_op, int threads);

/* Host twin of qg_gemm_w4a8_moe_down (qg.h): the same arguments with `ids` and `weights` in host memory, and `threads`
 * as above. d_u has the bits of qg_gemm_w4a8_moe_cpu at a_rows = n_used; the fold is the same: acc = +0.0f, then
 * acc = acc + weights[t * w_stride + u] * d_u in ascending u, one rounded fp32 operation each, an id outside
 * [0, n_expert) left out with its weight unread; weights == NULL is every weight 1.0f. C is [T][ldc], one row per
 * token. The same validation codes (wtype other than Q4_K / Q6_K is QG_ERR_UNSUPPORTED; no alignment is asked); no
 * shape is unsupported. */
int qg_gemm_w4a8_moe_down_cpu(const void* A_q8_1, const void* B_experts, int n_expert, const int32_t* ids,
                              int64_t ids_stride, const float* weights, int64_t w_stride, float* C, int64_t ldc, int T,
                              int n_used, int N, int K, int wtype, int threads);

/* Host twin of qg_gemm_w4a8_moe_prefill_bias / qg_gemm_w4a8_moe_batch_bias (qg.h), beside qg_gemm_w4a8_moe_cpu: the same
 * arguments without the workspace, `ids` and `bias` in host memory, `threads` as above; wtype Q4_K, Q6_K or MXFP4. Every
 * product has the bits of qg_gemm_w4a8_moe_cpu; where bias is non-null, bias[e][n] is then added with one rounded fp32
 * addition. An id outside [0, n_expert) gives N times +0.0f, its bias not read. The same validation codes (no alignment is
 * asked); no shape is unsupported. */
int qg_gemm_w4a8_moe_bias_cpu(const void* A_q8_1, int a_rows, const void* B_experts, const float* bias, int64_t bias_stride,
                              int n_expert, const int32_t* ids, int64_t ids_stride, float* C, int64_t ldc, int T, int n_used,
                              int N, int K, int wtype, int threads);

/* Host twins of qg_gemm_w4a8_moe_glu_bias / qg_gemm_w4a8_moe_down_bias (qg.h): the same arguments with `ids`, `weights`
 * and the biases in host memory, and `threads` as above; wtype Q4_K, Q6_K or MXFP4. The products have the bits of
 * qg_gemm_w4a8_moe_cpu; a non-null bias is added with one rounded fp32 addition (g + bias_gate[e][n], u + bias_up[e][n],
 * d_u + bias[e_u][n]) ahead of the op or the fold, which are those of the two twins above, and for QG_GLU_SWIGLU_OAI
 *   x = fminf(g, limit); y = fminf(fmaxf(u, -limit), limit); (x / (1.0f + expf(alpha * (-x)))) * (y + 1.0f)
 * with libm's expf. An id outside [0, n_expert) gives N times +0.0f (GLU) or contributes nothing (down); its bias is
 * not read. The same validation codes (no alignment is asked); no shape is unsupported. */
int qg_gemm_w4a8_moe_glu_bias_cpu(const void* A_q8_1, const void* B_gate, const void* B_up, const float* bias_gate,
                                  const float* bias_up, int64_t bias_stride, int n_expert, const int32_t* ids,
                                  int64_t ids_stride, float* C, int64_t ldc, int T, int n_used, int N, int K, int wtype,
                                  int glu_op, float alpha, float limit, int threads);
int qg_gemm_w4a8_moe_down_bias_cpu(const void* A_q8_1, const void* B_experts, const float* bias, int64_t bias_stride,
                                   int n_expert, const int32_t* ids, int64_t ids_stride, const float* weights,
                                   int64_t w_stride, float* C, int64_t ldc, int T, int n_used, int N, int K, int wtype,
                                   int threads);

/* gemm_fp32_reference (include/gemm_reference.h:38-58): float accumulation in k order. */
int qg_gemm_fp32_cpu(const float* A, const float* B, float* C, int M, int N, int K);

/* Host twin of qg_dequantize for QG_TYPE_MXFP4: k elements (a multiple of 32, else QG_ERR_BAD_K) of block_mxfp4 ->
 * y[i] = float(kv[code]) * scale(e), exact for every (code, e), +0.0f for code 8 (qg.h, "MXFP4 weights"). */
int qg_dequantize_row_mxfp4_cpu(const void* x, float* y, int64_t k);

/* quantize_row_q8_1_ref / quantize_row_q4_0_ref (include/quantize.h:165-193, 35-70). */
int qg_quantize_row_q8_1_cpu(const float* x, void* y, int64_t k);
int qg_quantize_row_q4_0_cpu(const float* x, void* y, int64_t k);

/* The measurement recipe of SURVEY.md §8(d) (tests/step4_w4a8_gemm.cu:142-148): glibc
 * srand(seed), then A[M][K] and B[N][K] drawn as 2*rand()/RAND_MAX - 1, A first. Writes A (if a
 * is not NULL) and rows [row0, row1) of B (if b is not NULL; a rank's shard), advancing the
 * generator over the rows it skips. Uses the process-wide libc generator. */
int qg_fill_step4_cpu(unsigned seed, int M, int N, int K, int row0, int row1, float* a, float* b);

#ifdef __cplusplus
}
#endif

#endif /* QG_QG_HOST_H */
