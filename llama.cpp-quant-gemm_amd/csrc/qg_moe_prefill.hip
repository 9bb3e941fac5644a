// qg_moe_prefill.hip — the expert-grouped MFMA prefill (qg_gemm_w4a8_moe_prefill, ggml's mul_mat_id at prompt
// sizes), families "moe:q4k_mmq" and "moe:q6k_mmq". DESIGN.md 3d. And its biased twin qg_gemm_w4a8_moe_prefill_bias with
// MXFP4 experts beside them, family "moe:mxfp4_mmq" (DESIGN.md 3j): kernels of its own further down, these untouched.
//
// Two launches on the caller's stream, no allocation, no synchronisation, the host never reads ids:
//  1. moe_plan_kernel (qg_moe_plan.hip) with tiles of R = 16 TT rows: the T * n_used slots counting-sorted by expert id
//     into the caller's workspace (qg_moe_plan.hpp, MoePlanLayout), one record {bin, first sorted position, rows} per
//     tile with their number n_tiles.
//  2. q4k_moe_mmq_kernel / q6k_moe_mmq_kernel<TT, RG>: the K loops of q4k_mmq_kernel / q6k_mmq_kernel (qg_q4k_mmq.hip,
//     qg_q6k_mmq.hip: the work decomposition is described there), the same text included (qg_q4k_mmq_body.inc,
//     qg_q6k_mmq_body.inc; text and not a function, so that the shipped code objects do not move: DESIGN.md 3c), between
//     a prologue and a reduction of their own. What differs:
//       * blockIdx.y is a tile index. The workgroup reads n_tiles and its record (uniform) and returns at once
//         beyond n_tiles: gridDim.y is the host's upper bound moe_max_tiles.
//       * the activation row of tile position p is rows[first + min(p, rows - 1)]: positions past the tile's rows
//         are loaded and multiplied, never stored (the shipped kernels' rule at M - 1). Each lane loads the row
//         indices it needs once, before the K loop; a token load takes its (wave-uniform) index with v_readlane.
//       * the expert's matrix is B + e * estride, formed in 64 bits before any weight address.
//       * the output row of position p is C + sorted[first + p] * ldc.
//       * a tile of the invalid bin stores +0.0f to its rows and returns before any weight address is formed.
//     Staging, the one barrier per step, the Q6_K realigned loads, the clamps at N - 1 and the K-slice reduction
//     through LDS in slice order are the shipped kernels'; every workgroup that passes the tile lookup runs the same
//     number of barriers. An output's arithmetic depends on its activation row, its weight row and KS alone, so its
//     bits do not depend on TT, on the tile or on the position the sort gave its slot.
#include "../../include/qg/qg.h"
#include "qg_kq_launch.hpp"
#include "qg_moe_prefill.hpp"
#include "qg_q4k.hpp"
#include "qg_q6k.hpp"

namespace qg {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

// (TT, RG) of the product (0: by shape, moe_prefill_form; A/B builds force 1 = (1,1), 2 = (2,1), 3 = (4,1), 4 = (4,4))
#ifndef QG_MOE_PREFILL_FORM
#define QG_MOE_PREFILL_FORM 0
#endif

// ---- what the two gathered kernels share --------------------------------------------------------------------------
constexpr int MMQ_WAVES = 8;
constexpr int MMQ_WGS = 64 * MMQ_WAVES;
constexpr int TOK_DW = Q4K_TOK_DW;  // one token's 8 blocks of a super-block: the gathered loads serve both types
static_assert(Q6K_TOK_DW == TOK_DW, "one activation staging layout");

// The activation rows this lane needs, loaded once: rowv[t] that of position 16 t + (lane & 15) (a token load reads
// position p's from lane p & 15), tailv[t][b] that of the lane's tail load b. Positions past the tile's rows take
// the last valid row.
template <int TT, int RG> struct MoeRows {
    static constexpr int NT = RG == 1 ? 2 : 1;
    int rowv[TT], tailv[TT][NT];
    __device__ __forceinline__ void load(const MoeTile& tl, int lane, int rg) {
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            rowv[t] = tl.arows[min(16 * t + (lane & 15), tl.rows - 1)];
#pragma unroll
            for (int b = 0; b < NT; ++b)
                tailv[t][b] = tl.arows[min(16 * t + 8 * (RG == 1 ? b : rg) + (lane >> 3), tl.rows - 1)];
        }
    }
};

// this wave's share of a 16-token tile of super-block sb: token loads r take dwords 0..63 of token NR rg + r (the
// token's row is wave-uniform, so its address lives in SGPRs), a tail load dwords 64..71 of 8 tokens
template <int TT, int RG>
__device__ __forceinline__ void moe_load_tile(uint32_t (&dst)[16 / RG + (RG == 1 ? 2 : 1)], const uint32_t* A, long arow,
                                              const MoeRows<TT, RG>& rows, int sb, int t, int lane, int rg) {
    constexpr int NR = 16 / RG, NT = RG == 1 ? 2 : 1;
    const uint32_t* a = A + (long)sb * TOK_DW;
#pragma unroll
    for (int r = 0; r < NR; ++r) dst[r] = a[(long)__builtin_amdgcn_readlane(rows.rowv[t], NR * rg + r) * arow + lane];
    if (RG == 1 || rg < 2) {
#pragma unroll
        for (int b = 0; b < NT; ++b) dst[NR + b] = a[(long)rows.tailv[t][b] * arow + 64 + (lane & 7)];
    }
}
template <int RG>
__device__ __forceinline__ void moe_store_tile(const uint32_t (&src)[16 / RG + (RG == 1 ? 2 : 1)], uint32_t* buf, int lane,
                                               int rg) {
    constexpr int NR = 16 / RG, NT = RG == 1 ? 2 : 1;
#pragma unroll
    for (int r = 0; r < NR; ++r) buf[(NR * rg + r) * TOK_DW + lane] = src[r];
    if (RG == 1 || rg < 2) {
#pragma unroll
        for (int b = 0; b < NT; ++b) buf[(8 * (RG == 1 ? b : rg) + (lane >> 3)) * TOK_DW + 64 + (lane & 7)] = src[NR + b];
    }
}

// A tile of the invalid bin: +0.0f to this workgroup's 16 RG rows of the tile's slots.
template <int TT, int RG> __device__ __forceinline__ void moe_zero_tile(const MoePlanArgs& a, const MoeTile& tl, int tile) {
    constexpr int PT = TT * 256;
    for (int idx = threadIdx.x; idx < RG * PT; idx += MMQ_WGS) {
        const int g = idx / PT, o = idx - g * PT;
        const int p = o >> 4, n = tile * (16 * RG) + 16 * g + (o & 15);
        if (p < tl.rows && n < a.N) a.C[(long)tl.sorted[p] * a.ldc + n] = 0.0f;
    }
}

// The K-slice reduction: partial tiles as [slice][row group][token][row] (over the staging buffers, once every wave
// has read its last tile), lane (c, q) writes rows 4q .. 4q + 3 of token c (one 16-B store); then each output is the
// sum of its KS partials in slice order, stored to its slot's row.
template <int TT, int RG>
__device__ __forceinline__ void moe_reduce_store(const MoePlanArgs& a, const MoeTile& tl, uint32_t* smem,
                                                 const float (&acc)[TT][4], int ks, int rg, int r16, int q, int tile) {
    constexpr int KS = MMQ_WAVES / RG, PT = TT * 256;  // outputs per (slice, row group)
    __syncthreads();
    float* part = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int t = 0; t < TT; ++t)
        *reinterpret_cast<float4*>(&part[(ks * RG + rg) * PT + (16 * t + r16) * 16 + 4 * q]) =
            make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
    __syncthreads();
    for (int idx = threadIdx.x; idx < RG * PT; idx += MMQ_WGS) {
        float sum = part[idx];
#pragma unroll
        for (int k = 1; k < KS; ++k) sum += part[k * (RG * PT) + idx];
        const int g = idx / PT, o = idx - g * PT;
        const int p = o >> 4, n = tile * (16 * RG) + 16 * g + (o & 15);
        if (p < tl.rows && n < a.N) a.C[(long)tl.sorted[p] * a.ldc + n] = sum;
    }
}

// ---- Q4_K: q4k_mmq_kernel (qg_q4k_mmq.hip) on a tile of gathered rows ----------------------------------------------
template <int TT, int RG> __global__ __launch_bounds__(MMQ_WGS) void q4k_moe_mmq_kernel(const MoePlanArgs a) {
    static_assert(RG == 1 || RG == 4, "row groups per workgroup");
    constexpr int W = MMQ_WAVES, KS = W / RG;
    constexpr int NBUF = RG > 1 ? 2 : 1;
    constexpr int NR = 16 / RG;          // token loads (dwords 0..63 of a token) per wave and tile
    constexpr int NT = RG == 1 ? 2 : 1;  // tail loads (dwords 64..71 of 8 tokens) per wave (RG = 4: waves 0, 1)
    constexpr int STAGE_DW = KS * NBUF * Q4K_TILE_DW, PART_DW = W * TT * 256;
    __shared__ __attribute__((aligned(16))) uint32_t smem[STAGE_DW > PART_DW ? STAGE_DW : PART_DW];
    MoeTile mt;
    if (!moe_tile_lookup(a, mt)) return;
    const int N = a.N, nb = a.K / QK, nsb = a.K / SB_ELEMS;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int rg = wave % RG, ks = wave / RG;
    const int r16 = lane & 15, q = lane >> 4;
    // xcd_tile_x() (qg_common.hpp), written out: through the function these kernels' code objects move
    const int tile = gridDim.x <= 512 ? xcd_tile(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    if (mt.e >= a.n_expert) {
        moe_zero_tile<TT, RG>(a, mt, tile);
        return;
    }
    const int n0 = tile * (16 * RG) + 16 * rg;
    const long wrow = (long)nsb * Q4K_BYTES;
    const long arow = (long)nb * 9;  // dwords per activation row
    const uint32_t* A = static_cast<const uint32_t*>(a.A);
    const uint8_t* B = static_cast<const uint8_t*>(a.B) + (long)mt.e * a.estride;
    // rows past the end are clamped to the last one: loaded and multiplied, never stored
    const uint8_t* wq = B + (long)min(n0 + r16, N - 1) * wrow + 16 + 8 * q;
    const uint8_t* wh[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) wh[e] = B + (long)min(n0 + 4 * q + e, N - 1) * wrow;
    uint32_t* stage = smem + ks * (NBUF * Q4K_TILE_DW);
    MoeRows<TT, RG> rows;
    rows.load(mt, lane, rg);
    // the gathered loads under the names the K loop uses; its SUMI branch is discarded here, its names resolve to these
    auto load_tile = [&](uint32_t (&dst)[NR + NT], int sb, int t) {
        moe_load_tile<TT, RG>(dst, A, arow, rows, sb, t, lane, rg);
    };
    auto store_tile = [&](const uint32_t (&src)[NR + NT], uint32_t* buf) { moe_store_tile<RG>(src, buf, lane, rg); };
    constexpr bool SUMI = false;
    constexpr int m0 = 0, M = 0;
    constexpr void* out = nullptr;
#include "qg_q4k_mmq_body.inc"
    moe_reduce_store<TT, RG>(a, mt, smem, acc, ks, rg, r16, q, tile);
}

// ---- Q6_K: q6k_mmq_kernel (qg_q6k_mmq.hip) on a tile of gathered rows ----------------------------------------------
template <int TT, int RG> __global__ __launch_bounds__(MMQ_WGS) void q6k_moe_mmq_kernel(const MoePlanArgs a) {
    static_assert(RG == 1 || RG == 4, "row groups per workgroup");
    constexpr int W = MMQ_WAVES, KS = W / RG;
    constexpr int NBUF = RG > 1 ? 2 : 1;
    constexpr int NR = 16 / RG;
    constexpr int NT = RG == 1 ? 2 : 1;
    constexpr int STAGE_DW = KS * NBUF * Q6K_TILE_DW, PART_DW = W * TT * 256;
    __shared__ __attribute__((aligned(16))) uint32_t smem[STAGE_DW > PART_DW ? STAGE_DW : PART_DW];
    MoeTile mt;
    if (!moe_tile_lookup(a, mt)) return;
    const int N = a.N, nb = a.K / QK, nsb = a.K / SB_ELEMS;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int rg = wave % RG, ks = wave / RG;
    const int r16 = lane & 15, q = lane >> 4;
    // xcd_tile_x() (qg_common.hpp), written out: through the function these kernels' code objects move
    const int tile = gridDim.x <= 512 ? xcd_tile(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    if (mt.e >= a.n_expert) {
        moe_zero_tile<TT, RG>(a, mt, tile);
        return;
    }
    const int n0 = tile * (16 * RG) + 16 * rg;
    const long wrow = (long)nsb * Q6K_BYTES;
    const long arow = (long)nb * 9;  // dwords per activation row
    const uint32_t* A = static_cast<const uint32_t*>(a.A);
    const uint8_t* B = static_cast<const uint8_t*>(a.B) + (long)mt.e * a.estride;
    // rows past the end are clamped to the last one: loaded and multiplied, never stored
    const uint8_t* wq = B + (long)min(n0 + r16, N - 1) * wrow;  // the operand row of MFMA lane (r16, q)
    const uint8_t* wh[4];                                       // the result lane's rows 4q .. 4q + 3
#pragma unroll
    for (int e = 0; e < 4; ++e) wh[e] = B + (long)min(n0 + 4 * q + e, N - 1) * wrow;
    uint32_t* stage = smem + ks * (NBUF * Q6K_TILE_DW);
    MoeRows<TT, RG> rows;
    rows.load(mt, lane, rg);
    // the gathered loads under the names the K loop uses; its SUMI branch is discarded here, its names resolve to these
    auto load_tile = [&](uint32_t (&dst)[NR + NT], int sb, int t) {
        moe_load_tile<TT, RG>(dst, A, arow, rows, sb, t, lane, rg);
    };
    auto store_tile = [&](const uint32_t (&src)[NR + NT], uint32_t* buf) { moe_store_tile<RG>(src, buf, lane, rg); };
    constexpr bool SUMI = false;
    constexpr int m0 = 0, M = 0;
    constexpr void* out = nullptr;
#include "qg_q6k_mmq_body.inc"
    moe_reduce_store<TT, RG>(a, mt, smem, acc, ks, rg, r16, q, tile);
}

// ---- the biased entry (qg_gemm_w4a8_moe_prefill_bias): kernels beside the two above, which stay --------
// The last loop of moe_reduce_store with the bias: part holds [slice][row group][token][row]; each output is the sum of
// its KS partials in slice order, then one rounded addition of the expert's bias (BIAS = false: no load, no test).
template <int TT, int RG, bool BIAS>
__device__ __forceinline__ void moe_sum_bias_store(const MoeBiasArgs& a, const MoeTile& tl, const float* part, int tile) {
    constexpr int KS = MMQ_WAVES / RG, PT = TT * 256;
    const float* bias = BIAS ? a.bias + (long)tl.e * a.bias_stride : nullptr;
    for (int idx = threadIdx.x; idx < RG * PT; idx += MMQ_WGS) {
        float sum = part[idx];
#pragma unroll
        for (int k = 1; k < KS; ++k) sum += part[k * (RG * PT) + idx];
        const int g = idx / PT, o = idx - g * PT;
        const int p = o >> 4, n = tile * (16 * RG) + 16 * g + (o & 15);
        if (p < tl.rows && n < a.N) {
            if constexpr (BIAS) sum = sum + bias[n];
            a.C[(long)tl.sorted[p] * a.ldc + n] = sum;
        }
    }
}

// Q4_K / Q6_K with a bias: the two kernels above as they are, then this one on the finished product (ggml's add_id):
// slot s = blockIdx.y adds its expert's bias row; a slot whose id names no expert keeps its +0.0f, no bias is read.
// A launch of its own and not a BIAS form of those kernels: their bodies stay included once per file, their code
// objects the shipped ones. qg_gemm_w4a8_moe_batch_bias runs it too (launch_moe_bias_add).
__global__ __launch_bounds__(256) void moe_bias_add_kernel(const MoeBiasArgs a) {
    const int s = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    const int t = s / a.n_used, u = s - t * a.n_used;
    const int e = a.ids[(long)t * a.ids_stride + u];
    if ((unsigned)e >= (unsigned)a.n_expert || n >= a.N) return;
    float* c = a.C + (long)s * a.ldc + n;
    *c = *c + a.bias[(long)e * a.bias_stride + n];
}

// MXFP4: mxfp4_mmq_kernel (qg_mxfp4_mmq.hip) on a tile of gathered rows, "moe:mxfp4_mmq". What differs from the two
// K-quant kernels above:
//   * a row is K / 32 blocks in groups of 8, the last group of 1 .. 8: the gathered loads clamp the dword index to the
//     row's last dword as mxfp4_mmq_kernel's do (moe_load_tile has no clamp: K-quant rows are whole super-blocks), so
//     nothing is read past a gathered row's end; the weight side is the body's own clamp.
//   * the body leaves lane (r16, q) with weight row r16 x tokens 4q .. 4q + 3, the transpose of the K-quant bodies: the
//     partials go to part[..][token 16t + 4q + e][row r16], after which the layout is the one moe_sum_bias_store reads.
//   * the expert's matrix starts at any byte: B + e * estride in 64 bits, the body realigns per block.
template <int TT, int RG, bool BIAS> __global__ __launch_bounds__(MMQ_WGS) void mxfp4_moe_mmq_kernel(const MoeBiasArgs a) {
    static_assert(RG == 1 || RG == 4, "row groups per workgroup");
    static_assert(MXFP4_TOK_DW == TOK_DW, "one activation staging layout");
    constexpr int W = MMQ_WAVES, KS = W / RG;
    constexpr int NBUF = RG > 1 ? 2 : 1;
    constexpr int NR = 16 / RG;
    constexpr int NT = RG == 1 ? 2 : 1;
    constexpr int STAGE_DW = KS * NBUF * MXFP4_TILE_DW, PART_DW = W * TT * 256, PT = TT * 256;
    __shared__ __attribute__((aligned(16))) uint32_t smem[STAGE_DW > PART_DW ? STAGE_DW : PART_DW];
    MoeTile mt;
    if (!moe_tile_lookup(a, mt)) return;
    const int N = a.N, nb = a.K / QK, ngrp = (nb + 7) / 8;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int rg = wave % RG, ks = wave / RG;
    const int r16 = lane & 15, q = lane >> 4;
    const int tile = xcd_tile_x();
    if (mt.e >= a.n_expert) {
        moe_zero_tile<TT, RG>(a, mt, tile);
        return;
    }
    const int n0 = tile * (16 * RG) + 16 * rg;
    const int arow = nb * 9;  // dwords per activation row
    const uint32_t* A = static_cast<const uint32_t*>(a.A);
    const uint8_t* B = static_cast<const uint8_t*>(a.B) + (long)mt.e * a.estride;
    // rows past the end are clamped to the last one: loaded and multiplied, never stored
    const uint8_t* wq = B + (long)min(n0 + r16, N - 1) * ((long)nb * MXFP4_BYTES);  // the row of MFMA lane (r16, q)
    uint32_t* stage = smem + ks * (NBUF * MXFP4_TILE_DW);
    MoeRows<TT, RG> rows;
    rows.load(mt, lane, rg);
    // moe_load_tile by groups of 8 blocks, the dword index clamped to the row's last dword (a partial last group)
    auto load_tile = [&](uint32_t (&dst)[NR + NT], int g, int t) {
        const int c0 = g * MXFP4_TOK_DW;
#pragma unroll
        for (int r = 0; r < NR; ++r)
            dst[r] = A[(long)__builtin_amdgcn_readlane(rows.rowv[t], NR * rg + r) * arow + min(c0 + lane, arow - 1)];
        if (RG == 1 || rg < 2) {
#pragma unroll
            for (int b = 0; b < NT; ++b) dst[NR + b] = A[(long)rows.tailv[t][b] * arow + min(c0 + 64 + (lane & 7), arow - 1)];
        }
    };
    auto store_tile = [&](const uint32_t (&src)[NR + NT], uint32_t* buf) { moe_store_tile<RG>(src, buf, lane, rg); };
    constexpr bool SUMI = false;
    constexpr int m0 = 0, M = 0;
    constexpr void* out = nullptr;
#include "qg_mxfp4_mmq_body.inc"
    // partial tiles as [slice][row group][token][row] (over the staging buffers, once every wave has read its last
    // tile): lane (r, q) writes row r of tokens 4q .. 4q + 3
    __syncthreads();
    float* part = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int t = 0; t < TT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) part[(ks * RG + rg) * PT + (16 * t + 4 * q + e) * 16 + r16] = acc[t][e];
    __syncthreads();
    moe_sum_bias_store<TT, RG, BIAS>(a, mt, part, tile);
}

// ---- host side ------------------------------------------------------------------------------------------------------
// (TT, RG) from (T, n_used, n_expert, N, K, the type, CU count) alone: the shipped prefill's rule (kq_mmq_launch_t)
// with the expected rows per expert, slots / n_expert, in the place of M for the tile's rows, and all the slots in
// the place of M for the 64 x 64 tiles' grid. One rule of its own: Q6_K at K <= 1024 takes the 64 x 64 tiles at any
// T -- with K / 256 <= 4 super-blocks at least half of the KS = 8 forms' waves idle, and its heavier body pays for
// that. profiles/moe_prefill/ab_moe_prefill_forms.txt, us per call, Qwen3-MoE down (N = 2048, K = 768, 128 experts,
// 8 used), (1, 1) -> (4, 4): Q6_K T = 16 169.5 -> 157.1, T = 64 255.0 -> 224.8, T = 256 362.9 -> 230.5; Q4_K
// T = 16 84.8 -> 137.1, T = 64 126.8 -> 196.7, T = 256 181.9 -> 202.6 (so Q4_K keeps the rule). Only K = 768 is
// measured below K = 2048, where (1, 1) wins for both types up to T = 256. The other thresholds: DESIGN.md 3d.
struct MoeForm {
    int tt, rg;
};
MoeForm moe_prefill_form(const MoePlanArgs& a, int wtype) {
    constexpr MoeForm forms[] = {{1, 1}, {2, 1}, {4, 1}, {4, 4}};
    if (QG_MOE_PREFILL_FORM) return forms[QG_MOE_PREFILL_FORM - 1];
    if (wtype == QG_TYPE_Q6_K && a.K <= 4 * SB_ELEMS) return forms[3];
    const long per = (a.slots + a.n_expert - 1) / a.n_expert;
    if (per <= 16) return forms[0];
    if (per <= 32) return forms[1];
    if ((long)((a.N + 63) / 64) * ((a.slots + 63) / 64) >= device_cus()) return forms[3];
    return forms[2];
}

using Launch = MoeLaunch<MoePlanArgs>;

template <int WT, int TT, int RG> hipError_t moe_prefill_k(const Launch& L) {
    const MoePlanArgs& a = L.a;
    const int gx = (a.N + 16 * RG - 1) / (16 * RG), gy = (int)moe_max_tiles(a.slots, a.n_expert, 16 * TT);
    if (L.describe) {
        describe_line(L.describe, L.describe_len, "moe:%s_mmq TT=%d RG=%d KS=%d R=%d grid=%dx%d", kq_family(WT), TT, RG,
                      MMQ_WAVES / RG, 16 * TT, gx, gy);
        return hipSuccess;
    }
    const hipError_t e = launch_moe_plan(a, TT, L.st);
    if (e != hipSuccess) return e;
    if constexpr (WT == QG_TYPE_Q4_K) hipLaunchKernelGGL((q4k_moe_mmq_kernel<TT, RG>), dim3(gx, gy), dim3(MMQ_WGS), 0, L.st, a);
    else hipLaunchKernelGGL((q6k_moe_mmq_kernel<TT, RG>), dim3(gx, gy), dim3(MMQ_WGS), 0, L.st, a);
    return hipGetLastError();
}

template <int WT> hipError_t moe_prefill_t(const Launch& L) {
    const MoeForm f = moe_prefill_form(L.a, WT);
    if (f.rg == 4) return moe_prefill_k<WT, 4, 4>(L);
    if (f.tt == 4) return moe_prefill_k<WT, 4, 1>(L);
    if (f.tt == 2) return moe_prefill_k<WT, 2, 1>(L);
    return moe_prefill_k<WT, 1, 1>(L);
}

// The biased entry. Q4_K / Q6_K: the launch of the entry beside it, kernels and all, then moe_bias_add_kernel where there
// is a bias. MXFP4 takes the
// general rule of moe_prefill_form (the Q6_K exception is keyed on the type); its thresholds are borrowed from the
// K-quants, DESIGN.md 3j says what has been measured of them.
using BiasLaunch = MoeLaunch<MoeBiasArgs>;

template <int WT, int TT, int RG> hipError_t moe_prefill_bias_k(const BiasLaunch& L) {
    const MoeBiasArgs& a = L.a;
    if constexpr (WT != QG_TYPE_MXFP4) {
        const hipError_t e = moe_prefill_k<WT, TT, RG>(Launch{a, L.st, L.describe, L.describe_len});
        return e != hipSuccess || L.describe || !a.bias ? e : launch_moe_bias_add(a, L.st);
    }
    const int gx = (a.N + 16 * RG - 1) / (16 * RG), gy = (int)moe_max_tiles(a.slots, a.n_expert, 16 * TT);
    if (L.describe) {
        describe_line(L.describe, L.describe_len, "moe:mxfp4_mmq TT=%d RG=%d KS=%d R=%d grid=%dx%d", TT, RG, MMQ_WAVES / RG,
                      16 * TT, gx, gy);
        return hipSuccess;
    }
    const hipError_t e = launch_moe_plan(a, TT, L.st);
    if (e != hipSuccess) return e;
    if (a.bias)
        hipLaunchKernelGGL((mxfp4_moe_mmq_kernel<TT, RG, true>), dim3(gx, gy), dim3(MMQ_WGS), 0, L.st, a);
    else
        hipLaunchKernelGGL((mxfp4_moe_mmq_kernel<TT, RG, false>), dim3(gx, gy), dim3(MMQ_WGS), 0, L.st, a);
    return hipGetLastError();
}

template <int WT> hipError_t moe_prefill_bias_t(const BiasLaunch& L) {
    const MoeForm f = moe_prefill_form(L.a, WT);
    if (f.rg == 4) return moe_prefill_bias_k<WT, 4, 4>(L);
    if (f.tt == 4) return moe_prefill_bias_k<WT, 4, 1>(L);
    if (f.tt == 2) return moe_prefill_bias_k<WT, 2, 1>(L);
    return moe_prefill_bias_k<WT, 1, 1>(L);
}

}  // namespace

int moe_prefill_tt(const MoePlanArgs& a, int wtype) { return moe_prefill_form(a, wtype).tt; }

hipError_t launch_moe_plan(const MoePlanArgs& a, int tt, hipStream_t st) {
    return launch_moe_plan_rows(a, tt == 4 ? 6 : tt == 2 ? 5 : 4, st);
}

hipError_t launch_moe_prefill(const MoePlanArgs& a, int wtype, hipStream_t st, char* describe, size_t describe_len) {
    const Launch L{a, st, describe, describe_len};
    if (wtype == QG_TYPE_Q4_K) return moe_prefill_t<QG_TYPE_Q4_K>(L);
    if (wtype == QG_TYPE_Q6_K) return moe_prefill_t<QG_TYPE_Q6_K>(L);
    return hipErrorInvalidValue;
}

hipError_t launch_moe_bias_add(const MoeBiasArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(moe_bias_add_kernel, dim3((a.N + 255) / 256, a.slots), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_moe_prefill_bias(const MoeBiasArgs& a, int wtype, hipStream_t st, char* describe, size_t describe_len) {
    const BiasLaunch L{a, st, describe, describe_len};
    if (wtype == QG_TYPE_Q4_K) return moe_prefill_bias_t<QG_TYPE_Q4_K>(L);
    if (wtype == QG_TYPE_Q6_K) return moe_prefill_bias_t<QG_TYPE_Q6_K>(L);
    if (wtype == QG_TYPE_MXFP4) return moe_prefill_bias_t<QG_TYPE_MXFP4>(L);
    return hipErrorInvalidValue;
}

}  // namespace qg
