// qg_moe_glu_batch.hip — the expert-grouped decode GEMV gate / up product with its GLU (qg_gemm_w4a8_moe_glu_batch),
// families "moeb_glu:q4k_gemv", "moeb_glu:q6k_gemv", "moeb_glu:mxfp4_gemv": act(gate_e(x) + bg[e]) * (up_e(x) + bu[e])
// at 2 to 16 slots per expert, the sizes between qg_gemm_w4a8_moe_glu_bias (a slot per workgroup) and
// qg_gemm_w4a8_moe_glu_prefill (MFMA on 16-row tiles). DESIGN.md 3o.
//
// Two launches on the caller's stream, no allocation, no synchronisation, the host never reads ids:
//  1. moe_plan_kernel (qg_moe_plan.hip) with tiles of R = 2, 4 or 8 rows (moe_batch_rows), once for both products.
//  2. moeb_glu_kernel<WT, MT = R, LPR, WGS, ONE, BIAS> on the grid of qg_gemm_w4a8_moe_batch: blockIdx.x the row tile,
//     blockIdx.y the plan's tile, gridDim.y the host's bound moe_max_tiles. A workgroup
//       * reads n_tiles and its record and returns beyond n_tiles; a tile of the invalid bin stores +0.0f to its rows
//         and returns before any weight address is formed (moeb_glu_tile);
//       * BIAS: the lane that will hold a row's reduced sums loads its two bias floats of expert e, ahead of the passes:
//         they have arrived when the sums are reduced;
//       * gate pass: the type's decode GEMV body (qg_<type>_gemv_body.inc, the text the shipped kernels include) at
//         MT = R on expert e of B_gate. QG_KQ_ABLK gathers the tile's activation rows into the LDS records of tokens
//         0 .. rows - 1 as qg_moe_batch.hip does; QG_KQ_OUT(m) is res[m], a register: g[MT];
//       * up pass: the body again with QG_KQ_A_STAGED on expert e of B_up. It reads the records the gate pass staged:
//         no second staging and no barrier between the passes (the form profiles/moe_glu/README.md measured as the
//         better one for the decode entry), so a wave starts its up units as soon as its own gate sums are reduced.
//         The sums land in u[MT], with g[MT] live across the pass;
//       * epilogue: the lane that holds the sums applies the bias adds and the op to g[m], u[m] for m < tile.rows and
//         makes the one store per (row, slot) through the sorted list, C[sorted[first + m] * ldc + row]. The
//         2 * slots * N intermediate floats of the sequence (two grouped products, the bias adds, the op) never exist.
//     LPR, WGS and ONE are the single M = 1 call's (kq_gemv_form, kq_gemv_form_units(K / 32) for MXFP4), which depend
//     on K alone, and acc[m] takes the same expression in the same unit order for every m and every MT: g and u carry
//     the bits of qg_gemm_w4a8_moe on either operand whatever R, the tile or the sort position, and the op's
//     expressions are qg_gemm_w4a8_moe_glu_bias's (glu_op below restates glu_bias_op of qg_moe_glu.hip), each step one
//     rounded fp32 operation. LDS: R rows of records, the batch entry's.
#include "../../include/qg/qg.h"
#include "qg_kq_launch.hpp"
#include "qg_moe_glu_batch.hpp"
#include "qg_q4k.hpp"
#include "qg_q6k.hpp"

namespace qg {

// One decode GEMV product of the tile's M gathered rows (arows[0 .. M - 1]) with one expert's matrix, res[m] in the lane
// that holds the row's reduced sums (row < N and lane % LPR == LPR - 1; res untouched in every other lane and for
// m >= M). The body's constants as the batch entry passes them.
#define QG_KQ_DECLARE_TILE  // tile is a parameter here
#define QG_KQ_ABLK(g) A + ((long)arows[(g) / nb] * nb + ((g) - (g) / nb * nb)) * 9
#define QG_KQ_OUT(m) (*((void)C, &res[m]))
template <int MT, int LPR, int WGS, bool ONE>
__device__ __forceinline__ void q4k_moeb_glu_product(const uint32_t* __restrict__ A, const int32_t* __restrict__ arows,
                                                     const uint8_t* __restrict__ B, int M, int N, int K, const int tile,
                                                     float (&res)[MT]) {
    constexpr bool SUMI = false;
    void* const out = nullptr;
#include "qg_q4k_gemv_body.inc"
}

template <int MT, int LPR, int WGS, bool ONE>
__device__ __forceinline__ void q6k_moeb_glu_product(const uint32_t* __restrict__ A, const int32_t* __restrict__ arows,
                                                     const uint8_t* __restrict__ B, int M, int N, int K, const int tile,
                                                     float (&res)[MT]) {
    constexpr bool SUMI = false;
    void* const out = nullptr;
#include "qg_q6k_gemv_body.inc"
}

// MXFP4: B at any byte.
template <int MT, int LPR, int WGS, bool ONE>
__device__ __forceinline__ void mxfp4_moeb_glu_product(const uint32_t* __restrict__ A, const int32_t* __restrict__ arows,
                                                       const uint8_t* __restrict__ B, int M, int N, int K, const int tile,
                                                       float (&res)[MT]) {
    constexpr bool SUMI = false;
    void* const out = nullptr;
#include "qg_mxfp4_gemv_body.inc"
}

// The same with the tile's rows already in the LDS records (QG_KQ_A_STAGED: the up pass after the gate pass).
#define QG_KQ_A_STAGED
template <int MT, int LPR, int WGS, bool ONE>
__device__ __forceinline__ void q4k_moeb_glu_product_staged(const uint8_t* __restrict__ B, int M, int N, int K, const int tile,
                                                            float (&res)[MT]) {
    constexpr bool SUMI = false;
    void* const out = nullptr;
#include "qg_q4k_gemv_body.inc"
}

template <int MT, int LPR, int WGS, bool ONE>
__device__ __forceinline__ void q6k_moeb_glu_product_staged(const uint8_t* __restrict__ B, int M, int N, int K, const int tile,
                                                            float (&res)[MT]) {
    constexpr bool SUMI = false;
    void* const out = nullptr;
#include "qg_q6k_gemv_body.inc"
}

template <int MT, int LPR, int WGS, bool ONE>
__device__ __forceinline__ void mxfp4_moeb_glu_product_staged(const uint8_t* __restrict__ B, int M, int N, int K,
                                                              const int tile, float (&res)[MT]) {
    constexpr bool SUMI = false;
    void* const out = nullptr;
#include "qg_mxfp4_gemv_body.inc"
}
#undef QG_KQ_A_STAGED
#undef QG_KQ_OUT
#undef QG_KQ_ABLK
#undef QG_KQ_DECLARE_TILE

namespace {

// The tile of this workgroup (moe_tile_lookup). false: blockIdx.y is beyond n_tiles, or the tile belongs to the invalid
// bin and its rows are zeroed here (RPB: the workgroup's output rows), before any weight or bias address exists.
template <int RPB, int WGS> __device__ __forceinline__ bool moeb_glu_tile(const MoeGluBatchArgs& a, int tile, MoeTile& t) {
    if (!moe_tile_lookup(a, t)) return false;
    if ((unsigned)t.e >= (unsigned)a.n_expert) {
        for (int idx = threadIdx.x; idx < t.rows * RPB; idx += WGS) {
            const int p = idx / RPB, n = tile * RPB + (idx - p * RPB);
            if (n < a.N) a.C[(long)t.sorted[p] * a.ldc + n] = 0.0f;
        }
        return false;
    }
    return true;
}

// glu_bias_op of qg_moe_glu.hip, expression for expression: each operation one rounded fp32 operation (the build has
// contraction off and the correctly rounded division); x and y the clamped gate and up of gpt-oss's op.
__device__ __forceinline__ float glu_op(float g, float u, const MoeGluBatchArgs& a) {
    if (a.glu_op == QG_GLU_REGLU) return (g > 0.0f ? g : 0.0f) * u;
    if (a.glu_op != QG_GLU_SWIGLU_OAI) return (g / (1.0f + expf(-g))) * u;
    const float x = fminf(g, a.limit), y = fminf(fmaxf(u, -a.limit), a.limit);
    return (x / (1.0f + expf(a.alpha * (-x)))) * (y + 1.0f);
}

// BIAS: one of the two bias pointers is non-null; false: no bias load and no test of a pointer.
template <int WT, int MT, int LPR, int WGS, bool ONE, bool BIAS>
__global__ __launch_bounds__(WGS) void moeb_glu_kernel(const MoeGluBatchArgs a) {
    constexpr int RPW = 64 / LPR, RPB = (WGS / 64) * RPW;
    const int tile = xcd_tile_x();
    MoeTile mt;
    if (!moeb_glu_tile<RPB, WGS>(a, tile, mt)) return;
    // the body's row of this lane, and its holder of the reduced sums
    const int tid = threadIdx.x, lane = tid & 63;
    // LPR = 64: a wave per row, so the row, its biases and (once reduced) its sums are wave-uniform: SGPRs hold them
    constexpr bool WAVE_ROW = LPR == 64;
    const int lrow = tile * RPB + (tid >> 6) * RPW + lane / LPR;
    const int row = WAVE_ROW ? __builtin_amdgcn_readfirstlane(lrow) : lrow;
    const bool holder = row < a.N && lane % LPR == LPR - 1;
    float bg = 0.0f, bu = 0.0f;
    if constexpr (BIAS) {
        if (WAVE_ROW ? row < a.N : holder) {
            const long bo = (long)mt.e * a.bias_stride + row;
            if (a.bias_gate) bg = a.bias_gate[bo];
            if (a.bias_up) bu = a.bias_up[bo];
        }
        if constexpr (WAVE_ROW) {  // (the wait is the staging's: the loads stand ahead of its activation loads)
            bg = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(bg)));
            bu = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(bu)));
        }
    }
    // srt[m]: the slot of position m (positions past the tile's rows take the last one: loaded, never used)
    int srt[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) srt[m] = mt.sorted[min(m, mt.rows - 1)];
    const uint32_t* A = static_cast<const uint32_t*>(a.A);
    const long eoff = (long)mt.e * a.estride;  // 64 bits before any weight address
    const uint8_t* Bg = static_cast<const uint8_t*>(a.B) + eoff;
    const uint8_t* Bu = static_cast<const uint8_t*>(a.B_up) + eoff;
    float g[MT], u[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) g[m] = u[m] = 0.0f;
    // Between the passes. A wave per row: g[MT] leaves lane 63 for SGPRs, so the up pass carries no more VGPRs than the
    // batch entry's one product (Q6_K at MT = 8 does not fit 128 otherwise). Else the gate bias joins g here, so that bg
    // is dead across the up pass.
    auto after_gate = [&] {
        if constexpr (WAVE_ROW) {
#pragma unroll
            for (int m = 0; m < MT; ++m) g[m] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(g[m]), 63));
        } else if constexpr (BIAS) {
            if (a.bias_gate) {
#pragma unroll
                for (int m = 0; m < MT; ++m) g[m] = g[m] + bg;
            }
        }
    };
    if constexpr (WT == QG_TYPE_Q4_K) {
        q4k_moeb_glu_product<MT, LPR, WGS, ONE>(A, mt.arows, Bg, mt.rows, a.N, a.K, tile, g);
        after_gate();
        q4k_moeb_glu_product_staged<MT, LPR, WGS, ONE>(Bu, mt.rows, a.N, a.K, tile, u);
    } else if constexpr (WT == QG_TYPE_MXFP4) {
        mxfp4_moeb_glu_product<MT, LPR, WGS, ONE>(A, mt.arows, Bg, mt.rows, a.N, a.K, tile, g);
        after_gate();
        mxfp4_moeb_glu_product_staged<MT, LPR, WGS, ONE>(Bu, mt.rows, a.N, a.K, tile, u);
    } else {
        q6k_moeb_glu_product<MT, LPR, WGS, ONE>(A, mt.arows, Bg, mt.rows, a.N, a.K, tile, g);
        after_gate();
        q6k_moeb_glu_product_staged<MT, LPR, WGS, ONE>(Bu, mt.rows, a.N, a.K, tile, u);
    }
    if (holder) {
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < mt.rows) {
                float gm = g[m], um = u[m];
                if constexpr (BIAS) {
                    if (WAVE_ROW && a.bias_gate) gm = gm + bg;
                    if (a.bias_up) um = um + bu;
                }
                a.C[(long)srt[m] * a.ldc + row] = glu_op(gm, um, a);
            }
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
using Launch = MoeLaunch<MoeGluBatchArgs>;

// The plan for tiles of MT rows, once, then the fused product at the single M = 1 call's LPR, WGS and ONE.
template <int WT, int MT> hipError_t moeb_glu_mt(const Launch& L) {
    return kq_gemv_form_units(kq_row_units(WT, L.a.K), [&](auto lpr, auto wgs, auto one) -> hipError_t {
        constexpr int LPR = lpr, WGS = wgs, RPB = (WGS / 64) * (64 / LPR);
        constexpr bool ONE = one;
        const MoeGluBatchArgs& a = L.a;
        const size_t lds = (size_t)MT * moe_batch_row_lds(a.K, WT);
        const int gy = (int)moe_max_tiles(a.slots, a.n_expert, MT);
        if (L.describe) {
            describe_line(L.describe, L.describe_len, "moeb_glu:%s_gemv R=%d LPR=%d WGS=%d ONE=%d grid=%dx%d lds=%zu",
                          kq_family(WT), MT, LPR, WGS, (int)ONE, (a.N + RPB - 1) / RPB, gy, lds);
            return hipSuccess;
        }
        int rsh = 0;
        while ((1 << rsh) < MT) ++rsh;
        const hipError_t e = launch_moe_plan_rows(a, rsh, L.st);
        if (e != hipSuccess) return e;
        static std::atomic<unsigned long long> done[2];
        if (a.bias_gate || a.bias_up)
            return moe_enqueue(moeb_glu_kernel<WT, MT, LPR, WGS, ONE, true>, L, RPB, gy, WGS, lds, done[0]);
        return moe_enqueue(moeb_glu_kernel<WT, MT, LPR, WGS, ONE, false>, L, RPB, gy, WGS, lds, done[1]);
    });
}

template <int WT> hipError_t moeb_glu_r(const Launch& L) {
    switch (moe_batch_rows(L.a.slots, L.a.n_expert, L.a.K, WT)) {
        case 2: return moeb_glu_mt<WT, 2>(L);
        case 4: return moeb_glu_mt<WT, 4>(L);
        case 8: return moeb_glu_mt<WT, 8>(L);
    }
    return hipErrorInvalidValue;
}

}  // namespace

hipError_t launch_moe_glu_batch(const MoeGluBatchArgs& a, int wtype, hipStream_t st, char* describe, size_t describe_len) {
    const Launch L{a, st, describe, describe_len};
    switch (wtype) {
        case QG_TYPE_Q4_K: return moeb_glu_r<QG_TYPE_Q4_K>(L);
        case QG_TYPE_Q6_K: return moeb_glu_r<QG_TYPE_Q6_K>(L);
        case QG_TYPE_MXFP4: return moeb_glu_r<QG_TYPE_MXFP4>(L);
    }
    return hipErrorInvalidValue;
}

}  // namespace qg
