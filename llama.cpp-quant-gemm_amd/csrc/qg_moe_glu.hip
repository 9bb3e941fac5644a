// qg_moe_glu.hip — the fused gate / up mul_mat_id with its GLU (qg_gemm_w4a8_moe_glu), families "moe_glu:q4k_gemv",
// "moe_glu:q6k_gemv": the first half of an MoE FFN block, act(gate(x)) * up(x), in one launch.
//
// The grid is the decode entry's (qg_moe.hip): blockIdx.y is the slot s = t * n_used + u, blockIdx.x its row tile, the
// expert id one scalar load, an id outside [0, n_expert) a workgroup-uniform branch that stores +0.0f and returns
// before any weight address is formed. A workgroup then runs the Q4_K / Q6_K decode GEMV body twice on the token's
// activation row, at the single call's LPR, WGS and ONE: once on expert e of B_gate, once on expert e of B_up. The body
// is the very text the shipped kernel and the decode entry include (qg_q4k_gemv_body.inc, qg_q6k_gemv_body.inc) with its
// output bound to a register, so g and u carry the bits of qg_gemm_w4a8_moe on either operand. The lane that holds the
// reduced sums applies the op and makes the slot's one store per row: the two slots x N intermediate floats of the
// three-kernel sequence are never written.
// The gate pass stages the activation row into the LDS records (the body's own prologue, with its barrier); the up pass
// includes the body with QG_KQ_A_STAGED and reads the same records: no second staging and no barrier between the
// passes, so a wave starts its up units as soon as its own gate sum is reduced. profiles/moe_glu/README.md: against
// staging in both passes (QG_MOE_GLU_STAGE_ONCE=0, the form the entry started from), captured, it takes 0.83 - 0.96 of
// the time in seven of the eight measured classes and the same time in one (Mixtral Q4_K at 16 slots), with the same bits.
// The arguments travel by value (no device allocation, capture-safe); the host never reads ids.
// qg_gemm_w4a8_moe_glu_bias (the same with per-expert bias rows, gpt-oss's clamped SwiGLU and MXFP4 experts, family
// "moe_glu:mxfp4_gemv" beside the two above) is kq_moe_glu_bias_kernel below: the same structure in a kernel of its own.
#include "../../include/qg/qg.h"
#include "qg_kq_launch.hpp"
#include "qg_moe_glu.hpp"
#include "qg_q4k.hpp"
#include "qg_q6k.hpp"

namespace qg {

// One decode GEMV product at one activation row, returned in the lane that holds the row's reduced sum (row < N and
// lane % LPR == LPR - 1; 0.0f in every other lane): the body's four constants as the single call passes them at M = 1.
#define QG_KQ_DECLARE_TILE  // tile is a parameter here
#define QG_KQ_ABLK(g) A + (long)g * 9
#define QG_KQ_OUT(m) (*((void)C, &res))
template <int LPR, int WGS, bool ONE>
__device__ __forceinline__ float q4k_glu_product(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B, int N, int K,
                                                 const int tile) {
    constexpr int MT = 1, M = 1;
    constexpr bool SUMI = false;
    void* const out = nullptr;
    float res = 0.0f;
#include "qg_q4k_gemv_body.inc"
    return res;
}

template <int LPR, int WGS, bool ONE>
__device__ __forceinline__ float q6k_glu_product(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B, int N, int K,
                                                 const int tile) {
    constexpr int MT = 1, M = 1;
    constexpr bool SUMI = false;
    void* const out = nullptr;
    float res = 0.0f;
#include "qg_q6k_gemv_body.inc"
    return res;
}

// The same with the activation row already in the LDS records (QG_KQ_A_STAGED: the up pass after the gate pass).
#define QG_KQ_A_STAGED
template <int LPR, int WGS, bool ONE>
__device__ __forceinline__ float q4k_glu_product_staged(const uint8_t* __restrict__ B, int N, int K, const int tile) {
    constexpr int MT = 1, M = 1;
    constexpr bool SUMI = false;
    void* const out = nullptr;
    float res = 0.0f;
#include "qg_q4k_gemv_body.inc"
    return res;
}

template <int LPR, int WGS, bool ONE>
__device__ __forceinline__ float q6k_glu_product_staged(const uint8_t* __restrict__ B, int N, int K, const int tile) {
    constexpr int MT = 1, M = 1;
    constexpr bool SUMI = false;
    void* const out = nullptr;
    float res = 0.0f;
#include "qg_q6k_gemv_body.inc"
    return res;
}
#undef QG_KQ_A_STAGED

// MXFP4 (qg_gemm_w4a8_moe_glu_bias alone): the same two forms of qg_mxfp4_gemv_body.inc, B at any byte.
template <int LPR, int WGS, bool ONE>
__device__ __forceinline__ float mxfp4_glu_product(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B, int N, int K,
                                                   const int tile) {
    constexpr int MT = 1, M = 1;
    constexpr bool SUMI = false;
    void* const out = nullptr;
    float res = 0.0f;
#include "qg_mxfp4_gemv_body.inc"
    return res;
}

#define QG_KQ_A_STAGED
template <int LPR, int WGS, bool ONE>
__device__ __forceinline__ float mxfp4_glu_product_staged(const uint8_t* __restrict__ B, int N, int K, const int tile) {
    constexpr int MT = 1, M = 1;
    constexpr bool SUMI = false;
    void* const out = nullptr;
    float res = 0.0f;
#include "qg_mxfp4_gemv_body.inc"
    return res;
}
#undef QG_KQ_A_STAGED
#undef QG_KQ_OUT
#undef QG_KQ_ABLK
#undef QG_KQ_DECLARE_TILE

// 1: the up pass reads the records the gate pass staged; 0: both passes stage, a barrier between them (A/B builds).
#ifndef QG_MOE_GLU_STAGE_ONCE
#define QG_MOE_GLU_STAGE_ONCE 1
#endif

namespace {

// Each operation one rounded fp32 operation (the build has contraction off and the correctly rounded division).
__device__ __forceinline__ float glu(float g, float u, int op) {
    if (op == QG_GLU_REGLU) return (g > 0.0f ? g : 0.0f) * u;
    return (g / (1.0f + expf(-g))) * u;
}

template <int WT, int LPR, int WGS, bool ONE>
__global__ __launch_bounds__(WGS) void kq_moe_glu_kernel(const MoeGluArgs a) {
    constexpr int RPW = 64 / LPR, RPB = (WGS / 64) * RPW;
    const int tile = xcd_tile_x();  // the single launch's order within the slot
    const int slot = blockIdx.y;
    const int t = slot / a.n_used, us = slot - t * a.n_used;
    const int e = a.ids[(long)t * a.ids_stride + us];
    float* C = a.C + (long)slot * a.ldc;
    if ((unsigned)e >= (unsigned)a.n_expert) {
        const int r1 = min(a.N, (tile + 1) * RPB);
        for (int r = tile * RPB + (int)threadIdx.x; r < r1; r += WGS) C[r] = 0.0f;
        return;
    }
    const uint32_t* A = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(a.A) + (long)t * a.arow);
    const long eoff = (long)e * a.estride;
    const uint8_t* Bg = static_cast<const uint8_t*>(a.B_gate) + eoff;
    const uint8_t* Bu = static_cast<const uint8_t*>(a.B_up) + eoff;
    float g, u;
    if constexpr (WT == QG_TYPE_Q4_K) {
        g = q4k_glu_product<LPR, WGS, ONE>(A, Bg, a.N, a.K, tile);
#if QG_MOE_GLU_STAGE_ONCE
        u = q4k_glu_product_staged<LPR, WGS, ONE>(Bu, a.N, a.K, tile);
#else
        __syncthreads();
        u = q4k_glu_product<LPR, WGS, ONE>(A, Bu, a.N, a.K, tile);
#endif
    } else {
        g = q6k_glu_product<LPR, WGS, ONE>(A, Bg, a.N, a.K, tile);
#if QG_MOE_GLU_STAGE_ONCE
        u = q6k_glu_product_staged<LPR, WGS, ONE>(Bu, a.N, a.K, tile);
#else
        __syncthreads();
        u = q6k_glu_product<LPR, WGS, ONE>(A, Bu, a.N, a.K, tile);
#endif
    }
    // the body's row of this lane, and its holder of the reduced sum
    const int tid = threadIdx.x, lane = tid & 63;
    const int row = tile * RPB + (tid >> 6) * RPW + lane / LPR;
    if (row < a.N && lane % LPR == LPR - 1) C[row] = glu(g, u, a.glu_op);
}

// qg_gemm_w4a8_moe_glu_bias: gpt-oss's op beside the two above, x and y the clamped gate and up.
__device__ __forceinline__ float glu_bias_op(float g, float u, const MoeGluBiasArgs& a) {
    if (a.glu_op != QG_GLU_SWIGLU_OAI) return glu(g, u, a.glu_op);
    const float x = fminf(g, a.limit), y = fminf(fmaxf(u, -a.limit), a.limit);
    return (x / (1.0f + expf(a.alpha * (-x)))) * (y + 1.0f);
}

// The kernel above (its grid, id load and zero-store branch, its two passes) for Q4_K / Q6_K / MXFP4 with the per-expert
// bias rows and the third op: a kernel of its own, so that kq_moe_glu_kernel keeps its argument block and its code.
// BIAS: one of the two bias pointers is non-null; false: no bias load and no test of a pointer. The lane that will hold
// the reduced sums loads its two bias floats ahead of the passes, once the id is known to be in range: they have arrived
// when the sums are reduced.
template <int WT, int LPR, int WGS, bool ONE, bool BIAS>
__global__ __launch_bounds__(WGS) void kq_moe_glu_bias_kernel(const MoeGluBiasArgs a) {
    constexpr int RPW = 64 / LPR, RPB = (WGS / 64) * RPW;
    const int tile = xcd_tile_x();
    const int slot = blockIdx.y;
    const int t = slot / a.n_used, us = slot - t * a.n_used;
    const int e = a.ids[(long)t * a.ids_stride + us];
    float* C = a.C + (long)slot * a.ldc;
    if ((unsigned)e >= (unsigned)a.n_expert) {
        const int r1 = min(a.N, (tile + 1) * RPB);
        for (int r = tile * RPB + (int)threadIdx.x; r < r1; r += WGS) C[r] = 0.0f;
        return;
    }
    const int tid = threadIdx.x, lane = tid & 63;
    const int row = tile * RPB + (tid >> 6) * RPW + lane / LPR;
    const bool holder = row < a.N && lane % LPR == LPR - 1;
    float bg = 0.0f, bu = 0.0f;
    if constexpr (BIAS) {
        if (holder) {
            const long bo = (long)e * a.bias_stride + row;
            if (a.bias_gate) bg = a.bias_gate[bo];
            if (a.bias_up) bu = a.bias_up[bo];
        }
    }
    const uint32_t* A = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(a.A) + (long)t * a.arow);
    const long eoff = (long)e * a.estride;
    const uint8_t* Bg = static_cast<const uint8_t*>(a.B_gate) + eoff;
    const uint8_t* Bu = static_cast<const uint8_t*>(a.B_up) + eoff;
    float g, u;
    if constexpr (WT == QG_TYPE_Q4_K) {
        g = q4k_glu_product<LPR, WGS, ONE>(A, Bg, a.N, a.K, tile);
        u = q4k_glu_product_staged<LPR, WGS, ONE>(Bu, a.N, a.K, tile);
    } else if constexpr (WT == QG_TYPE_MXFP4) {
        g = mxfp4_glu_product<LPR, WGS, ONE>(A, Bg, a.N, a.K, tile);
        u = mxfp4_glu_product_staged<LPR, WGS, ONE>(Bu, a.N, a.K, tile);
    } else {
        g = q6k_glu_product<LPR, WGS, ONE>(A, Bg, a.N, a.K, tile);
        u = q6k_glu_product_staged<LPR, WGS, ONE>(Bu, a.N, a.K, tile);
    }
    if (holder) {
        if constexpr (BIAS) {
            if (a.bias_gate) g = g + bg;
            if (a.bias_up) u = u + bu;
        }
        C[row] = glu_bias_op(g, u, a);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------
// The single M = 1 call's LPR, WGS and ONE (kq_gemv_form, qg_kq_launch.hpp), on the decode entry's grid.
template <int WT> hipError_t moe_glu_launch_t(const MoeLaunch<MoeGluArgs>& L) {
    return kq_gemv_form(L.a.K, [&](auto lpr, auto wgs, auto one) -> hipError_t {
        constexpr int LPR = lpr, WGS = wgs, RPB = (WGS / 64) * (64 / LPR);
        const size_t lds = (size_t)(L.a.K / SB_ELEMS) * kq_gemv_rec_dw(WT) * 4;
        if (L.describe) {
            describe_line(L.describe, L.describe_len, "moe_glu:%s_gemv LPR=%d WGS=%d ONE=%d grid=%dx%d lds=%zu", kq_family(WT), LPR,
                          WGS, (int)one, (L.a.N + RPB - 1) / RPB, L.a.slots, lds);
            return hipSuccess;
        }
        static std::atomic<unsigned long long> done;
        return moe_enqueue(kq_moe_glu_kernel<WT, LPR, WGS, one>, L, RPB, L.a.slots, WGS, lds, done);
    });
}

// The same form; MXFP4: a block per unit and per LDS record, as moe_kq_launch (qg_moe.hip).
template <int WT> hipError_t moe_glu_bias_launch_t(const MoeLaunch<MoeGluBiasArgs>& L) {
    constexpr bool MX = WT == QG_TYPE_MXFP4;
    return kq_gemv_form_units(MX ? (L.a.K / QK + MXFP4_UB - 1) / MXFP4_UB : L.a.K / 64, [&](auto lpr, auto wgs, auto one) -> hipError_t {
        constexpr int LPR = lpr, WGS = wgs, RPB = (WGS / 64) * (64 / LPR);
        const size_t lds = MX ? (size_t)(L.a.K / QK) * MXFP4_REC_DW * 4 : (size_t)(L.a.K / SB_ELEMS) * kq_gemv_rec_dw(WT) * 4;
        if (L.describe) {
            describe_line(L.describe, L.describe_len, "moe_glu:%s_gemv LPR=%d WGS=%d ONE=%d grid=%dx%d lds=%zu",
                          MX ? "mxfp4" : kq_family(WT), LPR, WGS, (int)one, (L.a.N + RPB - 1) / RPB, L.a.slots, lds);
            return hipSuccess;
        }
        static std::atomic<unsigned long long> done_bias, done_plain;
        if (L.a.bias_gate || L.a.bias_up)
            return moe_enqueue(kq_moe_glu_bias_kernel<WT, LPR, WGS, one, true>, L, RPB, L.a.slots, WGS, lds, done_bias);
        return moe_enqueue(kq_moe_glu_bias_kernel<WT, LPR, WGS, one, false>, L, RPB, L.a.slots, WGS, lds, done_plain);
    });
}

}  // namespace

hipError_t launch_moe_glu_bias(const MoeGluBiasArgs& a, int wtype, hipStream_t st, char* describe, size_t describe_len) {
    const MoeLaunch<MoeGluBiasArgs> L{a, st, describe, describe_len};
    switch (wtype) {
        case QG_TYPE_Q4_K: return moe_glu_bias_launch_t<QG_TYPE_Q4_K>(L);
        case QG_TYPE_Q6_K: return moe_glu_bias_launch_t<QG_TYPE_Q6_K>(L);
        case QG_TYPE_MXFP4: return moe_glu_bias_launch_t<QG_TYPE_MXFP4>(L);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_moe_glu(const MoeGluArgs& a, int wtype, hipStream_t st, char* describe, size_t describe_len) {
    const MoeLaunch<MoeGluArgs> L{a, st, describe, describe_len};
    switch (wtype) {
        case QG_TYPE_Q4_K: return moe_glu_launch_t<QG_TYPE_Q4_K>(L);
        case QG_TYPE_Q6_K: return moe_glu_launch_t<QG_TYPE_Q6_K>(L);
    }
    return hipErrorInvalidValue;
}

}  // namespace qg
