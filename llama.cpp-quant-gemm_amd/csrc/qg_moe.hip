// qg_moe.hip — the expert-indexed decode GEMV (qg_gemm_w4a8_moe, ggml's mul_mat_id), families "moe:gemv",
// "moe:q4k_gemv", "moe:q6k_gemv", "moe:mxfp4_gemv".
//
// One launch computes the T * n_used expert products of a decode step: blockIdx.y is the slot s = t * n_used + u,
// blockIdx.x its row tile. The workgroup reads its expert id e = ids[t * ids_stride + u] from device memory with one
// scalar load (the slot is uniform over the workgroup), forms the slot's activation row, expert matrix and output
// row from 64-bit offsets and then runs the very body the single M = 1 product runs for this (type, K):
//   * Q4_0 .. Q8_0: gemv_body<F, 1, BPL, LPR, ...> (qg_gemv_kernel.hpp) with the BPL / LPR / ONEU of the single call:
//     the launcher visits the single call's own choice, gemv_form (qg_gemv_impl.hpp) and gemv_unit_form
//     (qg_gemv_kernel.hpp). The workgroup size and the row tiles per workgroup are the grouped launch's
//     (gemv_small_wg): half-size workgroups of two tiles while N fits one round of full-size ones, full-size ones
//     beyond (of one tile for Q8_0, moe_big_tpw). Neither changes a row's arithmetic.
//   * Q4_K / Q6_K: q4k_moe_body / q6k_moe_body<LPR, WGS, ONE> (below: the shipped kernels' bodies at one activation
//     row, the same text included: qg_q4k_gemv_body.inc, qg_q6k_gemv_body.inc), the single call's LPR, WGS and ONE
//     (kq_gemv_form, qg_kq_launch.hpp).
//   * MXFP4: mxfp4_moe_body<LPR, WGS, ONE> (qg_mxfp4_gemv_body.inc at one activation row), the single call's form for
//     K / 32 units (kq_gemv_form_units). The expert stride N * K/32 * 17 is any number of bytes: the body's loads are
//     realigned by each block's own address, so an expert at any byte offset is read as the single call reads it.
// So every slot's outputs are bit-identical to the eager qg_gemm_w4a8 on that slot's operands.
// An id outside [0, n_expert) is a workgroup-uniform branch taken before any weight address is formed: the
// workgroup stores +0.0f to its rows of the slot and returns.
// The arguments travel by value (no device allocation, capture-safe); the host never reads ids.
#include "../../include/qg/qg.h"
#include "qg_gemv_impl.hpp"
#include "qg_kq_launch.hpp"
#include "qg_mxfp4.hpp"
#include "qg_q4k.hpp"
#include "qg_q6k.hpp"

namespace qg {

// The shipped Q4_K / Q6_K decode GEMV bodies at one activation row: the four constants the single call passes at
// M = 1, the row tile as a parameter, and the very text q4k_gemv_kernel / q6k_gemv_kernel include.
#define QG_KQ_DECLARE_TILE  // tile is a parameter here
#define QG_KQ_ABLK(g) A + (long)g * 9
#define QG_KQ_OUT(m) C[m * ldc + row]
template <int LPR, int WGS, bool ONE>
__device__ __forceinline__ void q4k_moe_body(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B, int N, int K,
                                             void* __restrict__ out, const int tile) {
    constexpr int MT = 1, M = 1;
    constexpr bool SUMI = false;
    constexpr long ldc = 0;
#include "qg_q4k_gemv_body.inc"
}

template <int LPR, int WGS, bool ONE>
__device__ __forceinline__ void q6k_moe_body(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B, int N, int K,
                                             void* __restrict__ out, const int tile) {
    constexpr int MT = 1, M = 1;
    constexpr bool SUMI = false;
    constexpr long ldc = 0;
#include "qg_q6k_gemv_body.inc"
}

template <int LPR, int WGS, bool ONE>
__device__ __forceinline__ void mxfp4_moe_body(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B, int N, int K,
                                               void* __restrict__ out, const int tile) {
    constexpr int MT = 1, M = 1;
    constexpr bool SUMI = false;
    constexpr long ldc = 0;
#include "qg_mxfp4_gemv_body.inc"
}
#undef QG_KQ_OUT
#undef QG_KQ_ABLK
#undef QG_KQ_DECLARE_TILE

namespace {

// Row tiles per full-size workgroup of the loop-free row form once N exceeds one round (0: per format; A/B builds
// force 1 or 2). profiles/moe/ab_moe_tpw.txt, N = 14336, K = 4096, us per slot at 2 / 8 / 16 slots, two tiles -> one:
// Q8_0 13.91 -> 12.21, 10.26 -> 9.55, 9.56 -> 8.93 (at 2 slots two tiles lose to one kernel node per slot, 12.8);
// Q4_0 8.22 -> 8.33, 5.59 -> 5.79, 4.78 -> 5.10. Q4_1 / Q5_0 / Q5_1 are not measured and keep the grouped launch's 2.
#ifndef QG_MOE_BIG_TPW
#define QG_MOE_BIG_TPW 0
#endif
template <int F> constexpr int moe_big_tpw = QG_MOE_BIG_TPW ? QG_MOE_BIG_TPW : F == FMT_Q8_0 ? 1 : 2;

struct MoeSlot {
    const uint32_t* A;
    const uint8_t* B;
    float* C;
};

// The slot of this workgroup. false: its id names no expert; the workgroup's RPB rows of the slot are zeroed.
template <int WGS> __device__ __forceinline__ bool moe_slot(const MoeArgs& a, int RPB, int tile, MoeSlot& s) {
    const int slot = blockIdx.y;
    const int t = slot / a.n_used, u = slot - t * a.n_used;
    const int e = a.ids[(long)t * a.ids_stride + u];
    s.C = a.C + (long)slot * a.ldc;
    if ((unsigned)e >= (unsigned)a.n_expert) {
        const int r1 = min(a.N, (tile + 1) * RPB);
        for (int r = tile * RPB + (int)threadIdx.x; r < r1; r += WGS) s.C[r] = 0.0f;
        return false;
    }
    // a_rows is 1 (the token's one row) or n_used (a row per slot): u % a_rows
    const int ar = a.a_rows > 1 ? u : 0;
    s.A = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(a.A) + ((long)t * a.a_rows + ar) * a.arow);
    s.B = static_cast<const uint8_t*>(a.B) + (long)e * a.estride;
    return true;
}

template <int F, int BPL, int LPR, int WGS, int ONEU, int TPW>
__global__ __launch_bounds__(WGS) void gemv_moe_kernel(const MoeArgs a) {
    constexpr int RPB = (WGS / 64) * (64 / LPR) * TPW;  // rows per workgroup
    const int tile = xcd_tile_x();  // the single launch's order within the slot
    MoeSlot s;
    if (!moe_slot<WGS>(a, RPB, tile, s)) return;
    gemv_body<F, 1, BPL, LPR, WGS, false, AIN_Q8_1, false, true, ONEU, TPW>(s.A, s.B, 0, 0, 1, a.N, a.K, s.C, 0, 0, 1,
                                                                             nullptr, tile);
}

template <int WT, int LPR, int WGS, bool ONE>
__global__ __launch_bounds__(WGS) void kq_moe_kernel(const MoeArgs a) {
    constexpr int RPB = (WGS / 64) * (64 / LPR);
    const int tile = xcd_tile_x();  // the single launch's order within the slot
    MoeSlot s;
    if (!moe_slot<WGS>(a, RPB, tile, s)) return;
    if constexpr (WT == QG_TYPE_Q4_K) q4k_moe_body<LPR, WGS, ONE>(s.A, s.B, a.N, a.K, s.C, tile);
    else if constexpr (WT == QG_TYPE_MXFP4) mxfp4_moe_body<LPR, WGS, ONE>(s.A, s.B, a.N, a.K, s.C, tile);
    else q6k_moe_body<LPR, WGS, ONE>(s.A, s.B, a.N, a.K, s.C, tile);
}

// ---- host side -----------------------------------------------------------------------------------------------
using Launch = MoeLaunch<MoeArgs>;

template <int F, int BPL, int LPR, int WGS, int ONEU, int TPW> hipError_t moe_row_k(const Launch& L) {
    constexpr int RPB = (WGS / 64) * (64 / LPR) * TPW;
    const size_t lds = gemv_lds_bytes<F, BPL>(1, L.a.K);
    if (L.describe) {
        describe_line(L.describe, L.describe_len, "moe:gemv F=%d BPL=%d LPR=%d WGS=%d ONEU=%d TPW=%d grid=%dx%d lds=%zu", F, BPL,
                      LPR, WGS, ONEU, TPW, (L.a.N + RPB - 1) / RPB, L.a.slots, lds);
        return hipSuccess;
    }
    static std::atomic<unsigned long long> done;
    return moe_enqueue(gemv_moe_kernel<F, BPL, LPR, WGS, ONEU, TPW>, L, RPB, L.a.slots, WGS, lds, done);
}

// The single M = 1 call's (BPL, LPR, WGS) and unit form (gemv_form, gemv_unit_form). This launch's own: the one-unit
// form takes the grouped launch's workgroups (gemv_small_wg: half-size ones of two row tiles while N fits one round of
// full-size ones) and moe_big_tpw tiles per full-size workgroup beyond.
template <int F, int BPL, int LPR, int WGS> hipError_t moe_row_cfg(const Launch& L) {
    const int nu = gemv_unit_form<F, 1>(L.a.K / QK / BPL, LPR);
    if (nu == 1) {
        constexpr GemvSmallWg S = gemv_small_wg(WGS, 1, QG_GEMVG_WDIV, QG_GEMVG_TPW);
        if constexpr (S.wgs > 0) {
            constexpr int RPBF = (WGS / 64) * (64 / LPR) * QG_GEMVG_TPW;
            if ((L.a.N + RPBF - 1) / RPBF <= device_cus()) return moe_row_k<F, BPL, LPR, S.wgs, 1, S.tpw>(L);
        }
        return moe_row_k<F, BPL, LPR, WGS, 1, moe_big_tpw<F>>(L);
    }
    if constexpr (gemv_nu_ok<F, 1>) {
        if (nu == 2) return moe_row_k<F, BPL, LPR, WGS, 2, 1>(L);
        if (nu == 4) return moe_row_k<F, BPL, LPR, WGS, 4, 1>(L);
    }
    return moe_row_k<F, BPL, LPR, WGS, 0, 1>(L);
}

template <int F> hipError_t moe_row(const Launch& L) {
    return gemv_form<F, 1, AIN_Q8_1, false>(L.a.N, L.a.K, [&](auto bpl, auto lpr, auto wgs, auto pre) {
        static_assert(decltype(pre)::value, "gemv_moe_kernel passes PRE = true");
        return moe_row_cfg<F, bpl, lpr, wgs>(L);
    });
}

// (MXFP4: a block per unit and per LDS record, where the super-block types have 64 elements and a super-block)
template <int WT> hipError_t moe_kq_launch(const Launch& L) {
    constexpr bool MX = WT == QG_TYPE_MXFP4;
    return kq_gemv_form_units(MX ? (L.a.K / QK + MXFP4_UB - 1) / MXFP4_UB : L.a.K / 64, [&](auto lpr, auto wgs, auto one) -> hipError_t {
        constexpr int LPR = lpr, WGS = wgs, RPB = (WGS / 64) * (64 / LPR);
        const size_t lds = MX ? (size_t)(L.a.K / QK) * MXFP4_REC_DW * 4 : (size_t)(L.a.K / SB_ELEMS) * kq_gemv_rec_dw(WT) * 4;
        if (L.describe) {
            describe_line(L.describe, L.describe_len, "moe:%s_gemv LPR=%d WGS=%d ONE=%d grid=%dx%d lds=%zu", MX ? "mxfp4" : kq_family(WT), LPR, WGS,
                          (int)one, (L.a.N + RPB - 1) / RPB, L.a.slots, lds);
            return hipSuccess;
        }
        static std::atomic<unsigned long long> done;
        return moe_enqueue(kq_moe_kernel<WT, LPR, WGS, one>, L, RPB, L.a.slots, WGS, lds, done);
    });
}

}  // namespace

// The row types' LDS records of one activation row must fit (the single call has no such test at M <= 2 and fails
// in the launch instead); the super-block types' and MXFP4's bound is their gemv_eligible.
bool moe_lds_ok(int wtype, int K) {
    if (wtype == QG_TYPE_Q4_K || wtype == QG_TYPE_Q6_K || wtype == QG_TYPE_MXFP4) return true;
    return gemv_lds_bytes<FMT_Q4_0, 2>(1, K) <= MAX_LDS_BYTES;  // (2-block units: the record size is the formats' common one)
}

hipError_t launch_moe(const MoeArgs& a, int wtype, hipStream_t st, char* describe, size_t describe_len) {
    const Launch L{a, st, describe, describe_len};
    switch (wtype) {
        case FMT_Q4_0: return moe_row<FMT_Q4_0>(L);
        case FMT_Q4_1: return moe_row<FMT_Q4_1>(L);
        case FMT_Q5_0: return moe_row<FMT_Q5_0>(L);
        case FMT_Q5_1: return moe_row<FMT_Q5_1>(L);
        case FMT_Q8_0: return moe_row<FMT_Q8_0>(L);
        case QG_TYPE_Q4_K: return moe_kq_launch<QG_TYPE_Q4_K>(L);
        case QG_TYPE_Q6_K: return moe_kq_launch<QG_TYPE_Q6_K>(L);
        case QG_TYPE_MXFP4: return moe_kq_launch<QG_TYPE_MXFP4>(L);
    }
    return hipErrorInvalidValue;
}

}  // namespace qg
