// qg_moe_batch.hip — the expert-grouped decode GEMV (qg_gemm_w4a8_moe_batch, ggml's mul_mat_id for batched decode),
// families "moeb:q4k_gemv" and "moeb:q6k_gemv". DESIGN.md 3e. And its biased twin qg_gemm_w4a8_moe_batch_bias with MXFP4
// experts beside them, family "moeb:mxfp4_gemv" (DESIGN.md 3j): kernels of its own further down, these untouched.
//
// Two launches on the caller's stream, no allocation, no synchronisation, the host never reads ids:
//  1. moe_plan_kernel (qg_moe_plan.hip) with tiles of R = 2, 4 or 8 rows: the T * n_used slots counting-sorted by
//     expert id into the caller's workspace, one record {bin, first sorted position, rows} per tile.
//  2. q4k_moeb_kernel / q6k_moeb_kernel<MT = R, LPR, WGS, ONE>: the body of q4k_gemv_kernel / q6k_gemv_kernel
//     (qg_q4k_gemv.hip, qg_q6k_gemv.hip: the work decomposition is described there), the same text included
//     (qg_q4k_gemv_body.inc, qg_q6k_gemv_body.inc), at the LPR, WGS and ONE the single M = 1 call takes for this K
//     (kq_gemv_form, qg_kq_launch.hpp). What differs, all of it in the prologue and in the body's two hooks:
//       * blockIdx.y is a tile index. The workgroup reads n_tiles and its record (uniform) and returns at once
//         beyond n_tiles: gridDim.y is the host's upper bound moe_max_tiles.
//       * activation block g = m * K/32 + b of the staging is block b of row rows[first + m] (QG_KQ_ABLK): the R
//         gathered rows land in the LDS records of tokens 0 .. rows - 1, and the body runs with M = tile.rows.
//       * the expert's matrix is B + e * estride, formed in 64 bits before any weight address.
//       * token m's output goes to C + sorted[first + m] * ldc (QG_KQ_OUT).
//       * a tile of the invalid bin stores +0.0f to its rows and returns before any weight address is formed.
//     A token's accumulation chain is its own: acc[m] takes the same expression in the same unit order for every m and
//     every MT, and LPR / ONE depend on K alone. So a slot's bits do not depend on R, on the tile or on the position
//     the sort gave it, and equal those of qg_gemm_w4a8_moe and of the eager M = 1 qg_gemm_w4a8.
#include "../../include/qg/qg.h"
#include "qg_kq_launch.hpp"
#include "qg_moe_batch.hpp"
#include "qg_q4k.hpp"
#include "qg_q6k.hpp"

namespace qg {
namespace {

// The tile of this workgroup (moe_tile_lookup). false: blockIdx.y is beyond n_tiles, or the tile belongs to the invalid
// bin and its rows are zeroed here (RPB: the workgroup's weight rows).
template <int RPB, int WGS> __device__ __forceinline__ bool moeb_tile(const MoePlanArgs& a, int tile, MoeTile& t) {
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

// The body's names: the operands of the tile's expert, M = the tile's rows, and the two hooks. srt[m]: the slot of
// position m (positions past the tile's rows take the last one: loaded, never used), read before the weight stream.
#define QG_KQ_DECLARE_TILE  // declared by the kernels below, before the tile lookup
#define QG_KQ_ABLK(g) A + ((long)mt.arows[(g) / nb] * nb + ((g) - (g) / nb * nb)) * 9
#define QG_KQ_OUT(m) C[(long)srt[m] * ldc + row]
#define QG_MOEB_PROLOGUE                                                                          \
    constexpr int RPB_ = (WGS / 64) * (64 / LPR);                                                 \
    const int tile = xcd_tile_x();                                                                \
    MoeTile mt;                                                                                   \
    if (!moeb_tile<RPB_, WGS>(a, tile, mt)) return;                                               \
    const uint32_t* __restrict__ A = static_cast<const uint32_t*>(a.A);                           \
    const uint8_t* __restrict__ B = static_cast<const uint8_t*>(a.B) + (long)mt.e * a.estride;    \
    const int M = mt.rows, N = a.N, K = a.K;                                                      \
    void* __restrict__ out = a.C;                                                                 \
    const long ldc = a.ldc;                                                                       \
    constexpr bool SUMI = false;                                                                  \
    int srt[MT];                                                                                  \
    _Pragma("unroll") for (int m = 0; m < MT; ++m) srt[m] = mt.sorted[min(m, mt.rows - 1)];

template <int MT, int LPR, int WGS, bool ONE> __global__ __launch_bounds__(WGS) void q4k_moeb_kernel(const MoePlanArgs a) {
    QG_MOEB_PROLOGUE
#include "qg_q4k_gemv_body.inc"
}

template <int MT, int LPR, int WGS, bool ONE> __global__ __launch_bounds__(WGS) void q6k_moeb_kernel(const MoePlanArgs a) {
    QG_MOEB_PROLOGUE
#include "qg_q6k_gemv_body.inc"
}
#undef QG_MOEB_PROLOGUE
#undef QG_KQ_OUT
#undef QG_KQ_ABLK
#undef QG_KQ_DECLARE_TILE

// ---- the biased entry (qg_gemm_w4a8_moe_batch_bias): kernels beside the two above, which stay ----------
// MXFP4 alone: Q4_K / Q6_K run the two kernels above as they are and then launch_moe_bias_add (qg_moe_plan.hpp), so each
// K-quant body stays included once in this file. The same prologue and hooks on MoeBiasArgs. The body's last statement is `QG_KQ_OUT(m) = acc[m]`, run by the lane
// that holds the row's reduced sum: here the hook names a MoebOut, whose assignment stores the sum plus the expert's
// bias at the lane's row -- one rounded addition after the reduction (BIAS = false: no load, no pointer test).
template <bool BIAS> struct MoebOut {
    float* c;
    const float* b;
    __device__ __forceinline__ void operator=(float v) const {
        if constexpr (BIAS) *c = v + *b;
        else *c = v;
    }
};
#define QG_KQ_DECLARE_TILE
#define QG_KQ_ABLK(g) A + ((long)mt.arows[(g) / nb] * nb + ((g) - (g) / nb * nb)) * 9
#define QG_KQ_OUT(m) MoebOut<BIAS>{C + (long)srt[m] * ldc + row, BIAS ? bias_e + row : nullptr}
#define QG_MOEB_PROLOGUE                                                                          \
    constexpr int RPB_ = (WGS / 64) * (64 / LPR);                                                 \
    const int tile = xcd_tile_x();                                                                \
    MoeTile mt;                                                                                   \
    if (!moeb_tile<RPB_, WGS>(a, tile, mt)) return;                                               \
    const uint32_t* __restrict__ A = static_cast<const uint32_t*>(a.A);                           \
    const uint8_t* __restrict__ B = static_cast<const uint8_t*>(a.B) + (long)mt.e * a.estride;    \
    const float* __restrict__ bias_e = BIAS ? a.bias + (long)mt.e * a.bias_stride : nullptr;      \
    const int M = mt.rows, N = a.N, K = a.K;                                                      \
    void* __restrict__ out = a.C;                                                                 \
    const long ldc = a.ldc;                                                                       \
    constexpr bool SUMI = false;                                                                  \
    int srt[MT];                                                                                  \
    _Pragma("unroll") for (int m = 0; m < MT; ++m) srt[m] = mt.sorted[min(m, mt.rows - 1)];

// MXFP4: the body of mxfp4_gemv_kernel (qg_mxfp4_gemv.hip) at the LPR, WGS and ONE of the single M = 1 call
// (kq_gemv_form_units(K / 32)); an LDS record is one block. The expert's matrix starts at any byte.
template <int MT, int LPR, int WGS, bool ONE, bool BIAS>
__global__ __launch_bounds__(WGS) void mxfp4_moeb_kernel(const MoeBiasArgs a) {
    QG_MOEB_PROLOGUE
#include "qg_mxfp4_gemv_body.inc"
}
#undef QG_MOEB_PROLOGUE
#undef QG_KQ_OUT
#undef QG_KQ_ABLK
#undef QG_KQ_DECLARE_TILE

// ---- host side ------------------------------------------------------------------------------------------------------
using Launch = MoeLaunch<MoePlanArgs>;

// The plan for tiles of MT rows, then the product at the single M = 1 call's LPR, WGS and ONE (kq_gemv_form,
// qg_kq_launch.hpp), which depend on K alone.
template <int WT, int MT> hipError_t moeb_mt(const Launch& L) {
    return kq_gemv_form(L.a.K, [&](auto lpr, auto wgs, auto one) -> hipError_t {
        constexpr int LPR = lpr, WGS = wgs, RPB = (WGS / 64) * (64 / LPR);
        constexpr bool ONE = one;
        const MoePlanArgs& a = L.a;
        const size_t lds = (size_t)MT * (a.K / SB_ELEMS) * kq_gemv_rec_dw(WT) * 4;
        const int gy = (int)moe_max_tiles(a.slots, a.n_expert, MT);
        if (L.describe) {
            describe_line(L.describe, L.describe_len, "moeb:%s_gemv R=%d LPR=%d WGS=%d ONE=%d grid=%dx%d lds=%zu", kq_family(WT), MT,
                          LPR, WGS, (int)ONE, (a.N + RPB - 1) / RPB, gy, lds);
            return hipSuccess;
        }
        int rsh = 0;
        while ((1 << rsh) < MT) ++rsh;
        const hipError_t e = launch_moe_plan_rows(a, rsh, L.st);
        if (e != hipSuccess) return e;
        auto k = [] {
            if constexpr (WT == QG_TYPE_Q4_K) return q4k_moeb_kernel<MT, LPR, WGS, ONE>;
            else return q6k_moeb_kernel<MT, LPR, WGS, ONE>;
        }();
        static std::atomic<unsigned long long> done;
        return moe_enqueue(k, L, RPB, gy, WGS, lds, done);
    });
}

template <int WT> hipError_t moeb_r(const Launch& L) {
    switch (moe_batch_rows(L.a.slots, L.a.n_expert, L.a.K, WT)) {
        case 2: return moeb_mt<WT, 2>(L);
        case 4: return moeb_mt<WT, 4>(L);
        case 8: return moeb_mt<WT, 8>(L);
    }
    return hipErrorInvalidValue;
}

// The biased entry. Q4_K / Q6_K: the launch of the entry beside it, kernels and all, then the bias add where there is one.
using BiasLaunch = MoeLaunch<MoeBiasArgs>;

template <int WT, int MT> hipError_t moeb_bias_mt(const BiasLaunch& L) {
    const MoeBiasArgs& a = L.a;
    if constexpr (WT != QG_TYPE_MXFP4) {
        const hipError_t e = moeb_mt<WT, MT>(Launch{a, L.st, L.describe, L.describe_len});
        return e != hipSuccess || L.describe || !a.bias ? e : launch_moe_bias_add(a, L.st);
    }
    return kq_gemv_form_units(a.K / QK, [&](auto lpr, auto wgs, auto one) -> hipError_t {
        constexpr int LPR = lpr, WGS = wgs, RPB = (WGS / 64) * (64 / LPR);
        constexpr bool ONE = one;
        const size_t lds = (size_t)MT * moe_batch_row_lds(a.K, WT);
        const int gy = (int)moe_max_tiles(a.slots, a.n_expert, MT);
        if (L.describe) {
            describe_line(L.describe, L.describe_len, "moeb:mxfp4_gemv R=%d LPR=%d WGS=%d ONE=%d grid=%dx%d lds=%zu", MT, LPR, WGS,
                          (int)ONE, (a.N + RPB - 1) / RPB, gy, lds);
            return hipSuccess;
        }
        int rsh = 0;
        while ((1 << rsh) < MT) ++rsh;
        const hipError_t e = launch_moe_plan_rows(a, rsh, L.st);
        if (e != hipSuccess) return e;
        static std::atomic<unsigned long long> done[2];
        if (a.bias) return moe_enqueue(mxfp4_moeb_kernel<MT, LPR, WGS, ONE, true>, L, RPB, gy, WGS, lds, done[0]);
        else return moe_enqueue(mxfp4_moeb_kernel<MT, LPR, WGS, ONE, false>, L, RPB, gy, WGS, lds, done[1]);
    });
}

template <int WT> hipError_t moeb_bias_r(const BiasLaunch& L) {
    switch (moe_batch_rows(L.a.slots, L.a.n_expert, L.a.K, WT)) {
        case 2: return moeb_bias_mt<WT, 2>(L);
        case 4: return moeb_bias_mt<WT, 4>(L);
        case 8: return moeb_bias_mt<WT, 8>(L);
    }
    return hipErrorInvalidValue;
}

}  // namespace

// Bytes of the LDS records of one gathered row: K / 256 super-block records, or K / 32 block records for MXFP4 (48 B).
size_t moe_batch_row_lds(int K, int wtype) {
    if (wtype == QG_TYPE_MXFP4) return (size_t)(K / QK) * MXFP4_REC_DW * 4;
    return (size_t)(K / SB_ELEMS) * kq_gemv_rec_dw(wtype) * 4;
}

// Rows per tile. The expected rows per expert, per = ceil(slots / n_expert), rounded up to the body's MT = 2 / 4 / 8
// (a tile costs one pass over the expert whatever its rows; a larger MT than the rows need only adds registers and LDS),
// then halved until the R records of K / 256 super-blocks fit 160 KiB (Q4_K: R = 8 up to K = 15360, R = 4 up to 30976;
// Q6_K: 17152 and 34304; MXFP4, a 48-B record per block: R = 8 up to K = 13632, R = 4 up to 27296, R = 2 up to 54592).
// The thresholds are these by construction; profiles/moe_batch/README.md says what has been
// measured of them.
int moe_batch_rows(long slots, int n_expert, int K, int wtype) {
    const long per = (slots + n_expert - 1) / n_expert;
    int r = per <= 2 ? 2 : per <= 4 ? 4 : 8;
    const size_t row = moe_batch_row_lds(K, wtype);
    while (r >= MOE_BATCH_MIN_R && r * row > MOE_BATCH_LDS_MAX) r >>= 1;
    return r >= MOE_BATCH_MIN_R ? r : 0;
}

hipError_t launch_moe_batch(const MoePlanArgs& a, int wtype, hipStream_t st, char* describe, size_t describe_len) {
    const Launch L{a, st, describe, describe_len};
    if (wtype == QG_TYPE_Q4_K) return moeb_r<QG_TYPE_Q4_K>(L);
    if (wtype == QG_TYPE_Q6_K) return moeb_r<QG_TYPE_Q6_K>(L);
    return hipErrorInvalidValue;
}

hipError_t launch_moe_batch_bias(const MoeBiasArgs& a, int wtype, hipStream_t st, char* describe, size_t describe_len) {
    const BiasLaunch L{a, st, describe, describe_len};
    if (wtype == QG_TYPE_Q4_K) return moeb_bias_r<QG_TYPE_Q4_K>(L);
    if (wtype == QG_TYPE_Q6_K) return moeb_bias_r<QG_TYPE_Q6_K>(L);
    if (wtype == QG_TYPE_MXFP4) return moeb_bias_r<QG_TYPE_MXFP4>(L);
    return hipErrorInvalidValue;
}

}  // namespace qg
