// qg_moe_down.hip — the down mul_mat_id with the weighted expert sum (qg_gemm_w4a8_moe_down), families
// "moe_down:q4k_gemv", "moe_down:q6k_gemv": the second half of an MoE FFN block, sum_u w[t,u] * down_e(h[t,u]), in
// one launch.
//
// The grid is (row tiles x tokens): blockIdx.y is the token t, xcd_tile_x() its row tile. The workgroup has the
// decode GEMV's LPR, WGS and ONE for this K (kq_gemv_form), but its W = WGS / 64 waves are split: SW of them stand
// side by side on the slots of one row group, RW = W / SW row groups of 64 / LPR rows each make the workgroup's
// RPB = RW * 64 / LPR rows. So a token's n_used slots run in as many waves as the unfused launch gives them, not one
// after another in one workgroup.
//   1. The whole workgroup stages the token's n_used activation rows (contiguous: the body's own prologue at M = n_used,
//      the QG_KQ_STAGE_ONLY inclusion) into the LDS records; the prologue's barrier.
//   2. Wave w owns row group w / SW and the slots u = w % SW, + SW, ...: per slot one scalar load of the id, a
//      wave-uniform skip of an id outside [0, n_expert) before any weight address is formed, otherwise the decode GEMV
//      body (the very text, QG_KQ_A_STAGED on the records of row u) on expert e; the lane that holds the reduced sum
//      writes d_u into part[u][row], an LDS array behind the records.
//   3. One barrier, then the first RPB threads fold u = 0 .. n_used - 1 in ascending order, acc = acc + w * d_u, each
//      operation one rounded fp32 operation, out-of-range ids left out (neither their weight nor their part is read).
// d_u's bits depend on LPR and ONE alone (which wave owns a row does not enter a row's arithmetic), so they are those of
// qg_gemm_w4a8_moe at a_rows = n_used.
// Both barriers stand in workgroup-uniform code: none inside the per-slot loop, whose trip count differs between waves
// where SW does not divide n_used, and none under a branch on an id.
// The arguments travel by value (no device allocation, capture-safe); the host reads neither ids nor weights.
// qg_gemm_w4a8_moe_down_bias (the same with a per-expert bias row added to d_u and MXFP4 experts, family
// "moe_down:mxfp4_gemv" beside the two above) is kq_moe_down_bias_kernel below: the same structure in a kernel of its own.
#include "../../include/qg/qg.h"
#include "qg_kq_launch.hpp"
#include "qg_moe_down.hpp"
#include "qg_q4k.hpp"
#include "qg_q6k.hpp"

namespace qg {

// The body's staging prologue alone: M dense activation rows from A into the records at the start of the dynamic LDS,
// and its barrier.
#define QG_KQ_ABLK(g) A + (long)g * 9
#define QG_KQ_STAGE_ONLY
template <int LPR, int WGS> __device__ __forceinline__ void q4k_down_stage(const uint32_t* __restrict__ A, int M, int K) {
#include "qg_q4k_gemv_body.inc"
    (void)RPB; (void)U; (void)lir;
}

template <int LPR, int WGS> __device__ __forceinline__ void q6k_down_stage(const uint32_t* __restrict__ A, int M, int K) {
#include "qg_q6k_gemv_body.inc"
    (void)RPB; (void)U; (void)lir;
}

// MXFP4 (qg_gemm_w4a8_moe_down_bias alone): a record per block, row m's at m * K/32 records.
template <int LPR, int WGS> __device__ __forceinline__ void mxfp4_down_stage(const uint32_t* __restrict__ A, int M, int K) {
#include "qg_mxfp4_gemv_body.inc"
    (void)RPB; (void)U; (void)lir;
}
#undef QG_KQ_STAGE_ONLY
#undef QG_KQ_ABLK

// One decode GEMV product of the staged activation row whose records start at recs with the matrix B, at this lane's
// row, returned in the lane that holds the row's reduced sum (row < N and lane % LPR == LPR - 1; 0.0f in every other
// lane): the body's four constants as the single call passes them at M = 1.
#define QG_KQ_A_STAGED
#define QG_KQ_ROW ((void)RPB, lane_row)
#define QG_KQ_RECS recs
#define QG_KQ_OUT(m) (*((void)C, &res))
template <int LPR, int WGS, bool ONE>
__device__ __forceinline__ float q4k_down_product(const uint32_t* recs, const uint8_t* __restrict__ B, int N, int K,
                                                  const int lane_row) {
    constexpr int MT = 1, M = 1;
    constexpr bool SUMI = false;
    void* const out = nullptr;
    float res = 0.0f;
#include "qg_q4k_gemv_body.inc"
    return res;
}

template <int LPR, int WGS, bool ONE>
__device__ __forceinline__ float q6k_down_product(const uint32_t* recs, const uint8_t* __restrict__ B, int N, int K,
                                                  const int lane_row) {
    constexpr int MT = 1, M = 1;
    constexpr bool SUMI = false;
    void* const out = nullptr;
    float res = 0.0f;
#include "qg_q6k_gemv_body.inc"
    return res;
}

template <int LPR, int WGS, bool ONE>
__device__ __forceinline__ float mxfp4_down_product(const uint32_t* recs, const uint8_t* __restrict__ B, int N, int K,
                                                    const int lane_row) {
    constexpr int MT = 1, M = 1;
    constexpr bool SUMI = false;
    void* const out = nullptr;
    float res = 0.0f;
#include "qg_mxfp4_gemv_body.inc"
    return res;
}
#undef QG_KQ_OUT
#undef QG_KQ_RECS
#undef QG_KQ_ROW
#undef QG_KQ_A_STAGED

namespace {

// SW = 1 << SWSH waves per row group.
template <int WT, int LPR, int WGS, bool ONE, int SWSH>
__global__ __launch_bounds__(WGS) void kq_moe_down_kernel(const MoeDownArgs a) {
    constexpr int W = WGS / 64, SW = 1 << SWSH, RW = W / SW, RPW = 64 / LPR, RPB = RW * RPW;
    constexpr int REC_DW = kq_gemv_rec_dw(WT);
    static_assert(SW >= 1 && SW <= W && RW * SW == W, "the waves of a workgroup: RW row groups of SW");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tile = xcd_tile_x();
    const int t = blockIdx.y;
    const int nsb = a.K / SB_ELEMS;
    const uint32_t* A = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(a.A) + (long)t * a.n_used * a.arow);
    if constexpr (WT == QG_TYPE_Q4_K) q4k_down_stage<LPR, WGS>(A, a.n_used, a.K);
    else q6k_down_stage<LPR, WGS>(A, a.n_used, a.K);  // (ends in the prologue's barrier)

    float* part = reinterpret_cast<float*>(lds + (long)a.n_used * nsb * REC_DW);  // [n_used][RPB]
    const int32_t* ids = a.ids + (long)t * a.ids_stride;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int local = (wave >> SWSH) * RPW + lane / LPR;  // this lane's row within the workgroup's RPB
    const int row = tile * RPB + local;
    for (int u = wave & (SW - 1); u < a.n_used; u += SW) {  // (no barrier in here: the trip count is the wave's own)
        const int e = ids[u];
        if ((unsigned)e >= (unsigned)a.n_expert) continue;
        const uint8_t* B = static_cast<const uint8_t*>(a.B) + (long)e * a.estride;
        const uint32_t* recs = lds + u * nsb * REC_DW;
        float d;
        if constexpr (WT == QG_TYPE_Q4_K) d = q4k_down_product<LPR, WGS, ONE>(recs, B, a.N, a.K, row);
        else d = q6k_down_product<LPR, WGS, ONE>(recs, B, a.N, a.K, row);
        if (row < a.N && lane % LPR == LPR - 1) part[u * RPB + local] = d;
    }
    __syncthreads();
    const int frow = tile * RPB + tid;
    if (tid < RPB && frow < a.N) {
        const float* w = a.weights ? a.weights + (long)t * a.w_stride : nullptr;
        float acc = 0.0f;
        for (int u = 0; u < a.n_used; ++u) {
            if ((unsigned)ids[u] >= (unsigned)a.n_expert) continue;
            acc = acc + (w ? w[u] : 1.0f) * part[u * RPB + tid];
        }
        a.C[(long)t * a.ldc + frow] = acc;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------
// SWSH: log2 of the largest power of two <= min(n_used, W)
int moe_down_swsh(int n_used, int W) {
    int sh = 0;
    while ((2 << sh) <= n_used && (2 << sh) <= W) ++sh;
    return sh;
}

template <int WT, int LPR, int WGS, bool ONE, int SWSH> hipError_t moe_down_k(const MoeLaunch<MoeDownArgs>& L) {
    constexpr int RPB = (WGS / 64 >> SWSH) * (64 / LPR);
    const size_t lds = moe_down_form(L.a.n_used, L.a.K, WT).lds;
    if (L.describe) {
        describe_line(L.describe, L.describe_len, "moe_down:%s_gemv LPR=%d WGS=%d ONE=%d SW=%d grid=%dx%d lds=%zu", kq_family(WT),
                      LPR, WGS, (int)ONE, 1 << SWSH, (L.a.N + RPB - 1) / RPB, L.a.T, lds);
        return hipSuccess;
    }
    static std::atomic<unsigned long long> done;
    return moe_enqueue(kq_moe_down_kernel<WT, LPR, WGS, ONE, SWSH>, L, RPB, L.a.T, WGS, lds, done);
}

template <int WT> hipError_t moe_down_launch_t(const MoeLaunch<MoeDownArgs>& L) {
    return kq_gemv_form(L.a.K, [&](auto lpr, auto wgs, auto one) -> hipError_t {
        constexpr int LPR = lpr, WGS = wgs, W = WGS / 64;
        switch (moe_down_swsh(L.a.n_used, W)) {
            case 0: return moe_down_k<WT, LPR, WGS, one, 0>(L);
            case 1: return moe_down_k<WT, LPR, WGS, one, 1>(L);
            case 2: return moe_down_k<WT, LPR, WGS, one, 2>(L);
            case 3:
                if constexpr (W >= 8) return moe_down_k<WT, LPR, WGS, one, 3>(L);
                break;
            case 4:
                if constexpr (W >= 16) return moe_down_k<WT, LPR, WGS, one, 4>(L);
                break;
        }
        return hipErrorInvalidValue;
    });
}

// ---- qg_gemm_w4a8_moe_down_bias: kernel and host side ---------------------------------------------------------
// The records of one activation row in dwords: K/256 super-block records, or K/32 block records for MXFP4.
template <int WT> __host__ __device__ constexpr int down_row_dw(int K) {
    return WT == QG_TYPE_MXFP4 ? (K / QK) * MXFP4_REC_DW : (K / SB_ELEMS) * kq_gemv_rec_dw(WT);
}

// The kernel above (its three steps, its barriers) for Q4_K / Q6_K / MXFP4 with the per-expert bias row: a kernel of
// its own, so that kq_moe_down_kernel keeps its argument block and its code. BIAS: the bias pointer is non-null; the
// lane that holds d_u writes d_u + bias[e_u][row] into part, and the fold is the one above.
template <int WT, int LPR, int WGS, bool ONE, int SWSH, bool BIAS>
__global__ __launch_bounds__(WGS) void kq_moe_down_bias_kernel(const MoeDownBiasArgs a) {
    constexpr int W = WGS / 64, SW = 1 << SWSH, RW = W / SW, RPW = 64 / LPR, RPB = RW * RPW;
    static_assert(SW >= 1 && SW <= W && RW * SW == W, "the waves of a workgroup: RW row groups of SW");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const int tile = xcd_tile_x();
    const int t = blockIdx.y;
    const int row_dw = down_row_dw<WT>(a.K);
    const uint32_t* A = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(a.A) + (long)t * a.n_used * a.arow);
    if constexpr (WT == QG_TYPE_Q4_K) q4k_down_stage<LPR, WGS>(A, a.n_used, a.K);
    else if constexpr (WT == QG_TYPE_MXFP4) mxfp4_down_stage<LPR, WGS>(A, a.n_used, a.K);
    else q6k_down_stage<LPR, WGS>(A, a.n_used, a.K);  // (ends in the prologue's barrier)

    float* part = reinterpret_cast<float*>(lds + (long)a.n_used * row_dw);  // [n_used][RPB]
    const int32_t* ids = a.ids + (long)t * a.ids_stride;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int local = (wave >> SWSH) * RPW + lane / LPR;  // this lane's row within the workgroup's RPB
    const int row = tile * RPB + local;
    const bool holder = row < a.N && lane % LPR == LPR - 1;
    for (int u = wave & (SW - 1); u < a.n_used; u += SW) {  // (no barrier in here: the trip count is the wave's own)
        const int e = ids[u];
        if ((unsigned)e >= (unsigned)a.n_expert) continue;
        float b = 0.0f;
        if constexpr (BIAS) {
            if (holder) b = a.bias[(long)e * a.bias_stride + row];
        }
        const uint8_t* B = static_cast<const uint8_t*>(a.B) + (long)e * a.estride;
        const uint32_t* recs = lds + u * row_dw;
        float d;
        if constexpr (WT == QG_TYPE_Q4_K) d = q4k_down_product<LPR, WGS, ONE>(recs, B, a.N, a.K, row);
        else if constexpr (WT == QG_TYPE_MXFP4) d = mxfp4_down_product<LPR, WGS, ONE>(recs, B, a.N, a.K, row);
        else d = q6k_down_product<LPR, WGS, ONE>(recs, B, a.N, a.K, row);
        if constexpr (BIAS) d = d + b;
        if (holder) part[u * RPB + local] = d;
    }
    __syncthreads();
    const int frow = tile * RPB + tid;
    if (tid < RPB && frow < a.N) {
        const float* w = a.weights ? a.weights + (long)t * a.w_stride : nullptr;
        float acc = 0.0f;
        for (int u = 0; u < a.n_used; ++u) {
            if ((unsigned)ids[u] >= (unsigned)a.n_expert) continue;
            acc = acc + (w ? w[u] : 1.0f) * part[u * RPB + tid];
        }
        a.C[(long)t * a.ldc + frow] = acc;
    }
}

// the units of a row that pick the decode GEMV's form: K / 64, or MXFP4's blocks (moe_kq_launch, qg_moe.hip)
int down_units(int K, int wtype) { return wtype == QG_TYPE_MXFP4 ? (K / QK + MXFP4_UB - 1) / MXFP4_UB : K / 64; }

template <int WT, int LPR, int WGS, bool ONE, int SWSH> hipError_t moe_down_bias_k(const MoeLaunch<MoeDownBiasArgs>& L) {
    constexpr int RPB = (WGS / 64 >> SWSH) * (64 / LPR);
    const size_t lds = moe_down_form(L.a.n_used, L.a.K, WT).lds;
    if (L.describe) {
        describe_line(L.describe, L.describe_len, "moe_down:%s_gemv LPR=%d WGS=%d ONE=%d SW=%d grid=%dx%d lds=%zu",
                      WT == QG_TYPE_MXFP4 ? "mxfp4" : kq_family(WT), LPR, WGS, (int)ONE, 1 << SWSH, (L.a.N + RPB - 1) / RPB, L.a.T, lds);
        return hipSuccess;
    }
    static std::atomic<unsigned long long> done_bias, done_plain;
    if (L.a.bias) return moe_enqueue(kq_moe_down_bias_kernel<WT, LPR, WGS, ONE, SWSH, true>, L, RPB, L.a.T, WGS, lds, done_bias);
    return moe_enqueue(kq_moe_down_bias_kernel<WT, LPR, WGS, ONE, SWSH, false>, L, RPB, L.a.T, WGS, lds, done_plain);
}

template <int WT> hipError_t moe_down_bias_launch_t(const MoeLaunch<MoeDownBiasArgs>& L) {
    return kq_gemv_form_units(down_units(L.a.K, WT), [&](auto lpr, auto wgs, auto one) -> hipError_t {
        constexpr int LPR = lpr, WGS = wgs, W = WGS / 64;
        switch (moe_down_swsh(L.a.n_used, W)) {
            case 0: return moe_down_bias_k<WT, LPR, WGS, one, 0>(L);
            case 1: return moe_down_bias_k<WT, LPR, WGS, one, 1>(L);
            case 2: return moe_down_bias_k<WT, LPR, WGS, one, 2>(L);
            case 3:
                if constexpr (W >= 8) return moe_down_bias_k<WT, LPR, WGS, one, 3>(L);
                break;
            case 4:
                if constexpr (W >= 16) return moe_down_bias_k<WT, LPR, WGS, one, 4>(L);
                break;
        }
        return hipErrorInvalidValue;
    });
}

}  // namespace

MoeDownForm moe_down_form(int n_used, int K, int wtype) {
    return kq_gemv_form_units(down_units(K, wtype), [&](auto lpr, auto wgs, auto one) -> MoeDownForm {
        constexpr int LPR = lpr, WGS = wgs, W = WGS / 64;
        const int sh = moe_down_swsh(n_used, W);
        MoeDownForm f{LPR, WGS, (int)one, 1 << sh, (W >> sh) * (64 / LPR), SIZE_MAX};
        const size_t row = wtype == QG_TYPE_MXFP4 ? (size_t)down_row_dw<QG_TYPE_MXFP4>(K) * 4
                                                  : (size_t)(K / SB_ELEMS) * kq_gemv_rec_dw(wtype) * 4;
        if (n_used >= 0 && (size_t)n_used <= MAX_LDS_BYTES / 4) f.lds = (size_t)n_used * (row + (size_t)f.rpb * 4);
        return f;
    });
}

hipError_t launch_moe_down_bias(const MoeDownBiasArgs& a, int wtype, hipStream_t st, char* describe, size_t describe_len) {
    const MoeLaunch<MoeDownBiasArgs> L{a, st, describe, describe_len};
    switch (wtype) {
        case QG_TYPE_Q4_K: return moe_down_bias_launch_t<QG_TYPE_Q4_K>(L);
        case QG_TYPE_Q6_K: return moe_down_bias_launch_t<QG_TYPE_Q6_K>(L);
        case QG_TYPE_MXFP4: return moe_down_bias_launch_t<QG_TYPE_MXFP4>(L);
    }
    return hipErrorInvalidValue;
}

hipError_t launch_moe_down(const MoeDownArgs& a, int wtype, hipStream_t st, char* describe, size_t describe_len) {
    const MoeLaunch<MoeDownArgs> L{a, st, describe, describe_len};
    switch (wtype) {
        case QG_TYPE_Q4_K: return moe_down_launch_t<QG_TYPE_Q4_K>(L);
        case QG_TYPE_Q6_K: return moe_down_launch_t<QG_TYPE_Q6_K>(L);
    }
    return hipErrorInvalidValue;
}

}  // namespace qg
