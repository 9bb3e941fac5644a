// qg_kq_f32.hip — the Q4_K / Q6_K decode GEMV on FP32 rows (qg_gemm_w4a8_f32_kq), families "q4k_gemv_f32", "q6k_gemv_f32".
//
// C[M][N] = quantize_q8_1(X[M][K]) . B[N][K]^T in ONE launch and without a workspace: the workgroup quantizes the M
// rows to Q8_1 itself, straight into the LDS records the single call's GEMV (qg_q4k_gemv.hip, qg_q6k_gemv.hip) builds
// from Q8_1 blocks, and then runs that GEMV's product. The product is the same text (qg_q4k_gemv_body.inc,
// qg_q6k_gemv_body.inc) at the single call's (MT, LPR, WGS, ONE) — kq_gemv_form and the M ladder of kq_gemv_launch_m —
// and the records are byte for byte the ones put_ablk writes from qg_quantize_q8_1's blocks (below), so every output
// has the bits of qg_quantize_q8_1 followed by qg_gemm_w4a8.
//
// The staging split is the standalone quantizer's (q8_1_lanes, qg_quant_block.hpp), not the row GEMV's "one thread
// quantizes a whole block":
//  * Eight lanes per 32-element block. Float4 gi = tid + r * WGS of the dense rows belongs to block g = gi / 8 =
//    m * K/32 + b, lane j = gi % 8 = tid % 8 (WGS is a multiple of 8): one 16-B load per lane, 1 KB contiguous per wave
//    instruction. At M = 1, K = 4096 all 1024 threads quantize at once (128 blocks x 8 lanes); a thread per block
//    would use 128 of them for 32 elements each.
//  * amax over the 8 lanes is three DPP steps, s = sum(x) in element order the row_shr:1 chain, d = amax / 127 and the
//    rounding are q8_1_lanes's: the bytes of qg_quantize_q8_1 (variant 0).
//  * Lane j writes its packed qs dword into slot (b % 8) * 8 + j of the record of (m, b / 8); lane 7, which ends up
//    with the header, writes the fp32 values of the f16-rounded d_a (and, for Q4_K, s_a) behind the 64 qs dwords:
//    h2f of the header's halves, exactly what put_ablk stores from a Q8_1 block's first dword.
//  * WGS / 8 blocks per round; more go round a loop whose trip count is the same for the whole workgroup. All 64
//    lanes of a wave run every DPP step of every round (the rule q8_1_lanes states); only the loads and the LDS writes
//    are predicated, which is what the last round needs where it lies partly past M * K / 32. The next round's float4
//    is in flight while the current one is quantized.
//  * The weight stream starts before the quantizer: each lane's first float4 load, then the lane's first weight unit
//    (the body's load_unit), then the quantizer's ALU work and the record writes, then the barrier. The bodies take
//    the prologue through the hook pair QG_KQ_ROWS_LOAD / QG_KQ_ROWS_PUT, which no other includer defines.
// Every workgroup quantizes all M rows again (from L2 after the first): M * K * 4 bytes of FP32 against M * K / 32 * 36
// of Q8_1. DESIGN.md 3q has the measurements and where the two-call sequence stays ahead.
#include "qg_kq_f32.hpp"

#include "qg_kq_launch.hpp"
#include "qg_q4k.hpp"
#include "qg_q6k.hpp"
#include "qg_quant_block.hpp"

namespace qg {
namespace {

// Block g = m * nb + b by its 8 lanes, v this lane's four elements: quantized, into the record of (m, b / 8). Every lane of
// the wave runs the DPP steps, whether its block exists (g < totb) or not; the LDS writes alone are predicated.
template <int WT>
__device__ __forceinline__ void kq_f32_put(const float4 v, int g, int j, uint32_t* lds, int totb, int nb, int nsb) {
    constexpr int REC_DW = kq_gemv_rec_dw(WT);
    uint32_t hdr;
    const uint32_t qd = q8_1_lanes<0>(v, j, hdr);
#if QG_Q6K_ASUM
    // 32 x the exact sums of the block's first and last 16 bytes: lanes 0..3 and 4..7, both into lane 7
    int a1 = __builtin_amdgcn_sdot4(0x20202020, (int)qd, 0, false);
    a1 += __builtin_amdgcn_update_dpp(0, a1, 0xB1, 0xF, 0xF, false);
    a1 += __builtin_amdgcn_update_dpp(0, a1, 0x4E, 0xF, 0xF, false);
    const int a0 = __builtin_amdgcn_update_dpp(0, a1, 0x114, 0xF, 0xF, false);  // row_shr:4
#endif
    if (g >= totb) return;
    const int m = g / nb, b = g - m * nb;
    uint32_t* rec = lds + (m * nsb + (b >> 3)) * REC_DW;
    rec[(b & 7) * 8 + j] = qd;
    if (j != 7) return;
    if constexpr (WT == QG_TYPE_Q4_K) {
        *reinterpret_cast<uint2*>(rec + 64 + (b & 7) * 2) =
            make_uint2(__float_as_uint(h2f(hdr & 0xFFFFu)), __float_as_uint(h2f(hdr >> 16)));
    } else {
        rec[64 + (b & 7)] = __float_as_uint(h2f(hdr & 0xFFFFu));
#if QG_Q6K_ASUM
        *reinterpret_cast<uint2*>(rec + 72 + 2 * (b & 7)) = make_uint2((uint32_t)a0, (uint32_t)a1);
#endif
    }
}

// The M rows into the records of type WT, WGS / 8 blocks per round. v: this thread's float4 of the first round (zero past
// the rows), loaded ahead of the weight unit. The first round stands outside the loop so that its wait is for v alone and
// not, as at a loop's head, for every load in flight: the quantizer's ALU work runs under the weight unit's latency.
template <int WT, int WGS>
__device__ __forceinline__ void kq_f32_stage(const float4* __restrict__ X, float4 v, uint32_t* lds, int totb, int nb, int nsb,
                                             int tid) {
    constexpr int BPR = WGS / 8;
    const int j = tid & 7;
    const int rounds = (totb + BPR - 1) / BPR;  // uniform over the workgroup
    auto load = [&](int g) { return g < totb ? X[g * 8 + j] : make_float4(0.f, 0.f, 0.f, 0.f); };
    int g = tid >> 3;
    float4 nxt = load(g + BPR);
    kq_f32_put<WT>(v, g, j, lds, totb, nb, nsb);
    for (int r = 1; r < rounds; ++r) {
        g += BPR;
        v = nxt;
        nxt = load(g + BPR);
        kq_f32_put<WT>(v, g, j, lds, totb, nb, nsb);
    }
}

// The shipped bodies with the quantizing prologue in place of the copy of Q8_1 blocks.
#define QG_KQ_DECLARE_TILE const int tile = gridDim.x <= 512 ? xcd_tile(blockIdx.x, gridDim.x) : (int)blockIdx.x;
#define QG_KQ_OUT(m) C[m * ldc + row]
#define QG_KQ_ROWS_LOAD const float4 x0 = tid < totb * 8 ? X[tid] : make_float4(0.f, 0.f, 0.f, 0.f);
#define QG_KQ_ROWS_PUT kq_f32_stage<WT, WGS>(X, x0, lds, totb, nb, nsb, tid);
template <int MT, int LPR, int WGS, bool ONE>
__device__ __forceinline__ void q4k_f32_body(const float4* __restrict__ X, const uint8_t* __restrict__ B, int M, int N, int K,
                                             void* __restrict__ out, const long ldc) {
    constexpr bool SUMI = false;
    constexpr int WT = QG_TYPE_Q4_K;
#include "qg_q4k_gemv_body.inc"
}

template <int MT, int LPR, int WGS, bool ONE>
__device__ __forceinline__ void q6k_f32_body(const float4* __restrict__ X, const uint8_t* __restrict__ B, int M, int N, int K,
                                             void* __restrict__ out, const long ldc) {
    constexpr bool SUMI = false;
    constexpr int WT = QG_TYPE_Q6_K;
#include "qg_q6k_gemv_body.inc"
}
#undef QG_KQ_ROWS_PUT
#undef QG_KQ_ROWS_LOAD
#undef QG_KQ_OUT
#undef QG_KQ_DECLARE_TILE

// Argument order: everything (9 dwords) is preloaded into SGPRs by the dispatch (csrc/Makefile).
template <int WT, int MT, int LPR, int WGS, bool ONE>
__global__ __launch_bounds__(WGS) void kq_f32_kernel(const float4* __restrict__ X, const uint8_t* __restrict__ B, int M, int N,
                                                    int K, float* __restrict__ C) {
    if constexpr (WT == QG_TYPE_Q4_K) q4k_f32_body<MT, LPR, WGS, ONE>(X, B, M, N, K, C, N);
    else q6k_f32_body<MT, LPR, WGS, ONE>(X, B, M, N, K, C, N);
}

// ---- host side -----------------------------------------------------------------------------------------------
struct KqF32Launch {
    const KqF32Args& a;
    hipStream_t st;
    char* describe;
    size_t describe_len;
};

template <int WT, int MT> hipError_t kq_f32_form(const KqF32Launch& L) {
    const KqF32Args& a = L.a;
    // (LPR, WGS, ONE) of the single call: both types have K / 64 units per row
    return kq_gemv_form(a.K, [&](auto lpr, auto wgs, auto one) -> hipError_t {
        constexpr int LPR = lpr, WGS = wgs, RPB = (WGS / 64) * (64 / LPR);
        const size_t lds = kq_f32_lds_bytes(a.M, a.K, WT);
        const int grid = (a.N + RPB - 1) / RPB;
        if (L.describe) {
            describe_line(L.describe, L.describe_len, "%s_gemv_f32 MT=%d LPR=%d WGS=%d ONE=%d grid=%d lds=%zu", kq_family(WT), MT,
                          LPR, WGS, (int)one, grid, lds);
            return hipSuccess;
        }
        auto k = kq_f32_kernel<WT, MT, LPR, WGS, one>;
        static std::atomic<unsigned long long> done;
        const hipError_t e = lds_opt_in((const void*)k, lds, done);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k, dim3(grid), dim3(WGS), lds, L.st, reinterpret_cast<const float4*>(a.X), (const uint8_t*)a.B, a.M,
                           a.N, a.K, a.C);
        return hipGetLastError();
    });
}

// MT from M, as kq_gemv_launch_m picks it
template <int WT> hipError_t kq_f32_m(const KqF32Launch& L) {
    if (L.a.M <= 1) return kq_f32_form<WT, 1>(L);
    if (L.a.M <= 2) return kq_f32_form<WT, 2>(L);
    if (L.a.M <= 4) return kq_f32_form<WT, 4>(L);
    return kq_f32_form<WT, 8>(L);
}

}  // namespace

hipError_t launch_kq_f32(const KqF32Args& a, hipStream_t st, char* describe, size_t describe_len) {
    if (a.M < 1 || a.M > 8 || a.N < 1 || a.K <= 0 || a.K % 256 != 0 || kq_f32_lds_bytes(a.M, a.K, a.wtype) > MAX_LDS_BYTES)
        return hipErrorInvalidValue;
    const KqF32Launch L{a, st, describe, describe_len};
    if (a.wtype == QG_TYPE_Q4_K) return kq_f32_m<QG_TYPE_Q4_K>(L);
    if (a.wtype == QG_TYPE_Q6_K) return kq_f32_m<QG_TYPE_Q6_K>(L);
    return hipErrorInvalidValue;
}

}  // namespace qg
