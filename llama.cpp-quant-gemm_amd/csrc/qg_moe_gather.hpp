// qg_moe_gather.hpp — the gathered activation tile of the expert-grouped MFMA kernels: the workgroup's shape, the rows a
// lane loads, the tile's way through registers into LDS, and the tile of the invalid bin. What qg_moe_prefill.hip
// (q4k_moe_mmq_kernel, q6k_moe_mmq_kernel, mxfp4_moe_mmq_kernel) and qg_moe_glu_prefill.hip (moe_glu_mmq_kernel) share.
#pragma once
#include "qg_moe_plan.hpp"
#include "qg_q4k.hpp"
#include "qg_q6k.hpp"

namespace qg {

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

}  // namespace qg
