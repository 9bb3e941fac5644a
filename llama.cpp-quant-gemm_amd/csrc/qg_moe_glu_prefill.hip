// qg_moe_glu_prefill.hip — the expert-grouped MFMA gate / up product with its GLU (qg_gemm_w4a8_moe_glu_prefill),
// families "moe_glu:q4k_mmq" and "moe_glu:q6k_mmq": act(gate(x)) * up(x) of an MoE FFN block at prompt sizes, the
// function of qg_gemm_w4a8_moe_glu at the sizes of qg_gemm_w4a8_moe_prefill. DESIGN.md 3n.
//
// Two launches on the caller's stream, no allocation, no synchronisation, the host never reads ids:
//  1. moe_plan_kernel (qg_moe_plan.hip), once: the plan of qg_gemm_w4a8_moe_prefill, tiles of R = 16 TT rows.
//  2. moe_glu_mmq_kernel<S, TT, RG>, S the type's weight side (Q4KSide, Q6KSide below). The workgroup, its tile of
//     gathered rows, the K slices and the staging are those of q4k_moe_mmq_kernel / q6k_moe_mmq_kernel
//     (qg_moe_prefill.hip, qg_moe_gather.hpp). The K loop is this file's own:
//       * a step stages one 16-token activation tile (one barrier), and every block of it meets the gate weights and
//         the up weights from that one LDS tile: the B operand and the block's (d_a, s_a) are read once, two MFMA
//         results go into two accumulator sets, acc_g and acc_u.
//       * a lane's operand row and header rows are the same rows of both experts' matrices: one set of row offsets,
//         two uniform bases B_gate + e * estride and B_up + e * estride (64 bits).
//       * ahead of the barrier of a super-block's last step the next activation tile and both matrices' next
//         super-block are in flight.
//       * per matrix, the loads, the decode of a super-block and a block's fma chain restate qg_q4k_mmq_body.inc /
//         qg_q6k_mmq_body.inc expression by expression (the library is built with -ffp-contract=off), so g and u have
//         the bits of qg_gemm_w4a8_moe_prefill at the same RG on that tensor.
//     The epilogue reduces the K-slice partials through LDS in slice order, one product after the other in the one
//     W * TT * 256-float region: the gate sums wait in registers (RG TT / 2 per thread, at least 1) while the up
//     partials take the region, and the thread that then holds an output's g and u applies the op and stores it.
//     Neither g nor u is written to memory.
#include "../../include/qg/qg.h"
#include "qg_kq_launch.hpp"
#include "qg_moe_gather.hpp"
#include "qg_moe_glu_prefill.hpp"

namespace qg {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

// ---- the weight side of one matrix, per type -----------------------------------------------------------------------
// For MFMA lane (r16, q): oq is the byte offset of its operand row (row n0 + r16) from the expert's base, oh[e] those
// of the result lane's rows n0 + 4q + e, all clamped at N - 1. Raw: a super-block as loaded; Dec: as the blocks use it.
// block<j>: block j of the staged token (bfr its 8 codes of this lane, ds its d_a | s_a << 16) into acc[4].

struct Q4KSide {  // qg_q4k_mmq_body.inc: 8-byte operand loads, 16-B headers
    static constexpr int WT = QG_TYPE_Q4_K, BYTES = Q4K_BYTES;
    struct Raw {
        uint2 qs[4];
        uint4 hd[4];
    };
    struct Dec {
        long afr[8];
        q4k_scales s[4];
        float d[4], dmin[4];
    };
    static __device__ __forceinline__ void load(Raw& w, const uint8_t* B, long oq, const long (&oh)[4], int sb, int q) {
        const uint8_t* wq = B + oq + (long)sb * Q4K_BYTES + 16 + 8 * q;
#pragma unroll
        for (int i = 0; i < 4; ++i) w.qs[i] = *reinterpret_cast<const uint2*>(wq + 32 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) w.hd[e] = *reinterpret_cast<const uint4*>(B + oh[e] + (long)sb * Q4K_BYTES);
    }
    static __device__ __forceinline__ void decode(Dec& x, const Raw& w, const uint8_t*, long, const long (&)[4], int) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint2 v = w.qs[i];
            const uint32_t l0 = v.x & 0x0F0F0F0Fu, l1 = v.y & 0x0F0F0F0Fu;
            const uint32_t h0 = (v.x >> 4) & 0x0F0F0F0Fu, h1 = (v.y >> 4) & 0x0F0F0F0Fu;
            x.afr[2 * i] = (long)(((unsigned long)l1 << 32) | l0);
            x.afr[2 * i + 1] = (long)(((unsigned long)h1 << 32) | h0);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            x.s[e] = q4k_unpack_scales(w.hd[e].y, w.hd[e].z, w.hd[e].w);
            x.d[e] = h2f(w.hd[e].x & 0xFFFFu);
            x.dmin[e] = h2f(w.hd[e].x >> 16);
        }
    }
    template <int j> static __device__ __forceinline__ void block(const Dec& x, long bfr, uint32_t ds, int, float (&acc)[4]) {
        const v4i zero = {0, 0, 0, 0};
        const v4i c = __builtin_amdgcn_mfma_i32_16x16x32_i8(x.afr[j], bfr, zero, 0, 0, 0);
        const float da = h2f(ds & 0xFFFFu), sa = h2f(ds >> 16);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float dsc = x.d[e] * (float)q4k_byte<j>(x.s[e].sc);
            const float dm = -(x.dmin[e] * (float)q4k_byte<j>(x.s[e].mn));
            acc[e] = __builtin_fmaf(dsc * da, (float)c[e], acc[e]);
            acc[e] = __builtin_fmaf(dm, sa, acc[e]);
        }
    }
};

struct Q6KSide {  // qg_q6k_mmq_body.inc: the realigned q6k_load spans, two half-zeroed MFMAs per block
    static constexpr int WT = QG_TYPE_Q6_K, BYTES = Q6K_BYTES;
    struct Raw {
        uint32_t ql[4][3];  // 8 bytes at 32 i + 8q of ql (+ the realignment dword)
        uint32_t qh[2][3];  // 8 bytes at 32 h + 8q of qh
        uint32_t hd[4][5];  // scales[16] and d of the result lane's four rows
    };
    struct Dec {
        uint32_t cl[8][2];  // the signed codes of blocks 0..7, this lane's 8 elements
        uint32_t sc[4][4];
        float d[4];
    };
    static __device__ __forceinline__ void load(Raw& w, const uint8_t* B, long oq, const long (&oh)[4], int sb, int q) {
        const uint8_t* sbp = B + oq + (long)sb * Q6K_BYTES + 8 * q;
#pragma unroll
        for (int i = 0; i < 4; ++i) q6k_load<2>(sbp + 32 * i, w.ql[i]);
#pragma unroll
        for (int h = 0; h < 2; ++h) q6k_load<2>(sbp + Q6K_QH + 32 * h, w.qh[h]);
#pragma unroll
        for (int e = 0; e < 4; ++e) q6k_load<4>(B + oh[e] + (long)sb * Q6K_BYTES + Q6K_SC, w.hd[e]);
    }
    // sb: the super-block w holds. Every piece is realigned by the parity of its row's super-block address (each sits
    // at a multiple of 4 past it); the two matrices' parities need not agree.
    static __device__ __forceinline__ void decode(Dec& x, const Raw& w, const uint8_t* B, long oq, const long (&oh)[4], int sb) {
        const uint32_t sh = (uint32_t)((uintptr_t)(B + oq + (long)sb * Q6K_BYTES) & 3);
        uint32_t l[4][2], hq[2][2];
#pragma unroll
        for (int i = 0; i < 4; ++i) q6k_realign<2>(w.ql[i], sh, l[i]);
#pragma unroll
        for (int h = 0; h < 2; ++h) q6k_realign<2>(w.qh[h], sh, hq[h]);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                x.cl[4 * h + 0][c] = q6k_codes<0>(l[2 * h][c], l[2 * h + 1][c], hq[h][c]);
                x.cl[4 * h + 1][c] = q6k_codes<1>(l[2 * h][c], l[2 * h + 1][c], hq[h][c]);
                x.cl[4 * h + 2][c] = q6k_codes<2>(l[2 * h][c], l[2 * h + 1][c], hq[h][c]);
                x.cl[4 * h + 3][c] = q6k_codes<3>(l[2 * h][c], l[2 * h + 1][c], hq[h][c]);
            }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t she = (uint32_t)((uintptr_t)(B + oh[e] + (long)sb * Q6K_BYTES) & 3);
            q6k_realign<4>(w.hd[e], she, x.sc[e]);
            x.d[e] = h2f((w.hd[e][4] >> (8 * she)) & 0xFFFFu);
        }
    }
    template <int j> static __device__ __forceinline__ void block(const Dec& x, long bfr, uint32_t ds, int q, float (&acc)[4]) {
        const v4i zero = {0, 0, 0, 0};
        // the A operand of the s0 MFMA keeps lanes q < 2 (elements 0..15 of the block), that of the s1 MFMA the others
        const uint32_t keep0 = q < 2 ? 0xFFFFFFFFu : 0u, keep1 = ~keep0;
        const long a0 = (long)(((unsigned long)(x.cl[j][1] & keep0) << 32) | (x.cl[j][0] & keep0));
        const long a1 = (long)(((unsigned long)(x.cl[j][1] & keep1) << 32) | (x.cl[j][0] & keep1));
        const v4i c0 = __builtin_amdgcn_mfma_i32_16x16x32_i8(a0, bfr, zero, 0, 0, 0);
        const v4i c1 = __builtin_amdgcn_mfma_i32_16x16x32_i8(a1, bfr, zero, 0, 0, 0);
        const float da = h2f(ds & 0xFFFFu);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int isum = q6k_scale<2 * j>(x.sc[e]) * c0[e] + q6k_scale<2 * j + 1>(x.sc[e]) * c1[e];
            acc[e] = __builtin_fmaf(x.d[e] * da, (float)isum, acc[e]);
        }
    }
};

// the two ops, in the expressions of qg.h (qg_gemm_w4a8_moe_glu): one rounded operation per step
__device__ __forceinline__ float glu(float g, float u, int op) {
    if (op == QG_GLU_REGLU) return (g > 0.0f ? g : 0.0f) * u;
    return (g / (1.0f + expf(-g))) * u;
}

// ---- the epilogue ---------------------------------------------------------------------------------------------------
// This wave's partial tile into part as [slice][row group][token][row]: lane (c, q) writes rows 4q .. 4q + 3 of token c
// (one 16-B store), the layout of moe_reduce_store (qg_moe_prefill.hip).
template <int TT, int RG>
__device__ __forceinline__ void glu_put_partials(float* part, const float (&acc)[TT][4], int ks, int rg, int r16, int q) {
    constexpr int PT = TT * 256;
#pragma unroll
    for (int t = 0; t < TT; ++t)
        *reinterpret_cast<float4*>(&part[(ks * RG + rg) * PT + (16 * t + r16) * 16 + 4 * q]) =
            make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
}
// output idx of the workgroup: the sum of its KS partials in slice order
template <int TT, int RG> __device__ __forceinline__ float glu_sum_partials(const float* part, int idx) {
    constexpr int KS = MMQ_WAVES / RG, PT = TT * 256;
    float sum = part[idx];
#pragma unroll
    for (int k = 1; k < KS; ++k) sum += part[k * (RG * PT) + idx];
    return sum;
}

// ---- the kernel -----------------------------------------------------------------------------------------------------
template <class S, int TT, int RG> __global__ __launch_bounds__(MMQ_WGS) void moe_glu_mmq_kernel(const MoeGluPrefillArgs a) {
    static_assert(RG == 1 || RG == 4, "row groups per workgroup");
    constexpr int W = MMQ_WAVES, KS = W / RG;
    constexpr int NBUF = RG > 1 ? 2 : 1;
    constexpr int NR = 16 / RG;          // token loads (dwords 0..63 of a token) per wave and tile
    constexpr int NT = RG == 1 ? 2 : 1;  // tail loads (dwords 64..71 of 8 tokens) per wave (RG = 4: waves 0, 1)
    constexpr int TILE_DW = 16 * TOK_DW, PT = TT * 256;
    constexpr int STAGE_DW = KS * NBUF * TILE_DW, PART_DW = W * PT;
    constexpr int NI = (RG * PT + MMQ_WGS - 1) / MMQ_WGS;  // outputs per thread
    __shared__ __attribute__((aligned(16))) uint32_t smem[STAGE_DW > PART_DW ? STAGE_DW : PART_DW];
    MoeTile mt;
    if (!moe_tile_lookup(a, mt)) return;
    const int N = a.N, nb = a.K / QK, nsb = a.K / SB_ELEMS;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int rg = wave % RG, ks = wave / RG;
    const int r16 = lane & 15, q = lane >> 4;
    const int tile = xcd_tile_x();
    if (mt.e >= a.n_expert) {
        moe_zero_tile<TT, RG>(a, mt, tile);
        return;
    }
    const int n0 = tile * (16 * RG) + 16 * rg;
    const long wrow = (long)nsb * S::BYTES;
    const long arow = (long)nb * 9;  // dwords per activation row
    const uint32_t* A = static_cast<const uint32_t*>(a.A);
    const uint8_t* Bg = static_cast<const uint8_t*>(a.B) + (long)mt.e * a.estride;
    const uint8_t* Bu = static_cast<const uint8_t*>(a.B_up) + (long)mt.e * a.estride;
    // rows past the end are clamped to the last one: loaded and multiplied, never stored
    const long oq = (long)min(n0 + r16, N - 1) * wrow;
    long oh[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) oh[e] = (long)min(n0 + 4 * q + e, N - 1) * wrow;
    uint32_t* stage = smem + ks * (NBUF * TILE_DW);
    MoeRows<TT, RG> rows;
    rows.load(mt, lane, rg);

    float accg[TT][4], accu[TT][4];
#pragma unroll
    for (int t = 0; t < TT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) accg[t][e] = accu[t][e] = 0.0f;

    const int iters = (nsb + KS - 1) / KS;  // the same for every wave
    uint32_t tl[NR + NT];
    typename S::Raw wg, wu;
    {
        const int sb0 = min(ks, nsb - 1);
        moe_load_tile<TT, RG>(tl, A, arow, rows, sb0, 0, lane, rg);
        S::load(wg, Bg, oq, oh, sb0, q);
        S::load(wu, Bu, oq, oh, sb0, q);
    }
    for (int it = 0; it < iters; ++it) {
        const int sb = it * KS + ks;
        const bool valid = sb < nsb;       // wave-uniform
        const int sbl = min(sb, nsb - 1);  // the super-block wg and wu hold
        const int sbn = min(sb + KS, nsb - 1);
        typename S::Dec dg, du;
        S::decode(dg, wg, Bg, oq, oh, sbl);
        S::decode(du, wu, Bu, oq, oh, sbl);
        static_for<TT>([&](auto T) {
            constexpr int t = decltype(T)::value;
            // this tile into the slice's LDS buffer (step parity: TT is 1 or even, so the parity is t's, or it's at
            // TT = 1), the next one (and after the last, both matrices' next super-block) in flight, then the barrier
            // between the writes and the operand reads
            uint32_t* buf = stage + (NBUF > 1 ? ((TT == 1 ? it : t) & 1) * TILE_DW : 0);
            moe_store_tile<RG>(tl, buf, lane, rg);
            if constexpr (t + 1 < TT) {
                moe_load_tile<TT, RG>(tl, A, arow, rows, sbl, t + 1, lane, rg);
            } else {
                if (it + 1 < iters) {
                    moe_load_tile<TT, RG>(tl, A, arow, rows, sbn, 0, lane, rg);
                    S::load(wg, Bg, oq, oh, sbn, q);
                    S::load(wu, Bu, oq, oh, sbn, q);
                }
            }
            __syncthreads();
            if (valid) {
                const uint32_t* tok = buf + r16 * TOK_DW;
                static_for<8>([&](auto J) {
                    constexpr int j = decltype(J)::value;
                    const uint32_t b0 = tok[9 * j + 1 + 2 * q], b1 = tok[9 * j + 2 + 2 * q], ds = tok[9 * j];
                    const long bfr = (long)(((unsigned long)b1 << 32) | b0);
                    S::template block<j>(dg, bfr, ds, q, accg[t]);
                    S::template block<j>(du, bfr, ds, q, accu[t]);
                    // a block's MFMAs and their epilogues stay together: scheduled freely, hipcc issues the tile's
                    // MFMAs first and holds all their results
                    __builtin_amdgcn_sched_barrier(0);
                });
            }
        });
    }

    // over the staging buffers, once every wave has read its last tile: the gate partials, their sums into registers,
    // then the up partials in the same region
    float* part = reinterpret_cast<float*>(smem);
    float gsum[NI];
    __syncthreads();
    glu_put_partials<TT, RG>(part, accg, ks, rg, r16, q);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int idx = threadIdx.x + i * MMQ_WGS;
        gsum[i] = idx < RG * PT ? glu_sum_partials<TT, RG>(part, idx) : 0.0f;
    }
    __syncthreads();
    glu_put_partials<TT, RG>(part, accu, ks, rg, r16, q);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int idx = threadIdx.x + i * MMQ_WGS;
        if (idx >= RG * PT) continue;
        const float usum = glu_sum_partials<TT, RG>(part, idx);
        const int g = idx / PT, o = idx - g * PT;
        const int p = o >> 4, n = tile * (16 * RG) + 16 * g + (o & 15);
        if (p < mt.rows && n < N) a.C[(long)mt.sorted[p] * a.ldc + n] = glu(gsum[i], usum, a.glu_op);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------
using Launch = MoeLaunch<MoeGluPrefillArgs>;

template <class S, int TT, int RG> hipError_t moe_glu_prefill_k(const Launch& L) {
    const MoeGluPrefillArgs& a = L.a;
    const int gx = (a.N + 16 * RG - 1) / (16 * RG), gy = (int)moe_max_tiles(a.slots, a.n_expert, 16 * TT);
    if (L.describe) {
        describe_line(L.describe, L.describe_len, "moe_glu:%s_mmq TT=%d RG=%d KS=%d R=%d grid=%dx%d", kq_family(S::WT), TT, RG,
                      MMQ_WAVES / RG, 16 * TT, gx, gy);
        return hipSuccess;
    }
    const hipError_t e = launch_moe_plan(a, TT, L.st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((moe_glu_mmq_kernel<S, TT, RG>), dim3(gx, gy), dim3(MMQ_WGS), 0, L.st, a);
    return hipGetLastError();
}

// RG is moe_prefill_form's for the shape (qg_moe_prefill.hip): it decides the bits. TT is 1 in both forms: with two
// matrices' decoded super-blocks, their per-block scale products (which hipcc keeps across the tiles of a step) and
// two accumulator sets, TT = 2 already spills at either RG (Q4_K 284 / 156, Q6_K 372 / 252 bytes of scratch per lane
// at RG = 1 / 4, TT = 4 up to 572), while TT = 1 takes 179 .. 223 VGPRs and none
// (profiles/moe_glu_prefill/resource_usage.txt). Bits do not depend on TT.
template <class S> hipError_t moe_glu_prefill_t(const Launch& L) {
    return moe_prefill_rg(L.a, S::WT) == 4 ? moe_glu_prefill_k<S, 1, 4>(L) : moe_glu_prefill_k<S, 1, 1>(L);
}

}  // namespace

hipError_t launch_moe_glu_prefill(const MoeGluPrefillArgs& a, int wtype, hipStream_t st, char* describe, size_t describe_len) {
    const Launch L{a, st, describe, describe_len};
    if (wtype == QG_TYPE_Q4_K) return moe_glu_prefill_t<Q4KSide>(L);
    if (wtype == QG_TYPE_Q6_K) return moe_glu_prefill_t<Q6KSide>(L);
    return hipErrorInvalidValue;
}

}  // namespace qg
