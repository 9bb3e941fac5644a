// qg_q3k_mmq.hip — the Q3_K MFMA prefill (M >= 7 activation rows, and any M the GEMV cannot take), family "q3k_mmq".
//
// C[m * ldc + n] = sum_sb d * sum_b d_a * float(isum_b),  isum_b = s_2b * sum_{l<16} q a + s_2b+1 * sum_{l>=16} q a
// (qg_q3k.hpp)
//
// Work decomposition; the workgroup shapes, the activation staging and the K-slice reduction are those
// of qg_q4k_mmq.hip, the operand orientation that of qg_iq4xs_mmq.hip:
//  * A workgroup of 8 waves = RG row groups x KS = 8 / RG K slices owns 16 * RG weight rows x 16 * TT tokens and
//    all of K. Wave (rg, ks) takes rows 16 rg .. 16 rg + 15 and super-blocks ks, ks + KS, ...; the KS partial tiles of
//    a row group are summed through LDS in slice order, so two launches give identical bits.
//  * ONE v_mfma_i32_16x16x32_i8 per Q8_1 block and 16-token tile, where Q6_K needs two with half an operand zeroed:
//    the 16-element scale is inside the int8 operand ((4 - u) s, qg_q3k.hpp), so the MFMA's sum over k = 32 IS -isum_b.
//    The pre-scaled weights are the B operand, the activations the A operand, both in the plain element order: MFMA
//    lane (r, q) holds elements 8q .. 8q + 7 of block b of weight row r, all in scale group 2b + (q >> 1). The result
//    lane (r, q) then holds row r x tokens 4q .. 4q + 3: its own row's scales and d are the only ones it needs.
//  * Loads: per lane and super-block three 8-byte spans, qs[8q ..], qs[32 + 8q ..] and hmask[8q ..], which hold its
//    operand bytes of all 8 blocks, and scales[12] with d: four q6k_load spans, 3 + 3 + 3 + 4 aligned dwords, realigned
//    by the super-block's address parity. No cross-lane movement, straight from global memory.
//  * Per block: the group's table (q3k_table_lo / _hi), per operand dword a shift and a mask of qs, a shift and a mask
//    of hmask, an or and one v_perm_b32.
//  * The activations are staged through LDS per (K slice, 16-token tile) as in q4k_mmq: a token's 8 blocks of one
//    super-block are 288 contiguous bytes (9 dwords per block; s_a rides along and is ignored); one barrier per step;
//    double buffered with RG > 1.
//  * Epilogue per block: acc = fma((-d) * d_a, float(c), acc) with d_a of the lane's four tokens read from the tile;
//    |c| <= 2^19, its conversion is exact.
//  * Tolerance: W = Q3K_MMQ_W = 7 (derived in qg_q3k.hpp).
//  * SUMI: the same instantiation stores each block's isum = -c in place of the epilogue.
#include "qg_q3k.hpp"
#include "qg_kq_launch.hpp"

namespace qg {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int Q3K_MMQ_WAVES = 8;
constexpr int Q3K_MMQ_WGS = 64 * Q3K_MMQ_WAVES;
static_assert(Q3K_MMQ_W == Q3K_MMQ_WAVES - 1, "one slice addition per wave after the first");

// The K loop is qg_q3k_mmq_body.inc.
template <int TT, int RG, bool SUMI>
__global__ __launch_bounds__(Q3K_MMQ_WGS) void q3k_mmq_kernel(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                             int M, int N, int K, void* __restrict__ out, long ldc) {
    static_assert(RG == 1 || RG == 4, "row groups per workgroup");
    constexpr int W = Q3K_MMQ_WAVES, KS = W / RG;
    constexpr int NBUF = RG > 1 ? 2 : 1;
    constexpr int NR = 16 / RG;             // token loads (dwords 0..63 of a token) per wave and tile
    constexpr int NT = RG == 1 ? 2 : 1;     // tail loads (dwords 64..71 of 8 tokens) per wave (RG = 4: waves 0, 1)
    constexpr int STAGE_DW = KS * NBUF * Q3K_TILE_DW, PART_DW = SUMI ? 0 : W * TT * 256;
    __shared__ __attribute__((aligned(16))) uint32_t smem[STAGE_DW > PART_DW ? STAGE_DW : PART_DW];
    const int nb = K / QK, nsb = K / SB_ELEMS;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int rg = wave % RG, ks = wave / RG;
    const int r16 = lane & 15, q = lane >> 4;
    const int tile = gridDim.x <= 512 ? xcd_tile(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int n0 = tile * (16 * RG) + 16 * rg, m0 = blockIdx.y * (16 * TT);
    const long arow = (long)nb * 9;  // dwords per activation row
    // rows / tokens past the end are clamped to the last one: loaded and multiplied, never stored
    const uint8_t* wq = B + (long)min(n0 + r16, N - 1) * ((long)nsb * Q3K_BYTES);  // the row of MFMA lane (r16, q)
    uint32_t* stage = smem + ks * (NBUF * Q3K_TILE_DW);

    // this wave's share of a 16-token tile of super-block sb: token loads r take dwords 0..63 of token NR rg + r (the
    // token's row is wave-uniform, so its address lives in SGPRs), a tail load dwords 64..71 of 8 tokens
    const bool tail = RG == 1 || rg < 2;
    auto load_tile = [&](uint32_t (&dst)[NR + NT], int sb, int t) {
        const uint32_t* a = A + (long)sb * Q3K_TOK_DW;
#pragma unroll
        for (int r = 0; r < NR; ++r) dst[r] = a[(long)min(m0 + 16 * t + NR * rg + r, M - 1) * arow + lane];
        if (tail) {
#pragma unroll
            for (int b = 0; b < NT; ++b) {
                const int tk = 8 * (RG == 1 ? b : rg) + (lane >> 3);
                dst[NR + b] = a[(long)min(m0 + 16 * t + tk, M - 1) * arow + 64 + (lane & 7)];
            }
        }
    };
    auto store_tile = [&](const uint32_t (&src)[NR + NT], uint32_t* buf) {
#pragma unroll
        for (int r = 0; r < NR; ++r) buf[(NR * rg + r) * Q3K_TOK_DW + lane] = src[r];
        if (tail) {
#pragma unroll
            for (int b = 0; b < NT; ++b)
                buf[(8 * (RG == 1 ? b : rg) + (lane >> 3)) * Q3K_TOK_DW + 64 + (lane & 7)] = src[NR + b];
        }
    };
#include "qg_q3k_mmq_body.inc"
    if constexpr (!SUMI) {
        // partial tiles as [slice][row group][token][row] (over the staging buffers, once every wave has read its
        // last tile): lane (r, q) writes row r of tokens 4q .. 4q + 3
        constexpr int PT = TT * 256;  // outputs per (slice, row group)
        __syncthreads();
        float* part = reinterpret_cast<float*>(smem);
#pragma unroll
        for (int t = 0; t < TT; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) part[(ks * RG + rg) * PT + (16 * t + 4 * q + e) * 16 + r16] = acc[t][e];
        __syncthreads();
        float* C = static_cast<float*>(out);
        for (int idx = threadIdx.x; idx < RG * PT; idx += Q3K_MMQ_WGS) {
            float sum = part[idx];
#pragma unroll
            for (int k = 1; k < KS; ++k) sum += part[k * (RG * PT) + idx];
            const int g = idx / PT, o = idx - g * PT;
            const int m = m0 + (o >> 4), n = tile * (16 * RG) + 16 * g + (o & 15);
            if (m < M && n < N) C[m * ldc + n] = sum;
        }
    }
}

// instantiation choice, launch and eligibility: qg_kq_launch.hpp
struct q3k_mmq_fmt {
    static constexpr int WT = QG_TYPE_Q3_K, WAVES = Q3K_MMQ_WAVES;
    template <int TT, int RG, bool SUMI> static auto kernel() { return q3k_mmq_kernel<TT, RG, SUMI>; }
};

}  // namespace

bool q3k_mmq_eligible(const GemmArgs& g) { return kq_mmq_eligible<q3k_mmq_fmt>(g); }
hipError_t launch_q3k_mmq(const GemmArgs& g, hipStream_t st) { return kq_mmq_launch<q3k_mmq_fmt>(g, st); }

}  // namespace qg
