// qg_mxfp4_mmq.hip — the MXFP4 MFMA prefill (M >= 9 activation rows, and any M the GEMV cannot take), family
// "mxfp4_mmq".
//
// C[m * ldc + n] = sum_b (d_a * scale(e)) * float(sumi),  sumi = sum_j kv[code_j] * a_j   (qg_mxfp4.hpp)
//
// Work decomposition; the workgroup shapes, the activation staging and the K-slice reduction are those
// of qg_q4k_mmq.hip, by groups of 8 blocks where that kernel has super-blocks (K / 32 need be no multiple of 8: the
// last group of a row is partial, its missing blocks skipped by a wave-uniform test):
//  * A workgroup of 8 waves = RG row groups x KS = 8 / RG K slices owns 16 * RG weight rows x 16 * TT tokens and
//    all of K. Wave (rg, ks) takes rows 16 rg .. 16 rg + 15 and groups ks, ks + KS, ...; the KS partial tiles of a row
//    group are summed through LDS in slice order, so two launches give identical bits.
//  * One v_mfma_i32_16x16x32_i8 per block and 16-token tile. The decoded int8 weights are the B operand, the
//    activations the A operand: MFMA lane (r, q) holds elements 8q .. 8q + 7 of block b of weight row r, i.e. the low
//    (q < 2) or high nibbles of qs bytes 8 (q & 1) .. + 7, turned into kv bytes by mxfp4_kv4, no cross-lane movement,
//    straight from global memory. The result lane (r, q) then holds row r x tokens 4q .. 4q + 3: its own row's e is
//    the only scale it needs (with the weights as the A operand it would need e of four other rows per block).
//  * Loads (qg_mxfp4.hpp): of each block's five-dword cover a lane reads dword 0 (e) and the three dwords that hold its
//    8 qs bytes (0..2 or 2..4), realigned with v_alignbyte by the block address's low two bits. No load at an address
//    that is not a multiple of 4, none outside the cover of a block of the tensor: nothing is read past the tensor.
//  * The activations are staged through LDS per (K slice, 16-token tile) as in q4k_mmq: a token's 8 blocks of one
//    group are 288 contiguous bytes (9 dwords per block; s_a rides along and is ignored); one barrier per step; double
//    buffered with RG > 1. A partial group's loads are clamped to the row's last dword.
//  * Epilogue per block: acc = fma(d_a * scale(e), float(sumi), acc), d_a of the lane's four tokens read from the tile.
//  * Tolerance: W = MXFP4_MMQ_W = 8. An output is the sum of KS <= 8 slice partials, each an fma chain over the
//    slice's blocks.
//  * SUMI: the same instantiation stores sumi in place of the epilogue.
#include "qg_kq_launch.hpp"
#include "qg_mxfp4.hpp"

namespace qg {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int MXFP4_MMQ_WAVES = 8;
constexpr int MXFP4_MMQ_WGS = 64 * MXFP4_MMQ_WAVES;
static_assert(MXFP4_MMQ_W == MXFP4_MMQ_WAVES, "at most one partial per wave");

// The K loop is qg_mxfp4_mmq_body.inc.
template <int TT, int RG, bool SUMI>
__global__ __launch_bounds__(MXFP4_MMQ_WGS) void mxfp4_mmq_kernel(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                                 int M, int N, int K, void* __restrict__ out, long ldc) {
    static_assert(RG == 1 || RG == 4, "row groups per workgroup");
    constexpr int W = MXFP4_MMQ_WAVES, KS = W / RG;
    constexpr int NBUF = RG > 1 ? 2 : 1;
    constexpr int NR = 16 / RG;             // token loads (dwords 0..63 of a token) per wave and tile
    constexpr int NT = RG == 1 ? 2 : 1;     // tail loads (dwords 64..71 of 8 tokens) per wave (RG = 4: waves 0, 1)
    constexpr int STAGE_DW = KS * NBUF * MXFP4_TILE_DW, PART_DW = SUMI ? 0 : W * TT * 256;
    __shared__ __attribute__((aligned(16))) uint32_t smem[STAGE_DW > PART_DW ? STAGE_DW : PART_DW];
    const int nb = K / QK, ngrp = (nb + 7) / 8;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int rg = wave % RG, ks = wave / RG;
    const int r16 = lane & 15, q = lane >> 4;
    const int tile = gridDim.x <= 512 ? xcd_tile(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int n0 = tile * (16 * RG) + 16 * rg, m0 = blockIdx.y * (16 * TT);
    const int arow = nb * 9;  // dwords per activation row
    // rows / tokens past the end are clamped to the last one: loaded and multiplied, never stored
    const uint8_t* wq = B + (long)min(n0 + r16, N - 1) * ((long)nb * MXFP4_BYTES);  // the row of MFMA lane (r16, q)
    uint32_t* stage = smem + ks * (NBUF * MXFP4_TILE_DW);

    // this wave's share of a 16-token tile of group g: token loads r take dwords 0..63 of token NR rg + r (the token's
    // row is wave-uniform, so its address lives in SGPRs), a tail load dwords 64..71 of 8 tokens; dwords past the
    // row's end (a partial last group) are clamped to its last one
    const bool tail = RG == 1 || rg < 2;
    auto load_tile = [&](uint32_t (&dst)[NR + NT], int g, int t) {
        const int c0 = g * MXFP4_TOK_DW;
#pragma unroll
        for (int r = 0; r < NR; ++r)
            dst[r] = A[(long)min(m0 + 16 * t + NR * rg + r, M - 1) * arow + min(c0 + lane, arow - 1)];
        if (tail) {
#pragma unroll
            for (int b = 0; b < NT; ++b) {
                const int tk = 8 * (RG == 1 ? b : rg) + (lane >> 3);
                dst[NR + b] = A[(long)min(m0 + 16 * t + tk, M - 1) * arow + min(c0 + 64 + (lane & 7), arow - 1)];
            }
        }
    };
    auto store_tile = [&](const uint32_t (&src)[NR + NT], uint32_t* buf) {
#pragma unroll
        for (int r = 0; r < NR; ++r) buf[(NR * rg + r) * MXFP4_TOK_DW + lane] = src[r];
        if (tail) {
#pragma unroll
            for (int b = 0; b < NT; ++b)
                buf[(8 * (RG == 1 ? b : rg) + (lane >> 3)) * MXFP4_TOK_DW + 64 + (lane & 7)] = src[NR + b];
        }
    };
#include "qg_mxfp4_mmq_body.inc"
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
        for (int idx = threadIdx.x; idx < RG * PT; idx += MXFP4_MMQ_WGS) {
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
struct mxfp4_mmq_fmt {
    static constexpr const char* NAME = "mxfp4_mmq";
    static constexpr int WAVES = MXFP4_MMQ_WAVES, KMULT = QK;
    static constexpr uintptr_t WMASK = 0;  // any byte: every load is realigned
    template <int TT, int RG, bool SUMI> static auto kernel() { return mxfp4_mmq_kernel<TT, RG, SUMI>; }
};

}  // namespace

bool mxfp4_mmq_eligible(const GemmArgs& g) { return kq_mmq_eligible<mxfp4_mmq_fmt>(g); }
hipError_t launch_mxfp4_mmq(const GemmArgs& g, hipStream_t st) { return kq_mmq_launch<mxfp4_mmq_fmt>(g, st); }

}  // namespace qg
