// qg_q6k_mmq.hip — the Q6_K MFMA prefill (M >= 9 activation rows, and any M the GEMV cannot take), family "q6k_mmq".
//
// C[m * ldc + n] = sum_sb sum_b (d * d_a) * float(scales[2b] * s0 + scales[2b + 1] * s1)   (qg_q6k.hpp)
//
// Work decomposition ("Q6_K"); the workgroup shapes, the activation staging and the K-slice reduction
// are those of qg_q4k_mmq.hip:
//  * A workgroup of 8 waves = RG row groups x KS = 8 / RG K slices owns 16 * RG weight rows x 16 * TT tokens and
//    all of K. Wave (rg, ks) takes rows 16 rg .. 16 rg + 15 and super-blocks ks, ks + KS, ...; the KS partial tiles
//    of a row group are summed through LDS in slice order, so two launches give identical bits.
//  * v_mfma_i32_16x16x32_i8, the weights as the A operand: MFMA lane (r, q) holds k = 8q .. 8q + 7 of Q8_1 block
//    b = 4h + c of row r, i.e. 8 bytes of ql at 64h + 32(c & 1) + 8q and 8 bytes of qh at 32h + 8q. Per
//    super-block a lane reads four ql pieces and two qh pieces of 8 bytes and builds the 8 blocks' signed codes
//    from them (q6k_codes), no cross-lane movement, straight from global memory.
//  * A Q8_1 block spans two scale groups, and the lanes q < 2 hold exactly the first one: two MFMAs per block and
//    token tile, the A operand zeroed in lanes q >= 2 for s0 and in lanes q < 2 for s1 (the matrix pipe is far
//    from busy in the sibling kernels). isum = scales[2b] * s0 + scales[2b + 1] * s1 in int32.
//  * Loads (qg_q6k.hpp, q6k_load): every piece is 0 or 2 bytes off a dword depending on the lane's row and the
//    super-block; each is read as the dword-aligned span that covers it plus one dword and realigned with
//    v_alignbyte. The extra dword of a ql / qh piece ends before byte 196 of the super-block; the result lane's
//    header piece is scales[16] and d as one 18-byte stream (5 dwords: bytes 192..211 at parity 0, 190..209 at
//    parity 2). No load at an address that is not a multiple of 4, none of a dword without a byte of the tensor;
//    only the last super-block's final dword at parity 0 is half outside it, in the same page. By construction;
//    no test probes it.
//  * The activations are the B operand, staged through LDS per (K slice, 16-token tile) as in q4k_mmq: a token's
//    8 blocks of one super-block are 288 contiguous bytes; one barrier per step; double buffered with RG > 1.
//  * The result lane (c, q) holds token c x rows 4q .. 4q + 3, reads those rows' headers itself and applies
//    acc = fma(d * d_a, float(isum), acc) per block.
//  * Tolerance: W = 8. An output is the sum of KS <= 8 slice partials, each an fma chain over the slice's blocks:
//    K/32 terms of two roundings each plus at most 8 chained partial sums.
//  * SUMI: the same instantiation stores isum in place of the epilogue.
#include "qg_kq_launch.hpp"
#include "qg_q6k.hpp"

namespace qg {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int Q6K_MMQ_WAVES = 8;
constexpr int Q6K_MMQ_WGS = 64 * Q6K_MMQ_WAVES;

// The K loop is qg_q6k_mmq_body.inc, shared as text with the expert-grouped launch (qg_moe_prefill.hip).
template <int TT, int RG, bool SUMI>
__global__ __launch_bounds__(Q6K_MMQ_WGS) void q6k_mmq_kernel(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                             int M, int N, int K, void* __restrict__ out, long ldc) {
    static_assert(RG == 1 || RG == 4, "row groups per workgroup");
    constexpr int W = Q6K_MMQ_WAVES, KS = W / RG;
    constexpr int NBUF = RG > 1 ? 2 : 1;
    constexpr int NR = 16 / RG;             // token loads (dwords 0..63 of a token) per wave and tile
    constexpr int NT = RG == 1 ? 2 : 1;     // tail loads (dwords 64..71 of 8 tokens) per wave (RG = 4: waves 0, 1)
    constexpr int STAGE_DW = KS * NBUF * Q6K_TILE_DW, PART_DW = SUMI ? 0 : W * TT * 256;
    __shared__ __attribute__((aligned(16))) uint32_t smem[STAGE_DW > PART_DW ? STAGE_DW : PART_DW];
    const int nb = K / QK, nsb = K / SB_ELEMS;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int rg = wave % RG, ks = wave / RG;
    const int r16 = lane & 15, q = lane >> 4;
    const int tile = gridDim.x <= 512 ? xcd_tile(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int n0 = tile * (16 * RG) + 16 * rg, m0 = blockIdx.y * (16 * TT);
    const long wrow = (long)nsb * Q6K_BYTES;
    const long arow = (long)nb * 9;  // dwords per activation row
    // rows / tokens past the end are clamped to the last one: loaded and multiplied, never stored
    const uint8_t* wq = B + (long)min(n0 + r16, N - 1) * wrow;  // the operand row of MFMA lane (r16, q)
    const uint8_t* wh[4];                                       // the result lane's rows 4q .. 4q + 3
#pragma unroll
    for (int e = 0; e < 4; ++e) wh[e] = B + (long)min(n0 + 4 * q + e, N - 1) * wrow;
    uint32_t* stage = smem + ks * (NBUF * Q6K_TILE_DW);

    // this wave's share of a 16-token tile of super-block sb: token loads r take dwords 0..63 of token NR rg + r (the
    // token's row is wave-uniform, so its address lives in SGPRs), a tail load dwords 64..71 of 8 tokens
    const bool tail = RG == 1 || rg < 2;
    auto load_tile = [&](uint32_t (&dst)[NR + NT], int sb, int t) {
        const uint32_t* a = A + (long)sb * Q6K_TOK_DW;
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
        for (int r = 0; r < NR; ++r) buf[(NR * rg + r) * Q6K_TOK_DW + lane] = src[r];
        if (tail) {
#pragma unroll
            for (int b = 0; b < NT; ++b)
                buf[(8 * (RG == 1 ? b : rg) + (lane >> 3)) * Q6K_TOK_DW + 64 + (lane & 7)] = src[NR + b];
        }
    };
#include "qg_q6k_mmq_body.inc"
    if constexpr (!SUMI) {
        // partial tiles as [slice][row group][token][row] (over the staging buffers, once every wave has read its
        // last tile): lane (c, q) writes rows 4q .. 4q + 3 of token c (one 16-B store)
        constexpr int PT = TT * 256;  // outputs per (slice, row group)
        __syncthreads();
        float* part = reinterpret_cast<float*>(smem);
#pragma unroll
        for (int t = 0; t < TT; ++t)
            *reinterpret_cast<float4*>(&part[(ks * RG + rg) * PT + (16 * t + r16) * 16 + 4 * q]) =
                make_float4(acc[t][0], acc[t][1], acc[t][2], acc[t][3]);
        __syncthreads();
        float* C = static_cast<float*>(out);
        for (int idx = threadIdx.x; idx < RG * PT; idx += Q6K_MMQ_WGS) {
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
struct q6k_mmq_fmt {
    static constexpr const char* NAME = "q6k_mmq";
    static constexpr int WAVES = Q6K_MMQ_WAVES, KMULT = SB_ELEMS;
    static constexpr uintptr_t WMASK = 1;  // every load is realigned
    template <int TT, int RG, bool SUMI> static auto kernel() { return q6k_mmq_kernel<TT, RG, SUMI>; }
};

}  // namespace

bool q6k_mmq_eligible(const GemmArgs& g) { return kq_mmq_eligible<q6k_mmq_fmt>(g); }
hipError_t launch_q6k_mmq(const GemmArgs& g, hipStream_t st) { return kq_mmq_launch<q6k_mmq_fmt>(g, st); }

}  // namespace qg
