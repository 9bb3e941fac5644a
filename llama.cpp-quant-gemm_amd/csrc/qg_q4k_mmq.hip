// qg_q4k_mmq.hip — the Q4_K MFMA prefill (M >= 9 activation rows), family "q4k_mmq".
//
// C[m * ldc + n] = sum_sb sum_j [ (d * sc_j) * d_a * float(sumi_j) - (dmin * m_j) * s_a ]   (qg_q4k.hpp)
//
// Work decomposition ("Q4_K"):
//  * A workgroup of 8 waves = RG row groups x KS = 8 / RG K slices owns 16 * RG weight rows x 16 * TT tokens and
//    all of K. Wave (rg, ks) takes rows 16 rg .. 16 rg + 15 and super-blocks ks, ks + KS, ... (a fixed K slice);
//    the KS partial tiles of a row group are summed through LDS in slice order: a fixed order of at most 8
//    partials per output, so two launches give identical bits. RG = 1 (8 K slices) keeps every CU busy at small
//    M; RG = 4 (64-row tiles, 2 K slices) is taken once its grid fills the CUs: its 4 row groups share each staged
//    activation tile, a quarter of the activation traffic per output.
//  * One v_mfma_i32_16x16x32_i8 per sub-block and 16-token tile. The weights are the A operand: MFMA lane
//    (r, q) needs elements 8q .. 8q + 7 of row r, which for sub-block 2i are the low nibbles of
//    qs[32i + 8q .. + 7] and for sub-block 2i + 1 the high nibbles of the same 8 bytes — one 8-byte load and
//    two mask ops per lane give the A operands of two MFMAs, no cross-lane movement, straight from global memory.
//  * The activations are the B operand: lane (c, q) needs bytes 8q .. 8q + 7 of token c's Q8_1 block. A token's
//    8 blocks of one super-block are 288 contiguous bytes, so the K slice's waves copy the 16 tokens' segments
//    (1152 dwords, 18 coalesced dword loads split over the RG waves, the next tile's in flight while the current
//    one computes) into the slice's LDS buffer and read operands and (d_a, s_a) from there. (The first version
//    loaded every operand from global memory, 16 cache lines per load: 26.0 us at M = 32 and 244 us at M = 512,
//    N = K = 4096; profiles/q4k/README.md.) The token stride of 72 dwords puts tokens c and c + 8 on the same
//    banks: 128 dwords per operand read over 64 banks, the two-cycle minimum.
//  * One barrier per step, between the tile's LDS writes and its operand reads. With RG > 1 the buffer is shared
//    by the slice's waves, so it is double buffered: the step after next overwrites a buffer only after the
//    barrier in between, which every wave passes after its reads. Every wave runs the same number of steps
//    (super-blocks past K are skipped wave-uniformly), so all of them reach every barrier.
//  * The result lane (c, q) holds token c x rows 4q .. 4q + 3, so it reads those 4 rows' 16-B headers
//    (d, dmin, scales) itself — again no cross-lane movement — and applies the per-sub-block epilogue with
//    two fma per output: acc = fma((d * sc_j) * d_a, float(sumi), acc); acc = fma(-(dmin * m_j), s_a, acc).
//  * hipcc pads the MFMA results' 8 wait states (tests/test_isa_hazards.py scans this kernel too).
//  * SUMI: the same instantiation stores each sub-block's int32 dot in place of the epilogue.
#include "qg_kq_launch.hpp"
#include "qg_q4k.hpp"

namespace qg {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int Q4K_MMQ_WAVES = 8;
constexpr int Q4K_MMQ_WGS = 64 * Q4K_MMQ_WAVES;

// The K loop is qg_q4k_mmq_body.inc, shared as text with the expert-grouped launch (qg_moe_prefill.hip).
template <int TT, int RG, bool SUMI>
__global__ __launch_bounds__(Q4K_MMQ_WGS) void q4k_mmq_kernel(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                             int M, int N, int K, void* __restrict__ out, long ldc) {
    static_assert(RG == 1 || RG == 4, "row groups per workgroup");
    constexpr int W = Q4K_MMQ_WAVES, KS = W / RG;
    constexpr int NBUF = RG > 1 ? 2 : 1;
    constexpr int NR = 16 / RG;             // token loads (dwords 0..63 of a token) per wave and tile
    constexpr int NT = RG == 1 ? 2 : 1;     // tail loads (dwords 64..71 of 8 tokens) per wave (RG = 4: waves 0, 1)
    constexpr int STAGE_DW = KS * NBUF * Q4K_TILE_DW, PART_DW = SUMI ? 0 : W * TT * 256;
    __shared__ __attribute__((aligned(16))) uint32_t smem[STAGE_DW > PART_DW ? STAGE_DW : PART_DW];
    const int nb = K / QK, nsb = K / SB_ELEMS;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int rg = wave % RG, ks = wave / RG;
    const int r16 = lane & 15, q = lane >> 4;
    const int tile = gridDim.x <= 512 ? xcd_tile(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int n0 = tile * (16 * RG) + 16 * rg, m0 = blockIdx.y * (16 * TT);
    const long wrow = (long)nsb * Q4K_BYTES;
    const long arow = (long)nb * 9;  // dwords per activation row
    // rows / tokens past the end are clamped to the last one: loaded and multiplied, never stored
    const uint8_t* wq = B + (long)min(n0 + r16, N - 1) * wrow + 16 + 8 * q;
    const uint8_t* wh[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) wh[e] = B + (long)min(n0 + 4 * q + e, N - 1) * wrow;
    uint32_t* stage = smem + ks * (NBUF * Q4K_TILE_DW);

    // this wave's share of a 16-token tile of super-block sb: token loads r take dwords 0..63 of token NR rg + r (the
    // token's row is wave-uniform, so its address lives in SGPRs), a tail load dwords 64..71 of 8 tokens
    const bool tail = RG == 1 || rg < 2;
    auto load_tile = [&](uint32_t (&dst)[NR + NT], int sb, int t) {
        const uint32_t* a = A + (long)sb * Q4K_TOK_DW;
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
        for (int r = 0; r < NR; ++r) buf[(NR * rg + r) * Q4K_TOK_DW + lane] = src[r];
        if (tail) {
#pragma unroll
            for (int b = 0; b < NT; ++b)
                buf[(8 * (RG == 1 ? b : rg) + (lane >> 3)) * Q4K_TOK_DW + 64 + (lane & 7)] = src[NR + b];
        }
    };
#include "qg_q4k_mmq_body.inc"
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
        for (int idx = threadIdx.x; idx < RG * PT; idx += Q4K_MMQ_WGS) {
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
struct q4k_mmq_fmt {
    static constexpr const char* NAME = "q4k_mmq";
    static constexpr int WAVES = Q4K_MMQ_WAVES, KMULT = SB_ELEMS;
    static constexpr uintptr_t WMASK = 15;  // the 16-B header loads
    template <int TT, int RG, bool SUMI> static auto kernel() { return q4k_mmq_kernel<TT, RG, SUMI>; }
};

}  // namespace

bool q4k_mmq_eligible(const GemmArgs& g) { return kq_mmq_eligible<q4k_mmq_fmt>(g); }
hipError_t launch_q4k_mmq(const GemmArgs& g, hipStream_t st) { return kq_mmq_launch<q4k_mmq_fmt>(g, st); }

}  // namespace qg
