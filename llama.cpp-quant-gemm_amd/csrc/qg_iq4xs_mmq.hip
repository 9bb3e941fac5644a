// qg_iq4xs_mmq.hip — the IQ4_XS MFMA prefill (M >= 9 activation rows, and any M the GEMV cannot take), family
// "iq4xs_mmq".
//
// C[m * ldc + n] = sum_sb d * sum_j d_a * float((ls_j - 32) * sumi_j),  sumi_j = sum_i kv[code_i] * a_i  (qg_iq4xs.hpp)
//
// Work decomposition; the workgroup shapes, the activation staging and the K-slice reduction are those
// of qg_q4k_mmq.hip, the operand orientation that of qg_mxfp4_mmq.hip:
//  * A workgroup of 8 waves = RG row groups x KS = 8 / RG K slices owns 16 * RG weight rows x 16 * TT tokens and
//    all of K. Wave (rg, ks) takes rows 16 rg .. 16 rg + 15 and super-blocks ks, ks + KS, ...; the KS partial tiles of
//    a row group are summed through LDS in slice order, so two launches give identical bits.
//  * One v_mfma_i32_16x16x32_i8 per sub-block and 16-token tile. The decoded int8 weights are the B operand, the
//    activations the A operand, both in the plain element order (no permutation of k): MFMA lane (r, q) holds elements
//    8q .. 8q + 7 of sub-block j of weight row r, i.e. the low (q < 2) or high nibbles of qs bytes
//    16j + 8 (q & 1) .. + 7 — one 8-B load, one shift by 4 (q >> 1) and two iq4xs_kv4 per lane and sub-block, no
//    cross-lane movement, straight from global memory. The result lane (r, q) then holds row r x tokens 4q .. 4q + 3:
//    its own row's 8-B header (which it loads itself) is the only one it needs.
//  * Loads: nine 8-B loads per lane and super-block, each at a multiple of 8 inside the super-block (136 = 8 x 17).
//  * The activations are staged through LDS per (K slice, 16-token tile) as in q4k_mmq: a token's 8 blocks of one
//    super-block are 288 contiguous bytes (9 dwords per block; s_a rides along and is ignored); one barrier per step;
//    double buffered with RG > 1.
//  * VALU epilogue per sub-block: (ls_j - 32) * sumi in int32 (below 2^24), converted, inner = fma(d_a, .., inner) with
//    d_a of the lane's four tokens read from the tile; per super-block acc = fma(d, inner, acc).
//  * Tolerance: W = IQ4XS_MMQ_W = 8 (derived in qg_iq4xs.hpp).
//  * SUMI: the same instantiation stores each sub-block's int32 dot in place of the epilogue.
#include "qg_iq4xs.hpp"
#include "qg_kq_launch.hpp"

namespace qg {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));

constexpr int IQ4XS_MMQ_WAVES = 8;
constexpr int IQ4XS_MMQ_WGS = 64 * IQ4XS_MMQ_WAVES;
static_assert(IQ4XS_MMQ_W == IQ4XS_MMQ_WAVES, "at most one partial per wave");

// The K loop is qg_iq4xs_mmq_body.inc.
template <int TT, int RG, bool SUMI>
__global__ __launch_bounds__(IQ4XS_MMQ_WGS) void iq4xs_mmq_kernel(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                                 int M, int N, int K, void* __restrict__ out, long ldc) {
    static_assert(RG == 1 || RG == 4, "row groups per workgroup");
    constexpr int W = IQ4XS_MMQ_WAVES, KS = W / RG;
    constexpr int NBUF = RG > 1 ? 2 : 1;
    constexpr int NR = 16 / RG;             // token loads (dwords 0..63 of a token) per wave and tile
    constexpr int NT = RG == 1 ? 2 : 1;     // tail loads (dwords 64..71 of 8 tokens) per wave (RG = 4: waves 0, 1)
    constexpr int STAGE_DW = KS * NBUF * IQ4XS_TILE_DW, PART_DW = SUMI ? 0 : W * TT * 256;
    __shared__ __attribute__((aligned(16))) uint32_t smem[STAGE_DW > PART_DW ? STAGE_DW : PART_DW];
    const int nb = K / QK, nsb = K / SB_ELEMS;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int rg = wave % RG, ks = wave / RG;
    const int r16 = lane & 15, q = lane >> 4;
    const int tile = gridDim.x <= 512 ? xcd_tile(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int n0 = tile * (16 * RG) + 16 * rg, m0 = blockIdx.y * (16 * TT);
    const long arow = (long)nb * 9;  // dwords per activation row
    // rows / tokens past the end are clamped to the last one: loaded and multiplied, never stored
    const uint8_t* wq = B + (long)min(n0 + r16, N - 1) * ((long)nsb * IQ4XS_BYTES);  // the row of MFMA lane (r16, q)
    uint32_t* stage = smem + ks * (NBUF * IQ4XS_TILE_DW);

    // this wave's share of a 16-token tile of super-block sb: token loads r take dwords 0..63 of token NR rg + r (the
    // token's row is wave-uniform, so its address lives in SGPRs), a tail load dwords 64..71 of 8 tokens
    const bool tail = RG == 1 || rg < 2;
    auto load_tile = [&](uint32_t (&dst)[NR + NT], int sb, int t) {
        const uint32_t* a = A + (long)sb * IQ4XS_TOK_DW;
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
        for (int r = 0; r < NR; ++r) buf[(NR * rg + r) * IQ4XS_TOK_DW + lane] = src[r];
        if (tail) {
#pragma unroll
            for (int b = 0; b < NT; ++b)
                buf[(8 * (RG == 1 ? b : rg) + (lane >> 3)) * IQ4XS_TOK_DW + 64 + (lane & 7)] = src[NR + b];
        }
    };
#include "qg_iq4xs_mmq_body.inc"
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
        for (int idx = threadIdx.x; idx < RG * PT; idx += IQ4XS_MMQ_WGS) {
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
struct iq4xs_mmq_fmt {
    static constexpr int WT = QG_TYPE_IQ4_XS, WAVES = IQ4XS_MMQ_WAVES;
    template <int TT, int RG, bool SUMI> static auto kernel() { return iq4xs_mmq_kernel<TT, RG, SUMI>; }
};

}  // namespace

bool iq4xs_mmq_eligible(const GemmArgs& g) { return kq_mmq_eligible<iq4xs_mmq_fmt>(g); }
hipError_t launch_iq4xs_mmq(const GemmArgs& g, hipStream_t st) { return kq_mmq_launch<iq4xs_mmq_fmt>(g, st); }

}  // namespace qg
