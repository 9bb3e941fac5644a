// qg_q4k_gemv.hip — the Q4_K decode GEMV (M <= 8 activation rows), family "q4k_gemv".
//
// C[m * ldc + n] = sum_sb [ d * sum_j d_a * float(sc_j * sumi_j) - dmin * sum_j float(m_j) * s_a ]   (qg_q4k.hpp)
//
// Work decomposition ("Q4_K"):
//  * A lane's unit is one chunk of a super-block: its 16-B header (d, dmin, scales) and the chunk's 32 qs bytes
//    = sub-blocks 2i and 2i + 1, three global_load_dwordx4, always 16-B aligned (QG_Q4K_NT below: without the
//    nontemporal hint). LPR lanes share a weight row and stride over its K / 64 units, the next one in flight while
//    the current one computes; 64 / LPR rows per wave. At K = 4096 a wave is one row, a CU holds 16 waves and the
//    kernel has no unit loop (ONE).
//    (The first version gave a lane whole super-blocks, 9 loads: one wave per SIMD and no overlap of the dot
//    with the weight stream — 6.79 us against 3.30 for Q4_0 at M = 1, N = K = 4096; profiles/q4k/README.md.)
//  * The workgroup stages the M activation rows once into LDS, one thread per Q8_1 block: per (token,
//    super-block) the 8 blocks' qs dwords (64), then their (d_a, s_a) as fp32 pairs (16), 4 pad dwords. The
//    thread's first block is loaded before the weight stream, so the staging waits only on it.
//  * qs dword t of the chunk needs no nibble shuffling: v & 0x0F0F0F0F is four elements of sub-block 2i,
//    (v >> 4) & 0x0F0F0F0F the same four positions of sub-block 2i + 1; both feed v_dot4 against the matching
//    activation dwords, 8 dot4 per sub-block, exact int32 sumi. The chunk is masked once and reused by every
//    token.
//  * sc_j * sumi_j in int32 (below 2^24: the conversion is exact), one fp32 dot accumulator and one min
//    accumulator per (token, unit); d and dmin are applied once per unit.
//  * Per-lane partials (unit order) are reduced across the row's LPR lanes with DPP row ops (group_sum_last),
//    fixed order: two launches give identical bits.
//  * XCD-aware tile order on grids of one dispatch round (xcd_tile), as the row GEMV.
//  * SUMI: the same instantiation stores each sub-block's int32 dot in place of the epilogue.
// Argument order: everything (11 dwords) is preloaded into SGPRs by the dispatch (csrc/Makefile).
#include "qg_kq_launch.hpp"
#include "qg_q4k.hpp"

namespace qg {
namespace {

// ONE: every lane owns at most one unit (K <= 64 LPR): no unit loop in the kernel, so the wait for the weight
// loads sits at their first use, behind the activation records (the row GEMV's ONEU form).
// The body is qg_q4k_gemv_body.inc, shared as text with the MoE launches (qg_moe.hip, qg_moe_batch.hip).
template <int MT, int LPR, int WGS, bool SUMI, bool ONE>
__global__ __launch_bounds__(WGS) void q4k_gemv_kernel(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                      int M, int N, int K, void* __restrict__ out, long ldc) {
#define QG_KQ_DECLARE_TILE const int tile = gridDim.x <= 512 ? xcd_tile(blockIdx.x, gridDim.x) : (int)blockIdx.x;
#define QG_KQ_ABLK(g) A + (long)g * 9
#define QG_KQ_OUT(m) C[m * ldc + row]
#include "qg_q4k_gemv_body.inc"
#undef QG_KQ_OUT
#undef QG_KQ_ABLK
#undef QG_KQ_DECLARE_TILE
}

// instantiation choice, launch and eligibility: qg_kq_launch.hpp
struct q4k_gemv_fmt {
    static constexpr int REC_ELEMS = SB_ELEMS, REC_DW = Q4K_REC_DW, UNIT = 64;
    static constexpr uintptr_t WMASK = 15;  // the 16-B loads
    template <int MT, int LPR, int WGS, bool SUMI, bool ONE> static auto kernel() {
        return q4k_gemv_kernel<MT, LPR, WGS, SUMI, ONE>;
    }
    static void describe(const GemmArgs& g, int MT, int LPR, int WGS, int one, int grid, size_t lds) {
        describe_kernel(g, "q4k_gemv MT=%d LPR=%d WGS=%d ONE=%d NT=%d grid=%d lds=%zu", MT, LPR, WGS, one, QG_Q4K_NT, grid,
                        lds);
    }
};

}  // namespace

bool q4k_gemv_eligible(const GemmArgs& g) { return kq_gemv_eligible<q4k_gemv_fmt>(g); }
hipError_t launch_q4k_gemv(const GemmArgs& g, hipStream_t st) { return kq_gemv_launch<q4k_gemv_fmt>(g, st); }

}  // namespace qg
