// qg_q3k_gemv.hip — the Q3_K decode GEMV (M <= 8 activation rows; QG_ALGO_AUTO sends it M <= 6), family "q3k_gemv".
//
// C[m * ldc + n] = sum_sb d * sum_b d_a * float(isum_b),  isum_b = s_2b * sum_{l<16} q a + s_2b+1 * sum_{l>=16} q a
// (qg_q3k.hpp)
//
// Work decomposition:
//  * A lane's unit is 64 elements of a super-block: the Q8_1 blocks 4h + par and 4h + par + 2 (h = half, par = 0 / 1).
//    Both come out of the same 32 qs bytes (bit pairs par and par + 2 of qs[32h ..]) and the same 32 hmask bytes (bits
//    4h + par and 4h + par + 2), so a unit is those two spans plus scales[12] and d: whole blocks, and the lane owns each
//    block's isum. K / 64 units per row put the type on the K-quant ladder unchanged (kq_gemv_form, qg_kq_launch.hpp):
//    LPR lanes share a weight row and stride over its units, the next one in flight while the current one computes;
//    64 / LPR rows per wave; ONE where no lane owns a second unit (K = 4096: a wave per row).
//  * Loads: three q6k_load spans (9 + 9 + 4 aligned dwords), realigned by the super-block's address parity.
//  * Per unit, once: the four 6-bit scales of the unit's groups out of the scale dwords, their tables T[u] = (4 - u) s
//    (q3k_table_lo / _hi: a multiply and four bit operations each), the codes u = lo2 | hb << 2 (two shifts, two masks,
//    an or per four codes) and one v_perm_b32 per four codes: sixteen dwords of pre-scaled int8 weights, reused by every
//    token.
//  * Per token: eight v_dot4_i32_i8 per block in ONE chain (the scales are in the operand: no s0 / s1 split and no
//    integer multiplies), negated once: isum. d_a from the LDS record, d applied once per unit.
//  * The workgroup stages the M activation rows once into LDS, one thread per Q8_1 block: per (token, super-block) the
//    8 blocks' qs dwords (64), their d_a as fp32 (8), 4 pad dwords (Q3K_REC_DW = 76). The stored sums are not used.
//  * Per-lane partials (unit order) are reduced across the row's LPR lanes with DPP row ops (group_sum_last), fixed
//    order: two launches give identical bits. Tolerance: W = 0.
//  * XCD-aware tile order on grids of one dispatch round (xcd_tile), as the row GEMV.
//  * SUMI: the same instantiation stores each block's isum in place of the epilogue.
#include "qg_q3k.hpp"
#include "qg_kq_launch.hpp"

namespace qg {
namespace {

// The body is qg_q3k_gemv_body.inc, shared as text with the expert-indexed launch (qg_moe.hip).
template <int MT, int LPR, int WGS, bool SUMI, bool ONE>
__global__ __launch_bounds__(WGS) void q3k_gemv_kernel(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                      int M, int N, int K, void* __restrict__ out, long ldc) {
#define QG_KQ_DECLARE_TILE const int tile = gridDim.x <= 512 ? xcd_tile(blockIdx.x, gridDim.x) : (int)blockIdx.x;
#define QG_KQ_ABLK(g) A + (long)g * 9
#define QG_KQ_OUT(m) C[m * ldc + row]
#include "qg_q3k_gemv_body.inc"
#undef QG_KQ_OUT
#undef QG_KQ_ABLK
#undef QG_KQ_DECLARE_TILE
}

// instantiation choice, launch and eligibility: qg_kq_launch.hpp
struct q3k_gemv_fmt {
    static constexpr int WT = QG_TYPE_Q3_K;
    template <int MT, int LPR, int WGS, bool SUMI, bool ONE> static auto kernel() {
        return q3k_gemv_kernel<MT, LPR, WGS, SUMI, ONE>;
    }
};

}  // namespace

bool q3k_gemv_eligible(const GemmArgs& g) { return kq_gemv_eligible<q3k_gemv_fmt>(g); }
hipError_t launch_q3k_gemv(const GemmArgs& g, hipStream_t st) { return kq_gemv_launch<q3k_gemv_fmt>(g, st); }

}  // namespace qg
