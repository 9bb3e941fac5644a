// qg_mxfp4_gemv.hip — the MXFP4 decode GEMV (M <= 8 activation rows), family "mxfp4_gemv".
//
// C[m * ldc + n] = sum_b (d_a * scale(e)) * float(sumi),  sumi = sum_j kv[code_j] * a_j   (qg_mxfp4.hpp)
//
// Work decomposition:
//  * A lane's unit is one block (MXFP4_UB = 1; two per unit lost the A/B, qg_mxfp4.hpp): 32 elements, 17 bytes, K / 32
//    units per row. LPR lanes share a weight row and stride
//    over its units, the next one in flight while the current one computes; 64 / LPR rows per wave. Lanes per row,
//    workgroup size and the loop-free form come from the K-quant ladder (kq_gemv_form_units, qg_kq_launch.hpp) keyed on
//    K / 32: 64 lanes and 1024 threads from 64 blocks on, 16 and 512 from 16 on, 4 and 256 below; ONE where no lane
//    owns a second block.
//  * Loads (qg_mxfp4.hpp, mxfp4_load): a block starts at (row * K/32 + b) * 17 bytes past a pointer of any alignment.
//    The lane reads the five aligned dwords that cover the block and realigns them with v_alignbyte by the address's
//    low two bits. No load is issued at an address that is not a multiple of 4, and every one of the five dwords holds
//    a byte of the lane's own block: there is NO read past the tensor, not even inside the last dword's page (Q6_K has
//    one such dword; this format has none). Neighbouring lanes read neighbouring blocks, so a wave's request is one
//    contiguous run of 17 LPR bytes per row.
//  * Codebook (mxfp4_kv4): v_perm_b32 over the table dwords 0x03020100 / 0x0C080604 with code & 7 as the selector gives
//    the magnitudes, the same over the negated table the negatives, and a third v_perm takes each byte from the one or
//    the other by the code's sign bit. Decoded once per unit into eight int8 dwords and reused by every token:
//    8 v_dot4_i32_i8 per token and block, elements 0..15 (low nibbles) against the block's first four activation
//    dwords, 16..31 (high nibbles) against the last four.
//  * The workgroup stages the M activation rows once into LDS, one thread per Q8_1 block: per (token, block) the 8 qs
//    dwords, d_a as fp32, 3 pad dwords (12 = 4 x odd). The stored sum s_a is not used.
//  * acc += (d_a * scale(e)) * float(sumi): two rounded multiplications and one rounded addition per block, in that
//    order. scale(e) is built from its bits (mxfp4_scale), subnormal for e < 2.
//  * Per-lane partials (unit order) are reduced across the row's LPR lanes with DPP row ops (group_sum_last), fixed
//    order: two launches give identical bits. Tolerance: W = 0.
//  * XCD-aware tile order on grids of one dispatch round (xcd_tile), as the row GEMV.
//  * SUMI: the same instantiation stores sumi in place of the epilogue.
#include "qg_kq_launch.hpp"
#include "qg_mxfp4.hpp"

namespace qg {
namespace {

// The body is qg_mxfp4_gemv_body.inc, shared as text with the expert-indexed launch (qg_moe.hip).
template <int MT, int LPR, int WGS, bool SUMI, bool ONE>
__global__ __launch_bounds__(WGS) void mxfp4_gemv_kernel(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                        int M, int N, int K, void* __restrict__ out, long ldc) {
#define QG_KQ_DECLARE_TILE const int tile = gridDim.x <= 512 ? xcd_tile(blockIdx.x, gridDim.x) : (int)blockIdx.x;
#define QG_KQ_ABLK(g) A + (long)g * 9
#define QG_KQ_OUT(m) C[m * ldc + row]
#include "qg_mxfp4_gemv_body.inc"
#undef QG_KQ_OUT
#undef QG_KQ_ABLK
#undef QG_KQ_DECLARE_TILE
}

// instantiation choice, launch and eligibility: qg_kq_launch.hpp
struct mxfp4_gemv_fmt {
    static constexpr int REC_ELEMS = QK, REC_DW = MXFP4_REC_DW, UNIT = QK * MXFP4_UB;
    static constexpr uintptr_t WMASK = 0;  // any byte: every load is realigned
    template <int MT, int LPR, int WGS, bool SUMI, bool ONE> static auto kernel() {
        return mxfp4_gemv_kernel<MT, LPR, WGS, SUMI, ONE>;
    }
    static void describe(const GemmArgs& g, int MT, int LPR, int WGS, int one, int grid, size_t lds) {
        describe_kernel(g, "mxfp4_gemv MT=%d LPR=%d WGS=%d ONE=%d grid=%d lds=%zu", MT, LPR, WGS, one, grid, lds);
    }
};

}  // namespace

bool mxfp4_gemv_eligible(const GemmArgs& g) { return kq_gemv_eligible<mxfp4_gemv_fmt>(g); }
hipError_t launch_mxfp4_gemv(const GemmArgs& g, hipStream_t st) { return kq_gemv_launch<mxfp4_gemv_fmt>(g, st); }

}  // namespace qg
