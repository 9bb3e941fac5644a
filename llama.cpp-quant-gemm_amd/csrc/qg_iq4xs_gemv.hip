// qg_iq4xs_gemv.hip — the IQ4_XS decode GEMV (M <= 8 activation rows), family "iq4xs_gemv".
//
// C[m * ldc + n] = sum_sb d * sum_j d_a * float((ls_j - 32) * sumi_j),  sumi_j = sum_i kv[code_i] * a_i  (qg_iq4xs.hpp)
//
// Work decomposition:
//  * A lane's unit is 64 elements of a super-block: its 8-B header (d, scales_h, scales_l) and the 32 qs bytes of
//    sub-blocks 2i and 2i + 1, five global_load_dwordx2 at multiples of 8 (a super-block is 136 = 8 x 17 bytes, so 8 is
//    all a row guarantees). K / 64 units per row put the type on the K-quant ladder unchanged (kq_gemv_form,
//    qg_kq_launch.hpp): LPR lanes share a weight row and stride over its units, the next one in flight while the
//    current one computes; 64 / LPR rows per wave; ONE where no lane owns a second unit (K = 4096: a wave per row).
//  * Codebook (iq4xs_kv4): per qs dword v, kv4(v) is the int8 operand of elements i .. i + 3 of the sub-block and
//    kv4(v >> 4) that of elements 16 + i .. 16 + i + 3: three v_perm_b32 per four codes. A byte never straddles two
//    sub-blocks, so each sub-block's eight operand dwords line up with its activation block's eight dwords. Decoded
//    once per unit and reused by every token: 16 v_dot4_i32_i8 per token and unit.
//  * The two 6-bit scales of the unit are cut out of the header dwords with shifts and masks (no byte loads).
//  * The workgroup stages the M activation rows once into LDS, one thread per Q8_1 block: per (token, super-block)
//    the 8 blocks' qs dwords (64), their d_a as fp32 (8), 4 pad dwords (IQ4XS_REC_DW = 76, qg_iq4xs.hpp). The stored
//    sums are not used.
//  * (ls_j - 32) * sumi_j in int32 (below 2^24: the conversion is exact); fd = d_a0 * float(..) + d_a1 * float(..),
//    acc += d * fd: d is applied once per unit.
//  * Per-lane partials (unit order) are reduced across the row's LPR lanes with DPP row ops (group_sum_last),
//    fixed order: two launches give identical bits. Tolerance: W = 0.
//  * XCD-aware tile order on grids of one dispatch round (xcd_tile), as the row GEMV.
//  * SUMI: the same instantiation stores each sub-block's int32 dot in place of the epilogue.
#include "qg_iq4xs.hpp"
#include "qg_kq_launch.hpp"

namespace qg {
namespace {

// The body is qg_iq4xs_gemv_body.inc, shared as text with the expert-indexed launch (qg_moe.hip).
template <int MT, int LPR, int WGS, bool SUMI, bool ONE>
__global__ __launch_bounds__(WGS) void iq4xs_gemv_kernel(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                        int M, int N, int K, void* __restrict__ out, long ldc) {
#define QG_KQ_DECLARE_TILE const int tile = gridDim.x <= 512 ? xcd_tile(blockIdx.x, gridDim.x) : (int)blockIdx.x;
#define QG_KQ_ABLK(g) A + (long)g * 9
#define QG_KQ_OUT(m) C[m * ldc + row]
#include "qg_iq4xs_gemv_body.inc"
#undef QG_KQ_OUT
#undef QG_KQ_ABLK
#undef QG_KQ_DECLARE_TILE
}

// instantiation choice, launch and eligibility: qg_kq_launch.hpp
struct iq4xs_gemv_fmt {
    static constexpr int WT = QG_TYPE_IQ4_XS;
    template <int MT, int LPR, int WGS, bool SUMI, bool ONE> static auto kernel() {
        return iq4xs_gemv_kernel<MT, LPR, WGS, SUMI, ONE>;
    }
};

}  // namespace

bool iq4xs_gemv_eligible(const GemmArgs& g) { return kq_gemv_eligible<iq4xs_gemv_fmt>(g); }
hipError_t launch_iq4xs_gemv(const GemmArgs& g, hipStream_t st) { return kq_gemv_launch<iq4xs_gemv_fmt>(g, st); }

}  // namespace qg
