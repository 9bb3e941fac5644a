// qg_q6k_gemv.hip — the Q6_K decode GEMV (M <= 8 activation rows), family "q6k_gemv".
//
// C[m * ldc + n] = sum_sb d * sum_b d_a * float(scales[2b] * s0 + scales[2b + 1] * s1)   (qg_q6k.hpp)
//
// Work decomposition ("Q6_K"):
//  * A lane's unit is 64 elements: the Q8_1 blocks c = par and c = par + 2 of half h of a super-block, whole. Unit
//    u = 4 sb + 2h + par, K / 64 units per row, as q4k_gemv. It reads ql[64h + 32 par ..+31] (whose low nibbles are
//    block par, whose high nibbles block par + 2), qh[32h ..+31], the half's 8 scales (of which it uses bytes 2 par,
//    2 par + 1, 2 par + 4, 2 par + 5 = groups 8h + 2c, 8h + 2c + 1) and d. The four lanes of a super-block read its
//    128 ql bytes as one contiguous run; the lanes par = 0, 1 read the same qh bytes (one request). LPR lanes share a
//    weight row and stride over its units, the next one in flight while the current one computes; 64 / LPR rows per
//    wave. (The first version split a half by l-range instead, 16 bytes of each plane per lane, 13 payload dwords:
//    a block's two scale groups then sit in neighbouring lanes and isum needs a cross-lane add. It was slower on
//    every decode shape, 4.86 against 4.64 us at M = 1, N = K = 4096; profiles/q6k/ab_q6k_units.txt.)
//  * Loads (qg_q6k.hpp, q6k_load): a super-block starts at (row * K/256 + sb) * 210 bytes past a 2-B aligned
//    pointer, so every piece is 0 or 2 bytes off a dword and the parity varies per lane. Each piece is read as the
//    dword-aligned span that covers it, one dword more than its length, and realigned with v_alignbyte by the
//    address's low bits. No load is issued at an address that is not a multiple of 4. The extra dword of the ql
//    piece (bytes < 132 of the super-block), of the qh piece (< 196) and of the scales of half 0 still lies inside
//    the super-block; the extra dword of the scales of half 1 holds d (bytes 208..209); d itself is the one dword
//    at (sb + 208) & ~3. So every loaded dword holds a byte of the tensor; only the last super-block's d dword at
//    parity 0 is half outside it, in the same page. This is by construction; no test probes it.
//  * With l, h one dword of the ql and qh pieces, the unsigned codes (0..63 per byte) are
//      block par:      (l & 0x0F0F0F0F) | ((h << (4 - 2 par)) & 0x30303030)
//      block par + 2:  ((l >> 4) & 0x0F0F0F0F) | ((h >> (2 par)) & 0x30303030)
//    (the four forms c = 0..3 of DESIGN.md, two per lane), turned into signed bytes q - 32 once per unit,
//    ((u | 0x80808080) - 0x20202020) ^ 0x80808080, and reused by every token: 8 v_dot4_i32_i8 per block, s0 over the
//    block's first four activation dwords, s1 over the last four. (QG_Q6K_ASUM, A/B builds: the dot on the unsigned
//    codes and 32 x the activations' 16-element sums, exact integers staged with the record, subtracted per token:
//    identical bits, faster at M = 1 and slower at M = 8 by 3-4 %; profiles/q6k/ab_q6k_sub32.txt.)
//  * The workgroup stages the M activation rows once into LDS, one thread per Q8_1 block: per (token, super-block)
//    the 8 blocks' qs dwords (64), then their d_a as fp32 (8), 4 pad dwords.
//  * isum = scales[2b] * s0 + scales[2b + 1] * s1 in int32, inside the lane, before the conversion (the halves can
//    cancel; the contract's bound is relative to |d d_a isum|): fd = d_a * float(isum) + d_a' * float(isum'),
//    acc += d * fd.
//  * Per-lane partials (unit order) are reduced across the row's LPR lanes with DPP row ops (group_sum_last), fixed
//    order: two launches give identical bits. Tolerance: W = 0 — a lane-serial accumulation of at most K/32
//    terms per output (each lane chains its own blocks, then log2(LPR) pairwise sums), no extra partial sums.
//  * XCD-aware tile order on grids of one dispatch round (xcd_tile), as the row GEMV.
//  * SUMI: the same instantiation stores isum in place of the epilogue.
#include "qg_kq_launch.hpp"
#include "qg_q6k.hpp"

namespace qg {
namespace {

// The body is qg_q6k_gemv_body.inc, shared as text with the MoE launches (qg_moe.hip, qg_moe_batch.hip).
template <int MT, int LPR, int WGS, bool SUMI, bool ONE>
__global__ __launch_bounds__(WGS) void q6k_gemv_kernel(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                      int M, int N, int K, void* __restrict__ out, long ldc) {
#define QG_KQ_DECLARE_TILE const int tile = gridDim.x <= 512 ? xcd_tile(blockIdx.x, gridDim.x) : (int)blockIdx.x;
#define QG_KQ_ABLK(g) A + (long)g * 9
#define QG_KQ_OUT(m) C[m * ldc + row]
#include "qg_q6k_gemv_body.inc"
#undef QG_KQ_OUT
#undef QG_KQ_ABLK
#undef QG_KQ_DECLARE_TILE
}

// instantiation choice, launch and eligibility: qg_kq_launch.hpp
struct q6k_gemv_fmt {
    static constexpr int REC_ELEMS = SB_ELEMS, REC_DW = Q6K_REC_DW, UNIT = 64;
    static constexpr uintptr_t WMASK = 1;  // every load is realigned
    template <int MT, int LPR, int WGS, bool SUMI, bool ONE> static auto kernel() {
        return q6k_gemv_kernel<MT, LPR, WGS, SUMI, ONE>;
    }
    static void describe(const GemmArgs& g, int MT, int LPR, int WGS, int one, int grid, size_t lds) {
        describe_kernel(g, "q6k_gemv MT=%d LPR=%d WGS=%d ONE=%d grid=%d lds=%zu", MT, LPR, WGS, one, grid, lds);
    }
};

}  // namespace

bool q6k_gemv_eligible(const GemmArgs& g) { return kq_gemv_eligible<q6k_gemv_fmt>(g); }
hipError_t launch_q6k_gemv(const GemmArgs& g, hipStream_t st) { return kq_gemv_launch<q6k_gemv_fmt>(g, st); }

}  // namespace qg
