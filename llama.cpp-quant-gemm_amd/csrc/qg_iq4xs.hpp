// qg_iq4xs.hpp — IQ4_XS (ggml type 23) building blocks shared by the decode GEMV (qg_iq4xs_gemv.hip), the MFMA
// prefill (qg_iq4xs_mmq.hip), the expert-indexed GEMV (qg_moe.hip) and the dequantizer (qg_quantize.hip). Launch and
// eligibility: qg_kq_launch.hpp.
//
// block_iq4_xs (include/qg/blocks.h), 136 B = 34 dwords, 256 elements:
//   dword 0       f16 d | u16 scales_h << 16
//   dword 1       scales_l[4]
//   dwords 2..33  qs[128]: sub-block j = 0..7 is dwords 2 + 4j .. 2 + 4j + 3; the low nibble of byte i of the
//                 sub-block is element 32j + i, the high nibble element 32j + 16 + i (the Q4_0 / MXFP4 nibble order:
//                 no byte straddles two sub-blocks)
// The 6-bit scale of sub-block j: ls_j = ((scales_l[j/2] >> 4 (j%2)) & 15) | (((scales_h >> 2j) & 3) << 4).
// A 4-bit code indexes kv[16] = {-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113} (IQ4_NL's
// table). Sub-block j of super-block sb meets Q8_1 activation block 8 sb + j (qg.h, "IQ4_XS weights"):
//   sumi_j = sum_i kv[code_i] * a_i          (int32; |(ls_j - 32) * sumi_j| <= 32 * 32 * 127 * 128 < 2^24)
//   C(m, n) = sum_sb d * sum_j d_a(8 sb + j) * float((ls_j - 32) * sumi_j)
// The product by ls_j - 32 is formed in int32 and its conversion to float is exact. There is no min term: the
// activation block's stored sum is not used.
//
// 136 = 8 * 17: super-blocks alternate between 0 and 8 mod 16. Every weight load of the IQ4_XS kernels is 8 bytes at
// an 8-B aligned address inside its own super-block; nothing relies on more and nothing is read past the tensor.
#pragma once
#include "qg_common.hpp"
#include "qg_kernels.hpp"
#include "qg_types.hpp"

namespace qg {

constexpr int IQ4XS_BYTES = weight_type(QG_TYPE_IQ4_XS).bytes;
constexpr int IQ4XS_DW = 34;

// The codebook as four table dwords, entries 4t .. 4t + 3 in the bytes of IQ4XS_KV[t].
constexpr int IQ4XS_KV_VALUES[16] = {-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113};
constexpr uint32_t iq4xs_kv_dword(int t) {
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) r |= (uint32_t)(IQ4XS_KV_VALUES[4 * t + i] & 0xFF) << (8 * i);
    return r;
}
constexpr uint32_t IQ4XS_KV[4] = {iq4xs_kv_dword(0), iq4xs_kv_dword(1), iq4xs_kv_dword(2), iq4xs_kv_dword(3)};
static_assert(IQ4XS_KV[0] == 0xBFAD9881u && IQ4XS_KV[3] == 0x71594535u, "the table dwords, little endian");

// Four codes, one in the low nibble of each byte of x (the high nibbles are ignored) -> kv[code] as four int8 bytes,
// for a table of sixteen arbitrary int8 values T[0..3]: v_perm_b32 over the table's low half (T[0], T[1]) with
// code & 7 as the selector, the same over its high half, and a third v_perm that takes byte i from the one or the
// other by the code's bit 3. mxfp4_kv4's shape and cost without its sign trick; no arithmetic on packed bytes, so no
// carries between them.
__device__ __forceinline__ uint32_t kv4_lookup(uint32_t x, uint32_t t0, uint32_t t1, uint32_t t2, uint32_t t3) {
    const uint32_t t = x & 0x07070707u;
    const uint32_t lo = __builtin_amdgcn_perm(t1, t0, t);  // selector 0..3: the second operand
    const uint32_t hi = __builtin_amdgcn_perm(t3, t2, t);
    // selector of byte i: i (lo) or 4 + i (hi)
    return __builtin_amdgcn_perm(hi, lo, ((x >> 1) & 0x04040404u) | 0x03020100u);
}
__device__ __forceinline__ uint32_t iq4xs_kv4(uint32_t x) {
    return kv4_lookup(x, IQ4XS_KV[0], IQ4XS_KV[1], IQ4XS_KV[2], IQ4XS_KV[3]);
}

// The eight 6-bit scales of a super-block from its header dwords h0 = d | scales_h << 16 and h1 = scales_l, four
// bytes per dword: ls[0] = ls 0..3, ls[1] = ls 4..7 (the unbiased values 0..63; the kernels subtract 32). Dword
// operations alone: the nibbles of a half of scales_l and the bit pairs of a byte of scales_h are spread over four
// bytes by two shift-or-mask steps each.
struct iq4xs_scales {
    uint32_t ls[2];
};
__host__ __device__ __forceinline__ uint32_t iq4xs_spread(uint32_t l16, uint32_t h8) {
    uint32_t l = (l16 | (l16 << 8)) & 0x00FF00FFu;  // scales_l bytes 0, 1 -> bytes 0, 2
    l = (l | (l << 4)) & 0x0F0F0F0Fu;               // their nibbles -> bytes 0..3
    uint32_t h = (h8 | (h8 << 12)) & 0x000F000Fu;   // scales_h bit pairs 0, 1 -> byte 0, pairs 2, 3 -> byte 2
    h = (h | (h << 6)) & 0x03030303u;               // one pair per byte
    return l | (h << 4);
}
__host__ __device__ __forceinline__ iq4xs_scales iq4xs_unpack_scales(uint32_t h0, uint32_t h1) {
    iq4xs_scales r;
    r.ls[0] = iq4xs_spread(h1 & 0xFFFFu, (h0 >> 16) & 0xFFu);
    r.ls[1] = iq4xs_spread(h1 >> 16, h0 >> 24);
    return r;
}
// byte J (0..7) of the two dwords, minus the bias: ls_J - 32
template <int J> __host__ __device__ __forceinline__ int iq4xs_ls(const iq4xs_scales& s) {
    return (int)((s.ls[J / 4] >> (8 * (J % 4))) & 0xFFu) - 32;
}

// Decode GEMV (M <= 8): see qg_iq4xs_gemv.hip. A lane's unit is 64 elements: the 8-B header and the 32 qs bytes of
// sub-blocks 2i, 2i + 1, five 8-B loads. d is applied once per unit (per lane: its two sub-blocks' terms are summed
// first), so a lane's accumulator takes one rounded product by d and one rounded addition per unit.
constexpr int IQ4XS_UNIT_DW = 10;
// LDS per (token, super-block): the 8 blocks' qs dwords (64), their d_a as fp32 (8), 4 pad dwords. The stored sums
// are not kept. Lanes on consecutive units read 16-B pieces at dword offsets 16 i + 4 x of record u / 4: four
// consecutive lanes sweep one record's 64 qs dwords, i.e. every bank once, and the next four start 76 = 4 x 19 dwords
// on. 19 is odd, so the sixteen 16-B bank groups a quarter-wave's reads start in step through all residues before
// any repeats (72 = 4 x 18 would put records two apart on the same groups); the d_a pair of a unit is one 8-B read at
// 64 + 2i, which the same stride spreads likewise.
constexpr int IQ4XS_REC_DW = weight_type(QG_TYPE_IQ4_XS).rec_dw;

// MFMA prefill (M >= 9): see qg_iq4xs_mmq.hip. The activation staging in LDS, as the Q4_K / MXFP4 prefill's.
constexpr int IQ4XS_TOK_DW = 72;                   // one token's 8 blocks of a super-block: 288 B
constexpr int IQ4XS_TILE_DW = 16 * IQ4XS_TOK_DW;   // a 16-token tile: 1152 dwords
// Partial sums the prefill chains per output beyond its K/32 terms (the W of the contract's bound). An output is the
// sum of KS <= 8 K-slice partials; a slice partial is an fma chain over its super-blocks, acc = fma(d, inner, acc),
// and inner an fma chain over the super-block's 8 terms. A term therefore passes through at most 8 roundings in its
// super-block, one per super-block of its slice from its own on (at most ceil(K/256 / KS)) and KS - 1 slice
// additions: 8 + ceil(K/256 / KS) + KS - 1 <= K/32 + 8 for every K >= 256 and KS <= 8.
constexpr int IQ4XS_MMQ_W = 8;

// Shape / pointer rules of the two families (K % 256 == 0 and the alignments are checked by the C-ABI first).
bool iq4xs_gemv_eligible(const GemmArgs& g);
hipError_t launch_iq4xs_gemv(const GemmArgs& g, hipStream_t st);
bool iq4xs_mmq_eligible(const GemmArgs& g);
hipError_t launch_iq4xs_mmq(const GemmArgs& g, hipStream_t st);
// nsb super-blocks -> 256 * nsb floats, y = (d * float(ls - 32)) * float(kv[code]) (qg_quantize.hip)
hipError_t launch_dequantize_iq4xs(const void* x, float* y, int64_t nsb, hipStream_t st);

}  // namespace qg
