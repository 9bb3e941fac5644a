// qg_q3k.hpp — Q3_K (ggml type 11) building blocks shared by the decode GEMV (qg_q3k_gemv.hip), the MFMA prefill
// (qg_q3k_mmq.hip), the expert-indexed GEMV (qg_moe.hip) and the dequantizer (qg_quantize.hip). Launch and
// eligibility: qg_kq_launch.hpp.
//
// block_q3_K (include/qg/blocks.h), 110 B, 256 elements:
//   bytes   0..31   hmask[32]   the codes' high bit (set: no 4 is subtracted)
//   bytes  32..95   qs[64]      the codes' low 2 bits
//   bytes  96..107  scales[12]  sixteen 6-bit scales
//   bytes 108..109  f16 d
// Element e = 128h + 32j + l (h 0..1, j 0..3, l 0..31):
//   u = ((qs[32h + l] >> 2j) & 3) | ((hmask[l] >> (4h + j)) & 1) << 2      (0..7)
//   q = u - 4  (-4..3),  scale group g = 8h + 2j + l / 16,  s_g = sc_g - 32  (-32..31)
// Q8_1 block b = 4h + j of super-block sb (activation block 8 sb + b) meets exactly the groups 2b (l < 16) and 2b + 1.
//   isum_b = s_{2b} * sum_{l < 16} q a + s_{2b+1} * sum_{l >= 16} q a     (int32, |isum| <= 32 * 32 * 4 * 128 = 2^19)
//   C(m, n) = sum_sb d * sum_b d_a(8 sb + b) * float(isum_b)
// There is no min term: the activation block's stored sum is not used.
//
// The pre-scaled operand. (-q) * s = (4 - u) * s lies in [-128, 124]: q * s reaches (-4) * (-32) = +128, which is no
// int8, while its negation is; at the other end 4 * 31 = 124. So the 16-element scale is folded into the int8 operand
// before the dot: per group an eight-entry table T[u] = (4 - u) * s in two dwords, and one v_perm_b32 with four u bytes
// as the selector gives four pre-scaled weights. The dot over a whole Q8_1 block is then -isum_b, exact in int32.
//
// 110 is a multiple of 2 but not of 4: super-blocks (and rows with odd K / 256) alternate between 0 and 2 bytes off
// dword alignment, and the weights pointer itself need only be 2-B aligned. Every weight load goes through q6k_load
// (qg_q6k.hpp): the dword-aligned span that covers a piece, realigned with v_alignbyte by the address's low bits. No
// load is issued at an address that is not a multiple of 4, and every loaded dword holds at least one byte of the
// tensor: a span's first dword holds the piece's first two bytes, its last one a byte of the piece's own super-block
// (the scales' span ends in the dword of d, bytes 108..111 at parity 0: half of it is tensor, so it is in the same
// page). The bytes outside are shifted out by the realignment; no result depends on them.
#pragma once
#include "qg_common.hpp"
#include "qg_kernels.hpp"
#include "qg_types.hpp"
#include "qg_q6k.hpp"

namespace qg {

constexpr int Q3K_BYTES = weight_type(QG_TYPE_Q3_K).bytes;
constexpr int Q3K_QS = 32, Q3K_SC = 96;  // field offsets (hmask at 0; d follows the scales: one span holds both)

// The sixteen 6-bit scales sc_g (0..63, the bias of 32 still on) from the three dwords of scales[12], four per dword:
// sc[i] holds groups 4i .. 4i + 3. Low nibbles of bytes 0..7 are groups 0..7, their high nibbles groups 8..15; bit pair
// i of byte 8 + g % 4 is the high part of group 4i + g % 4. Dword operations alone.
struct q3k_scales {
    uint32_t sc[4];
};
__host__ __device__ __forceinline__ constexpr q3k_scales q3k_unpack_scales(uint32_t s0, uint32_t s1, uint32_t s2) {
    q3k_scales r = {};
    r.sc[0] = (s0 & 0x0F0F0F0Fu) | ((s2 << 4) & 0x30303030u);
    r.sc[1] = (s1 & 0x0F0F0F0Fu) | ((s2 << 2) & 0x30303030u);
    r.sc[2] = ((s0 >> 4) & 0x0F0F0F0Fu) | (s2 & 0x30303030u);
    r.sc[3] = ((s1 >> 4) & 0x0F0F0F0Fu) | ((s2 >> 2) & 0x30303030u);
    return r;
}

// The table of a group with the biased scale p = sc_g (0..63; s = p - 32): T[u] = (4 - u) * s as int8, entries 0..3 in
// the bytes of lo, 4..7 in those of hi. One multiply spreads k * p over the bytes (k * p <= 252: no carries), and the
// bias k * 32 comes off per byte without borrows between them (bit 7 guards the subtraction and is put right by the xor).
//   lo bytes: 4p - 128, 3p - 96, 2p - 64, p - 32        hi bytes: 0, 32 - p, 64 - 2p, 96 - 3p
__host__ __device__ __forceinline__ constexpr uint32_t q3k_table_lo(uint32_t p) {
    const uint32_t x = p * 0x01020304u;
    return ((x | 0x80808080u) - 0x20406000u) ^ ((x ^ 0x80808000u) & 0x80808080u);
}
__host__ __device__ __forceinline__ constexpr uint32_t q3k_table_hi(uint32_t p) {
    const uint32_t y = p * 0x03020100u;
    return (0xE0C0A080u - (y & 0x7F7F7F7Fu)) ^ (~y & 0x80808080u);
}
// exact for all 64 scales x 8 codes, (-(-4)) * (-32) = -128 included
constexpr bool q3k_table_exact() {
    for (int p = 0; p < 64; ++p)
        for (int u = 0; u < 8; ++u) {
            const uint32_t t = u < 4 ? q3k_table_lo((uint32_t)p) : q3k_table_hi((uint32_t)p);
            const int want = (4 - u) * (p - 32);
            if (want < -128 || want > 127) return false;
            if (((t >> (8 * (u & 3))) & 0xFFu) != (uint32_t)(want & 0xFF)) return false;
        }
    return true;
}
static_assert(q3k_table_exact(), "T[u] = (4 - u) * (sc - 32) for every scale and code");
static_assert(q3k_table_lo(0) == 0xE0C0A080u && q3k_table_hi(63) == 0xA3C2E100u, "the table dwords, little endian");

// Four codes u (0..7, one per byte) -> four pre-scaled int8 weights (4 - u) * s: selector 0..3 reads the second operand.
__device__ __forceinline__ uint32_t q3k_lookup(uint32_t u, uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, u); }

// Decode GEMV (M <= 8, M <= 6 by QG_ALGO_AUTO): see qg_q3k_gemv.hip. Raw dwords of a unit: the half's 32 qs bytes and the 32 hmask bytes
// (9 each: 8 + the realignment dword), scales[12] with d behind them (4).
constexpr int Q3K_UNIT_DW = 22;
// LDS per (token, super-block): the 8 blocks' qs dwords (64), their d_a as fp32 (8), 4 pad dwords: 76 = 4 x 19, and 19
// is odd, so the 16-B reads of lanes on consecutive super-blocks start in distinct bank groups (as Q6_K's record).
constexpr int Q3K_REC_DW = weight_type(QG_TYPE_Q3_K).rec_dw;

// MFMA prefill (M >= 7): see qg_q3k_mmq.hip. The activation staging in LDS, as the other prefills'.
constexpr int Q3K_TOK_DW = 72;                // one token's 8 blocks of a super-block: 288 B
constexpr int Q3K_TILE_DW = 16 * Q3K_TOK_DW;  // a 16-token tile: 1152 dwords
// Partial sums the prefill chains per output beyond its K/32 terms (the W of the contract's bound). An output is the
// sum of KS <= 8 K-slice partials; a slice partial is ONE fma chain over the 8 blocks of each of its super-blocks,
// acc = fma((-d) * d_a, float(c), acc): at most 8 * ceil(K/256 / KS) <= K/32 roundings (ceil(n / KS) <= n), and the
// coefficient's own rounding is one of the bound's "+ 2". Then KS - 1 <= 7 slice additions.
constexpr int Q3K_MMQ_W = 7;

// Shape / pointer rules of the two families (K % 256 == 0 and the alignments are checked by the C-ABI first).
bool q3k_gemv_eligible(const GemmArgs& g);
hipError_t launch_q3k_gemv(const GemmArgs& g, hipStream_t st);
bool q3k_mmq_eligible(const GemmArgs& g);
hipError_t launch_q3k_mmq(const GemmArgs& g, hipStream_t st);
// nsb super-blocks -> 256 * nsb floats, y = (d * float(sc - 32)) * float(q) (qg_quantize.hip)
hipError_t launch_dequantize_q3k(const void* x, float* y, int64_t nsb, hipStream_t st);

}  // namespace qg
