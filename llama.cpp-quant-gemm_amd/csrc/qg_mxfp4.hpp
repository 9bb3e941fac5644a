// qg_mxfp4.hpp — MXFP4 (ggml type 39) building blocks shared by the decode GEMV (qg_mxfp4_gemv.hip), the MFMA
// prefill (qg_mxfp4_mmq.hip) and the dequantizer (qg_quantize.hip). Launch and eligibility: qg_kq_launch.hpp.
//
// block_mxfp4 (include/qg/blocks.h), 17 B, 32 elements:
//   byte   0      e       E8M0 scale, 2^(e - 128)
//   bytes  1..16  qs[16]  element j = qs[j] & 15, element j + 16 = qs[j] >> 4 (the Q4_0 nibble order)
// A 4-bit code indexes kv[16] = {0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12}, the doubled E2M1 values
// (bit 3 the sign, code 8 the integer 0). The product with Q8_1 block b of the activation row (qg.h, "MXFP4 weights"):
//   sumi = sum_j kv[code_j] * a_j   (int32, |sumi| <= 32 * 12 * 128 < 2^24: the conversion to float is exact)
//   C(m, n) = sum_b (d_a * scale(e)) * float(sumi)
//
// 17 is odd: blocks, rows (K / 32 * 17 bytes) and expert matrices start at any byte. Every weight load in the MXFP4
// kernels reads dwords of the block's cover: a block at byte offset o lies in the aligned dwords o / 4 .. (o + 16) / 4,
// always exactly five, and each of them holds a byte of the block. The pieces are realigned with v_alignbyte by the
// address's low two bits (the form of q6k_load and qg_ragged.hip). No load is issued at an address that is not a
// multiple of 4, and, unlike Q6_K, no loaded dword lies outside its own block's cover: nothing is read past the tensor,
// not even by a byte's width. This is by construction; no test probes it.
#pragma once
#include "qg_common.hpp"
#include "qg_kernels.hpp"

namespace qg {

constexpr int MXFP4_BYTES = 17;
constexpr int MXFP4_COVER_DW = 5;  // aligned dwords that hold a block, whatever its address

// scale(e) = 2^(e - 128) from its fp32 bits: e = 0 and e = 1 are the subnormals 2^-128 and 2^-127, no NaN code
__host__ __device__ __forceinline__ uint32_t mxfp4_scale_bits(uint32_t e) { return e < 2 ? 0x00200000u << e : (e - 1) << 23; }
__device__ __forceinline__ float mxfp4_scale(uint32_t e) { return __uint_as_float(mxfp4_scale_bits(e)); }

// The first dword of block p's cover (p minus its low bits, not an integer round trip: the pointer stays a global one)
__device__ __forceinline__ const uint32_t* mxfp4_cover(const uint8_t* p) {
    return static_cast<const uint32_t*>(__builtin_assume_aligned(p - ((uintptr_t)p & 3), 4));
}
// NDW dwords of block p's cover, from its dword FIRST on (FIRST + NDW <= 5: all inside the cover)
template <int FIRST, int NDW> __device__ __forceinline__ void mxfp4_load(const uint8_t* p, uint32_t (&raw)[NDW]) {
    static_assert(FIRST >= 0 && FIRST + NDW <= MXFP4_COVER_DW, "inside the block's cover");
    const uint32_t* pa = mxfp4_cover(p);
#pragma unroll
    for (int i = 0; i < NDW; ++i) raw[i] = pa[FIRST + i];
}

// The dword of a byte stream held in (lo, hi) that starts sh = 1..4 bytes into lo (v_alignbyte takes 0..3: at 4 it is hi)
__device__ __forceinline__ uint32_t mxfp4_align(uint32_t lo, uint32_t hi, uint32_t sh) {
    const uint32_t a = __builtin_amdgcn_alignbyte(hi, lo, sh);
    return sh == 4 ? hi : a;
}

// Four codes, one in the low nibble of each byte of x (the high nibbles are ignored) -> kv[code] as four int8 bytes.
// The magnitudes come from v_perm_b32 over the two table dwords with code & 7 as the selector, their negations from the
// negated table; a third v_perm picks byte i from the one or the other by the code's bit 3. No arithmetic, so no
// carries between the bytes, and magnitude 0 stays 0 under the sign (code 8 is the integer 0).
__device__ __forceinline__ uint32_t mxfp4_kv4(uint32_t x) {
    const uint32_t t = x & 0x07070707u;
    const uint32_t mag = __builtin_amdgcn_perm(0x0C080604u, 0x03020100u, t);  // selector 0..3: the second operand
    const uint32_t neg = __builtin_amdgcn_perm(0xF4F8FAFCu, 0xFDFEFF00u, t);
    // selector of byte i: i (mag) or 4 + i (neg)
    return __builtin_amdgcn_perm(neg, mag, ((x >> 1) & 0x04040404u) | 0x03020100u);
}

// QG_MXFP4_UNIT_BLOCKS (A/B builds): consecutive blocks of a row a lane of the decode GEMV owns per unit, 1 (shipped)
// or 2: ten loads in flight per unit and a loop-free form up to K = 4096. Two: 3.97 against 3.94 us at M = 1,
// N = K = 4096, 7.90 against 6.84 at M = 8, 4.59 against 3.68 at 2880 x 2880 (profiles/mxfp4/ab_mxfp4_units.txt).
#ifndef QG_MXFP4_UNIT_BLOCKS
#define QG_MXFP4_UNIT_BLOCKS 1
#endif
constexpr int MXFP4_UB = QG_MXFP4_UNIT_BLOCKS;
constexpr int MXFP4_UNIT_DW = MXFP4_UB * MXFP4_COVER_DW;  // raw dwords of a unit: a cover per block

// Decode GEMV (M <= 8): see qg_mxfp4_gemv.hip. LDS per (token, block): the 8 qs dwords, d_a as fp32, 3 pad dwords
// (12 = 4 x odd: the 16-B reads of lanes on consecutive blocks hit distinct bank groups).
constexpr int MXFP4_REC_DW = 12;

// MFMA prefill (M >= 9): see qg_mxfp4_mmq.hip. The activation staging in LDS, by groups of 8 blocks as the super-block
// kernels' (the last group of a row may be partial).
constexpr int MXFP4_TOK_DW = 72;                  // one token's 8 blocks: 288 B
constexpr int MXFP4_TILE_DW = 16 * MXFP4_TOK_DW;  // a 16-token tile: 1152 dwords
// Partial sums the prefill chains per output beyond its K/32 terms (the W of the contract's bound): the K-slice
// partials of a workgroup, summed in slice order.
constexpr int MXFP4_MMQ_W = 8;

// Shape / pointer rules of the two families (K % 32 == 0 and the activations' alignment are checked by the C-ABI first).
bool mxfp4_gemv_eligible(const GemmArgs& g);
hipError_t launch_mxfp4_gemv(const GemmArgs& g, hipStream_t st);
bool mxfp4_mmq_eligible(const GemmArgs& g);
hipError_t launch_mxfp4_mmq(const GemmArgs& g, hipStream_t st);
// nblocks blocks -> 32 * nblocks floats, y = float(kv[code]) * scale(e) (qg_quantize.hip)
hipError_t launch_dequantize_mxfp4(const void* x, float* y, int64_t nblocks, hipStream_t st);

}  // namespace qg
