// qg_q6k.hpp — Q6_K (ggml type 14) building blocks shared by the decode GEMV (qg_q6k_gemv.hip), the MFMA
// prefill (qg_q6k_mmq.hip) and the dequantizer (qg_quantize.hip). Launch and eligibility: qg_kq_launch.hpp.
//
// block_q6_K (include/qg/blocks.h), 210 B, 256 elements:
//   bytes   0..127  ql[128]    low 4 bits of the codes
//   bytes 128..191  qh[64]     high 2 bits of the codes
//   bytes 192..207  scales[16] int8, one per 16 elements
//   bytes 208..209  f16 d
// Element e: h = e / 128, p = e % 128, c = p / 32, l = p % 32;
//   q = ((ql[64h + 32(c & 1) + l] >> 4(c >> 1)) & 15 | ((qh[32h + l] >> 2c) & 3) << 4) - 32,  scale g = 8h + 2c + l / 16.
// Q8_1 block b = 4h + c of super-block sb (activation block 8 sb + b) meets exactly the scale groups 2b (l < 16)
// and 2b + 1 (l >= 16). The product ("Q6_K"):
//   isum = scales[2b] * s0 + scales[2b + 1] * s1   (int32, |isum| <= 2^24: the conversion to float is exact)
//   C(m, n) = sum_sb d * sum_b d_a * float(isum)
//
// 210 is a multiple of 2 but not of 4: super-blocks (and rows with odd K / 256) alternate between 0 and 2 bytes off
// dword alignment, and the weights pointer itself need only be 2-B aligned. Every weight load in the Q6_K kernels
// goes through q6k_load below: the dword-aligned span that covers a piece, realigned with v_alignbyte by the
// address's low bits (the form of qg_ragged.hip). No load is issued at an address that is not a multiple of 4, and
// every loaded dword holds at least one byte of the tensor: each piece's span is chosen (see the callers) so that
// its last dword still holds a byte of the piece's own super-block. The one dword that can reach past the tensor
// is the last super-block's d at parity 0 (bytes 208..211 of 210): half of it is tensor, so it is in the same page.
#pragma once
#include "qg_common.hpp"
#include "qg_kernels.hpp"

namespace qg {

constexpr int Q6K_BYTES = 210;
constexpr int Q6K_QH = 128, Q6K_SC = 192, Q6K_D = 208;  // field offsets

// NDW dwords of a byte stream that starts at the 2-B aligned address p: NDW + 1 aligned dwords from p & ~3 (pa below),
// realigned by p & 3 (0 or 2). The caller guarantees that the dword at (p & ~3) + 4 NDW holds a byte of the tensor.
template <int NDW> __device__ __forceinline__ void q6k_load(const uint8_t* p, uint32_t (&raw)[NDW + 1]) {
    // (p minus its low bits, not an integer round trip: the pointer stays a global one)
    const uint32_t* pa = static_cast<const uint32_t*>(__builtin_assume_aligned(p - ((uintptr_t)p & 3), 4));
#pragma unroll
    for (int i = 0; i <= NDW; ++i) raw[i] = pa[i];
}
template <int NDW> __device__ __forceinline__ void q6k_realign(const uint32_t (&raw)[NDW + 1], uint32_t sh, uint32_t (&w)[NDW]) {
#pragma unroll
    for (int i = 0; i < NDW; ++i) w[i] = __builtin_amdgcn_alignbyte(raw[i + 1], raw[i], sh);
}

// Four unsigned 6-bit codes (0..63, one per byte) -> the signed codes q - 32 as int8 bytes, without carries
// between the bytes: bit 7 set guards the subtraction, then restored by the xor.
__device__ __forceinline__ uint32_t q6k_sub32(uint32_t u) { return ((u | 0x80808080u) - 0x20202020u) ^ 0x80808080u; }

// The code dword of block c (0..3) of a half from a dword of ql[64h + ..], ql[64h + 32 + ..] and qh[32h + ..].
template <int C> __device__ __forceinline__ uint32_t q6k_codes(uint32_t a, uint32_t b, uint32_t h) {
    const uint32_t lo = ((C & 1) ? b : a) >> (4 * (C >> 1));
    const uint32_t hi = C == 0 ? h << 4 : C == 1 ? h << 2 : C == 2 ? h : h >> 2;
    return q6k_sub32((lo & 0x0F0F0F0Fu) | (hi & 0x30303030u));
}

// QG_Q6K_ASUM (A/B builds): how the decode GEMV takes the 32 off the codes. 0: per byte, once per unit (q6k_sub32).
// 1: the dot runs on the unsigned codes and 32 x the activations' sum over the 16 elements, an exact integer staged
// with the LDS record, is subtracted per token.
#ifndef QG_Q6K_ASUM
#define QG_Q6K_ASUM 0
#endif
__device__ __forceinline__ uint32_t q6k_signed(uint32_t u) { return QG_Q6K_ASUM ? u : q6k_sub32(u); }

// Decode GEMV (M <= 8): see qg_q6k_gemv.hip. LDS per (token, super-block): the 8 blocks' qs dwords (64), their d_a
// as fp32 (8), with QG_Q6K_ASUM the 16 half-block sums x 32 (16), 4 pad dwords (76 / 92 = 4 x odd: the 16-B reads
// of lanes on consecutive super-blocks hit distinct bank groups).
constexpr int Q6K_REC_DW = QG_Q6K_ASUM ? 92 : 76;
// raw dwords of a unit: the ql and qh pieces (9 each: 32 bytes + the realignment dword), the half's scales (3), d (1)
constexpr int Q6K_UNIT_DW = 22;

// MFMA prefill (M >= 9): see qg_q6k_mmq.hip. The activation staging in LDS.
constexpr int Q6K_TOK_DW = 72;               // one token's 8 blocks of a super-block: 288 B
constexpr int Q6K_TILE_DW = 16 * Q6K_TOK_DW;  // a 16-token tile: 1152 dwords

// byte J (0..15) of a 16-byte group held in four dwords, sign extended
template <int J> __device__ __forceinline__ int q6k_scale(const uint32_t (&v)[4]) {
    return (int)(int8_t)(v[J / 4] >> (8 * (J % 4)));
}

// Shape / pointer rules of the two families (K % 256 == 0 and the alignments are checked by the C-ABI first).
bool q6k_gemv_eligible(const GemmArgs& g);
hipError_t launch_q6k_gemv(const GemmArgs& g, hipStream_t st);
bool q6k_mmq_eligible(const GemmArgs& g);
hipError_t launch_q6k_mmq(const GemmArgs& g, hipStream_t st);
// nsb super-blocks -> 256 * nsb floats, y = (d * float(scale)) * float(q) (qg_quantize.hip)
hipError_t launch_dequantize_q6k(const void* x, float* y, int64_t nsb, hipStream_t st);

}  // namespace qg
