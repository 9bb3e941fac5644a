// qg_q4k.hpp — Q4_K (ggml type 12) building blocks shared by the decode GEMV (qg_q4k_gemv.hip), the MFMA
// prefill (qg_q4k_mmq.hip) and the dequantizer (qg_quantize.hip). Launch and eligibility: qg_kq_launch.hpp.
//
// block_q4_K (include/qg/blocks.h), 144 B = 36 dwords, 256 elements:
//   dword 0      f16 d | f16 dmin << 16
//   dwords 1..3  scales[12]: eight 6-bit scales sc[0..7] and eight 6-bit mins m[0..7]
//   dwords 4..35 qs[128]: chunk i = 0..3 is dwords 4 + 8i .. 4 + 8i + 7; the low nibble of byte l of the chunk
//                is element l of sub-block 2i, the high nibble element l of sub-block 2i + 1
// Sub-block j of super-block sb meets activation block 8 sb + j. The product ("Q4_K"):
//   C(m, n) = sum_sb [ d * sum_j d_a * float(sc_j * sumi_j)  -  dmin * sum_j float(m_j) * s_a ]
// sc_j * sumi_j is below 2^24 in magnitude, so the int -> float conversion is exact.
#pragma once
#include "qg_common.hpp"
#include "qg_kernels.hpp"

namespace qg {

constexpr int Q4K_BYTES = 144;
constexpr int Q4K_DW = 36;

// The eight scales and eight mins of one super-block, four bytes per dword:
//   sc[0] = sc 0..3, sc[1] = sc 4..7, mn[0] = m 0..3, mn[1] = m 4..7.
struct q4k_scales {
    uint32_t sc[2], mn[2];
};
__host__ __device__ __forceinline__ q4k_scales q4k_unpack_scales(uint32_t u0, uint32_t u1, uint32_t u2) {
    q4k_scales r;
    r.sc[0] = u0 & 0x3F3F3F3Fu;
    r.mn[0] = u1 & 0x3F3F3F3Fu;
    r.sc[1] = (u2 & 0x0F0F0F0Fu) | ((u0 >> 2) & 0x30303030u);
    r.mn[1] = ((u2 >> 4) & 0x0F0F0F0Fu) | ((u1 >> 2) & 0x30303030u);
    return r;
}
// byte J (0..7) of a two-dword group
template <int J> __host__ __device__ __forceinline__ int q4k_byte(const uint32_t (&v)[2]) {
    return (int)((v[J / 4] >> (8 * (J % 4))) & 0xFFu);
}

// Decode GEMV (M <= 8): see qg_q4k_gemv.hip. LDS per (token, super-block): 64 qs dwords, 8 x (d_a, s_a) fp32,
// 4 pad dwords (84 = 4 x odd: the 16-B reads of lanes on consecutive super-blocks hit distinct bank groups).
constexpr int Q4K_REC_DW = 84;
constexpr int Q4K_UNIT_DW = 12;  // a lane's unit: header (4) + one chunk's qs (8)

// Weight loads: plain, as the row GEMV's product instantiations (NT = false there). 1 (A/B builds): the
// nontemporal hint, measured slower on every decode shape — M = 1, N = K = 4096: 4.00 us with it, 3.50 without;
// K = 14336: 10.26 against 8.30 (profiles/q4k/ab_q4k_variants.txt).
#ifndef QG_Q4K_NT
#define QG_Q4K_NT 0
#endif
template <class T> __device__ __forceinline__ T q4k_wload(const T* p) {
    if constexpr (QG_Q4K_NT) return __builtin_nontemporal_load(p);
    else return *p;
}

// MFMA prefill (M >= 9): see qg_q4k_mmq.hip. The activation staging in LDS.
constexpr int Q4K_TOK_DW = 72;               // one token's 8 blocks of a super-block: 288 B
constexpr int Q4K_TILE_DW = 16 * Q4K_TOK_DW;  // a 16-token tile: 1152 dwords

// Shape / pointer rules of the two families (K % 256 == 0 and the alignments are checked by the C-ABI first).
bool q4k_gemv_eligible(const GemmArgs& g);
hipError_t launch_q4k_gemv(const GemmArgs& g, hipStream_t st);
bool q4k_mmq_eligible(const GemmArgs& g);
hipError_t launch_q4k_mmq(const GemmArgs& g, hipStream_t st);
// nsb super-blocks -> 256 * nsb floats, y = (d * sc) * q - dmin * m (qg_quantize.hip)
hipError_t launch_dequantize_q4k(const void* x, float* y, int64_t nsb, hipStream_t st);

}  // namespace qg
