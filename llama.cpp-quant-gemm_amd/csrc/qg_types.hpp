// qg_types.hpp — the one table of weight types: what a type is (id, block geometry), what its kernels need (weight
// alignment, the decode GEMV's LDS record and unit, the largest M AUTO sends to that GEMV) and which entries take it.
// qg_api.hip, qg_kq_launch.hpp, qg_moe*.hip, qg_gguf.hip, the constants of qg_<type>.hpp and host/qg_host.cpp ask here.
// Plain C++, no HIP type. weight_type(id) is constexpr and returns a row by value: device code takes its numbers as
// constant expressions (a template argument, a constexpr local) and never reads the array at run time.
#pragma once
#include <stdint.h>

#include "../../include/qg/qg.h"

namespace qg {

// The largest M QG_ALGO_AUTO sends to a routed type's decode GEMV; beyond it, and wherever the GEMV's LDS records do
// not fit, the MFMA prefill. (A/B builds override one with -DQG_<TYPE>_GEMV_MAXM=...; the GEMV can be forced up to 8.)
//   Q4_K   8: interleaved A/B against 4 | 5 (profiles/q4k/ab_q4k_variants.txt, N = K = 4096): M = 5 GEMV 5.82 us, MFMA
//             7.43; M = 8 GEMV 7.31, MFMA 7.45. Q6_K keeps the threshold ("Q6_K", 3b).
//   MXFP4  8: profiles/mxfp4/ab_mxfp4_threshold.txt, each kernel forced: M = 5 GEMV 5.95 us, MFMA 12.04; M = 8 GEMV
//             6.99, MFMA 12.08.
//   IQ4_XS 8: profiles/iq4xs/ab_iq4xs_threshold.txt, each kernel forced.
//   Q3_K   6: profiles/q3k/ab_q3k_threshold.txt, each kernel forced: M = 5 GEMV 6.06 us, MFMA 6.56; M = 6 6.46 / 6.55;
//             M = 7 7.24 / 6.58; M = 8 7.56 / 6.59, each beyond the rounds' spread: its prefill needs one MFMA per
//             block and so starts cheaper than the others' (DESIGN.md 3l).
#ifndef QG_Q4K_GEMV_MAXM
#define QG_Q4K_GEMV_MAXM 8
#endif
#ifndef QG_Q6K_GEMV_MAXM
#define QG_Q6K_GEMV_MAXM 8
#endif
#ifndef QG_MXFP4_GEMV_MAXM
#define QG_MXFP4_GEMV_MAXM 8
#endif
#ifndef QG_IQ4XS_GEMV_MAXM
#define QG_IQ4XS_GEMV_MAXM 8
#endif
#ifndef QG_Q3K_GEMV_MAXM
#define QG_Q3K_GEMV_MAXM 6
#endif
#ifndef QG_Q6K_ASUM  // (and two A/B knobs that size a record or a unit: qg_q6k.hpp, qg_mxfp4.hpp)
#define QG_Q6K_ASUM 0
#endif
#ifndef QG_MXFP4_UNIT_BLOCKS
#define QG_MXFP4_UNIT_BLOCKS 1
#endif

// The entry classes (include/qg/qg.h says the same in prose, entry by entry).
enum : unsigned {
    IN_PRODUCT = 1,      // the products that take the routed types (qg_gemm_w4a8, _ex, _ldc, _f32, _from_view, the sumi hook)
    IN_MOE = 2,          // qg_gemm_w4a8_moe
    IN_MOE_PLAIN = 4,    // qg_gemm_w4a8_moe_prefill, _moe_batch, _moe_glu, _moe_down
    IN_MOE_BIAS = 8,     // the four _bias entries, qg_gemm_w4a8_moe_glu_batch
    IN_QUANTIZE = 16,    // qg_quantize
    IN_DEQUANTIZE = 32,  // qg_dequantize
    IN_GGUF = 64,        // the GGUF reader serves it (another known type stays listed with nbytes == 0)
};

struct WeightType {
    int id;
    const char* family;  // "q4k" + "_gemv" / "_mmq" in the config lines; "" for the 32-element types
    int bytes, elems;    // a block
    // routed: kernels, a K granule (elems) and a weight alignment of its own; the 32-element weight types share theirs,
    // and an entry that does not take a routed type refuses it as any other type, at the 32-element granule.
    bool routed;
    uintptr_t wmask;    // routed: the low bits of a weights pointer (and of an expert stride) that must be 0
    uintptr_t dq_mask;  // the same for qg_dequantize's input
    int rec_elems, rec_dw, unit;  // decode GEMV: elements and dwords of an LDS record, elements of a lane's unit
    int gemv_maxm;
    unsigned entries;
};

constexpr unsigned IN_ROWS = IN_PRODUCT | IN_MOE | IN_QUANTIZE | IN_DEQUANTIZE | IN_GGUF;
constexpr unsigned IN_ROUTED = IN_PRODUCT | IN_MOE | IN_DEQUANTIZE;
// Weight alignment: Q4_K's 144-B super-blocks are read with 16-B loads (the dequantizer reads bytes); a Q6_K super-block
// is 210 B, so its fp16 field's 2 B is all a row guarantees and the kernels realign every load; a Q3_K super-block is
// 110 B, 2 mod 4 likewise; an IQ4_XS super-block is 136 = 8 x 17 B and is read with 8-B loads; an MXFP4 block is 17 B
// of bytes, so there is no requirement at all.
// Records: a token's super-block (Q4_K: 84 dwords; Q6_K: 76, or 92 with the half-block sums of QG_Q6K_ASUM; IQ4_XS and
// Q3_K: 76), a lane's unit 64 of its elements; MXFP4: a block (12 dwords), a unit QG_MXFP4_UNIT_BLOCKS blocks.
constexpr WeightType WEIGHT_TYPES[] = {
    {QG_TYPE_Q4_0, "", 18, 32, false, 1, 1, 0, 0, 0, 0, IN_ROWS},
    {QG_TYPE_Q4_1, "", 20, 32, false, 1, 1, 0, 0, 0, 0, IN_ROWS},
    {QG_TYPE_Q5_0, "", 22, 32, false, 1, 1, 0, 0, 0, 0, IN_ROWS},
    {QG_TYPE_Q5_1, "", 24, 32, false, 1, 1, 0, 0, 0, 0, IN_ROWS},
    {QG_TYPE_Q8_0, "", 34, 32, false, 1, 1, 0, 0, 0, 0, IN_ROWS},
    {QG_TYPE_Q8_1, "", 36, 32, false, 1, 1, 0, 0, 0, 0, IN_QUANTIZE | IN_DEQUANTIZE | IN_GGUF},  // activations
    {QG_TYPE_Q3_K, "q3k", 110, 256, true, 1, 1, 256, 76, 64, QG_Q3K_GEMV_MAXM, IN_ROUTED | IN_GGUF},
    {QG_TYPE_Q4_K, "q4k", 144, 256, true, 15, 1, 256, 84, 64, QG_Q4K_GEMV_MAXM, IN_ROUTED | IN_MOE_PLAIN | IN_MOE_BIAS | IN_GGUF},
    {QG_TYPE_Q6_K, "q6k", 210, 256, true, 1, 1, 256, QG_Q6K_ASUM ? 92 : 76, 64, QG_Q6K_GEMV_MAXM, IN_ROUTED | IN_MOE_PLAIN | IN_MOE_BIAS},
    {QG_TYPE_IQ4_XS, "iq4xs", 136, 256, true, 7, 7, 256, 76, 64, QG_IQ4XS_GEMV_MAXM, IN_ROUTED | IN_GGUF},
    {QG_TYPE_MXFP4, "mxfp4", 17, 32, true, 0, 0, 32, 12, 32 * QG_MXFP4_UNIT_BLOCKS, QG_MXFP4_GEMV_MAXM, IN_ROUTED | IN_MOE_BIAS | IN_GGUF},
};
constexpr int N_WEIGHT_TYPES = sizeof(WEIGHT_TYPES) / sizeof(WEIGHT_TYPES[0]);

// the row's index (qg_api.hip's ROUTES runs parallel), -1 for an id the table does not have
constexpr int weight_type_index(int id) {
    for (int i = 0; i < N_WEIGHT_TYPES; ++i)
        if (WEIGHT_TYPES[i].id == id) return i;
    return -1;
}
// the row of an id; an unknown id gets a row of zeros that no entry takes
constexpr WeightType weight_type(int id) {
    const int i = weight_type_index(id);
    return i < 0 ? WeightType{id, "", 0, 0, false, 0, 0, 0, 0, 0, 0, 0} : WEIGHT_TYPES[i];
}
constexpr bool type_in(int id, unsigned entry_class) { return (weight_type(id).entries & entry_class) != 0; }

// One activation row's decode-GEMV LDS records (K is a multiple of rec_elems) and its units (rounded up: MXFP4's alone can be partial)
constexpr size_t kq_row_lds_bytes(int wtype, int K) {
    const WeightType w = weight_type(wtype);
    return (size_t)(K / w.rec_elems) * w.rec_dw * 4;
}
constexpr int kq_row_units(int wtype, int K) {
    const WeightType w = weight_type(wtype);
    return (K + w.unit - 1) / w.unit;
}

}  // namespace qg
