/*
 * qg/blocks.h — byte-exact llama.cpp block formats (C and C++, host and device).
 *
 * These are the on-HBM layouts the W4A8 path consumes. They are re-declared here as plain
 * POD structs with the fp16 fields stored as raw uint16_t bit patterns, so the header builds
 * with gcc, g++ and hipcc alike and carries no cuda_fp16/hip_fp16 dependency.
 *
 * Reference layouts (byte-identical):
 *   block_q4_0  18 B  include/quant_types.h:59-64   (compat/ggml_types.h:62-67)
 *   block_q8_0  34 B  include/quant_types.h:85-90
 *   block_q8_1  36 B  include/quant_types.h:116-121 (compat/ggml_types.h:186-191)
 *   block_q4_1  20 B  compat/ggml_types.h:90-96
 *   block_q5_0  22 B  compat/ggml_types.h:111-117
 *   block_q5_1  24 B  compat/ggml_types.h:125-132
 *   block_q4_K 144 B  ggml's K-quant (the reference defines only QK_K = 256 and the type id)
 *   block_q6_K 210 B  ggml's K-quant (likewise)
 *
 * Nibble packing (include/quantize.h:56-67): qs[j] low nibble = x[j], high nibble = x[j+16].
 * Q5 fifth bit (tests/framework/test_framework.cuh:309-325): bit i of the little-endian u32
 * qh holds bit 4 of element i.
 * Q8_1 ds = {d, s} as half2: d = amax/127, s = Σx of the ORIGINAL floats
 * (include/quantize.h:165-193).
 */
#ifndef QG_BLOCKS_H
#define QG_BLOCKS_H

#include <stdint.h>

#define QG_QK 32 /* elements per block, every format on this path */

typedef struct {
    uint16_t d;      /* fp16 scale */
    uint8_t qs[16];  /* 32 x u4, value = (q - 8) * d */
} qg_block_q4_0;

typedef struct {
    uint16_t d;      /* fp16 scale */
    uint16_t m;      /* fp16 min, value = q * d + m */
    uint8_t qs[16];
} qg_block_q4_1;

typedef struct {
    uint16_t d;      /* fp16 scale, value = (q - 16) * d, q in [0, 31] */
    uint8_t qh[4];   /* bit 4 of each element */
    uint8_t qs[16];  /* low 4 bits */
} qg_block_q5_0;

typedef struct {
    uint16_t d;
    uint16_t m;      /* value = q * d + m */
    uint8_t qh[4];
    uint8_t qs[16];
} qg_block_q5_1;

typedef struct {
    uint16_t d;
    int8_t qs[32];
} qg_block_q8_0;

typedef struct {
    uint16_t d;      /* ds.x: fp16 scale */
    uint16_t s;      /* ds.y: fp16 sum of the original values */
    int8_t qs[32];
} qg_block_q8_1;

/* ggml's block_q4_K: a super-block of 256 elements = 8 sub-blocks of 32.
 *   scales[12]: eight 6-bit scales sc[0..7] and eight 6-bit mins m[0..7]:
 *     j <  4: sc[j] = q[j] & 63                             m[j] = q[j+4] & 63
 *     j >= 4: sc[j] = (q[j+4] & 15) | ((q[j-4] >> 6) << 4)  m[j] = (q[j+4] >> 4) | ((q[j] >> 6) << 4)
 *   qs[128]: chunk i = 0..3 covers elements 64i .. 64i+63; for l = 0..31
 *     element 64i + l = qs[32i + l] & 15 (sub-block 2i), element 64i + 32 + l = qs[32i + l] >> 4 (sub-block 2i+1)
 *   value of element e of sub-block j = d * sc[j] * q_e - dmin * m[j] */
#define QG_QK_K 256
typedef struct {
    uint16_t d;          /* fp16 scale of the sub-block scales */
    uint16_t dmin;       /* fp16 scale of the sub-block mins */
    uint8_t scales[12];
    uint8_t qs[128];
} qg_block_q4_K;

/* ggml's block_q6_K: a super-block of 256 elements = 16 groups of 16 with signed 8-bit scales, 6-bit codes split
 * over a nibble plane and a 2-bit plane, no min term. For element e: h = e / 128, p = e % 128, c = p / 32, l = p % 32,
 *   lo = (ql[64h + 32(c & 1) + l] >> (4 (c >> 1))) & 15,  hi = (qh[32h + l] >> (2c)) & 3,  q = (lo | hi << 4) - 32
 *   value = d * scales[8h + 2c + l / 16] * q
 * 210 bytes: a multiple of 2, not of 4 -- consecutive super-blocks alternate between 0 and 2 bytes off a dword. */
typedef struct {
    uint8_t ql[128];     /* low 4 bits of the codes */
    uint8_t qh[64];      /* high 2 bits of the codes */
    int8_t scales[16];   /* one per 16 elements */
    uint16_t d;          /* fp16 scale of the group scales */
} qg_block_q6_K;

/* ggml's block_mxfp4 (type 39): 32 elements, an E8M0 scale byte and 4-bit E2M1 codes in the Q4_0 nibble order:
 *   element j (0..15) has the code qs[j] & 15, element j + 16 the code qs[j] >> 4
 *   value = kv[code] * 2^(e - 128),  kv[16] = {0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12}
 * (the doubled E2M1 values, hence 128 and not 127; code 8 is the integer 0). 17 bytes, alignment 1: blocks, rows and
 * expert matrices start at any byte. */
typedef struct {
    uint8_t e;       /* E8M0: the scale 2^(e - 128), fp32 bits e < 2 ? 0x00200000 << e : (e - 1) << 23 */
    uint8_t qs[16];
} qg_block_mxfp4;

#ifdef __cplusplus
static_assert(sizeof(qg_block_mxfp4) == 17 && alignof(qg_block_mxfp4) == 1, "block_mxfp4 must be 17 bytes, alignment 1");
static_assert(sizeof(qg_block_q4_K) == 144, "block_q4_K must be 144 bytes");
static_assert(sizeof(qg_block_q6_K) == 210, "block_q6_K must be 210 bytes");
static_assert(sizeof(qg_block_q4_0) == 18, "block_q4_0 must be 18 bytes");
static_assert(sizeof(qg_block_q4_1) == 20, "block_q4_1 must be 20 bytes");
static_assert(sizeof(qg_block_q5_0) == 22, "block_q5_0 must be 22 bytes");
static_assert(sizeof(qg_block_q5_1) == 24, "block_q5_1 must be 24 bytes");
static_assert(sizeof(qg_block_q8_0) == 34, "block_q8_0 must be 34 bytes");
static_assert(sizeof(qg_block_q8_1) == 36, "block_q8_1 must be 36 bytes");
#else
_Static_assert(sizeof(qg_block_mxfp4) == 17 && _Alignof(qg_block_mxfp4) == 1, "block_mxfp4 must be 17 bytes, alignment 1");
_Static_assert(sizeof(qg_block_q4_K) == 144, "block_q4_K must be 144 bytes");
_Static_assert(sizeof(qg_block_q6_K) == 210, "block_q6_K must be 210 bytes");
_Static_assert(sizeof(qg_block_q4_0) == 18, "block_q4_0 must be 18 bytes");
_Static_assert(sizeof(qg_block_q4_1) == 20, "block_q4_1 must be 20 bytes");
_Static_assert(sizeof(qg_block_q5_0) == 22, "block_q5_0 must be 22 bytes");
_Static_assert(sizeof(qg_block_q5_1) == 24, "block_q5_1 must be 24 bytes");
_Static_assert(sizeof(qg_block_q8_0) == 34, "block_q8_0 must be 34 bytes");
_Static_assert(sizeof(qg_block_q8_1) == 36, "block_q8_1 must be 36 bytes");
#endif

#endif /* QG_BLOCKS_H */
