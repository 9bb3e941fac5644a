// qg_gemv_kernel.hpp — the W4A8 GEMV / small-batch kernels (M <= 8 activation rows).
//
// Included by qg_gemv.hip (the product's instantiations + dispatch) and by profiles/tools_archive/gemv_probe.hip
// (the tuning sweep). Computes, for the reference's activation-major contract
// C[M,N] = A_q8_1[M,K] . B_w[N,K]^T (include/gemm_reference.h:175-222):
//   C[m*ldc_m + n*ldc_n] = sum_b term(A[m][b], B[n][b]).
//
// Work decomposition:
//  * A lane owns "units" of BPL consecutive Q-blocks of one weight row (BPL*BB bytes, e.g. Q4_0
//    BPL=4 -> 72 B; 4 x dwordx4 + 1 x dwordx2). LPR lanes share a row and stride over its units
//    (the next unit in flight while the current one computes); 64/LPR rows per wave, WGS/64 waves
//    per workgroup.
//  * The workgroup stages the M activation rows once into LDS, one 12-dword record per Q8_1 block
//    (one thread per block; unit stride 12*BPL+4 dwords = 4 x odd, so the 16 lanes of a
//    ds_read_b128 group hit distinct bank slots). The first block's loads are issued before the
//    weight stream, so the staging waits only on them.
//  * Integer dot, exact int32 sumi, two forms:
//      - nibble planes (Q4_0, Q4_1 weights): each activation byte a = 16*h + l with h = a >> 4
//        (signed 4-bit) and l = a & 15; the record holds the l and h nibbles of elements
//        (4i+k, 16+4i+k) interleaved exactly like the weight nibbles of qs dword i, so one raw
//        weight dword q feeds v_dot8_u32_u4(q, l) and, XORed with 0x88888888 (= signed q - 8),
//        v_dot8_i32_i4(q^0x8.., h): sumi = L + 16*H + 128*sum(h), the last term (activation only)
//        folded into the accumulator's initial value. 8 dot8 + 4 XOR per block, no nibble
//        unpacking;
//      - bytes (Q5_0, Q5_1, Q8_0): blocks decoded in registers with compile-time
//        alignbyte/shift/mask (qg_common.hpp), 8 v_dot4c_i32_i8 per block.
//    Both accumulate on top of the bit pattern of 1.5*2^23, so the int32 result read as f32 is
//    1.5*2^23 + sumi (|sumi| < 2^22): no int->float convert.
//  * Per-block epilogue in the reference's operation order, so each block's fp32 term is
//    bit-identical to the CPU oracle's: fma(d_a, cf, -1.5*2^23*d_a) = round(d_a*sumi) (the
//    constant is exact), c*s_a precomputed in the record (exact: c is 8, 16 or 1), d_w (and m_w)
//    taken straight from the f16 bits by v_fma_mix_f32 with a zero addend (= one rounding of the
//    f32 product, as the reference's d_w * (...)).
//    tests/test_gpu_q32_extremes.py pins this over the whole finite f16 range (subnormal, negative, zero and
//    +-65504 d_a, s_a, d_w and m_w: v_fma_mix_f32 keeps f16 subnormal inputs on gfx950).
//  * Per-lane partials (unit order, block order) are reduced across the row's LPR lanes with DPP
//    row ops (group_sum_last); the row's last lane stores. Deterministic.
//  * AIN != 0 (fused activation quantization): A is FP32 (AIN_F32, quantized as
//    quantize_row_q8_1_ref) or FP16 (AIN_F16_FUSED, as kernels/gemm/gemm_fused.cuh:76-143) [M][K];
//    each thread quantizes whole 32-element blocks (qg_quant_block.hpp) and builds the same LDS
//    record, so every output is bit-identical to the two-step quantize + GEMV path.
//  * NT: the weight stream is loaded with the nontemporal hint (read once per launch).
// Tuning record (probes, per-wave timelines, rejected designs): profiles/r01_tuning/README.md.
#pragma once
#include <assert.h>

#include "qg_common.hpp"
#include "qg_group_affine.hpp"
#include "qg_kernels.hpp"
#include "qg_quant_block.hpp"

namespace qg {

constexpr uint32_t ACC_BIAS = 0x4B400000u;  // bits of 12582912.0f = 1.5 * 2^23
constexpr float ACC_BIAS_F = 12582912.0f;

// row tiles of a launch: N rows at rpw rows per workgroup (host: grid.x; device: the XCD-order test)
__host__ __device__ constexpr int gemv_tiles(int N, int rpw) { return (int)(((unsigned)N + (unsigned)rpw - 1u) / (unsigned)rpw); }

template <int F, int BPL> struct gemv_geom {
    static constexpr int BB = wfmt<F>::BB;
    static constexpr int UB = BPL * BB;          // unit bytes
    static constexpr int UDW = UB / 4;           // unit dwords (BB even, BPL even -> whole dwords)
    static constexpr int REC_DW = 12 * BPL + 4;  // LDS record dwords per (m, unit)
};

// Nibble-plane dot for Q4_0 / Q4_1 weights (see header).
template <int F> constexpr bool gemv_planes = F == FMT_Q4_0 || F == FMT_Q4_1;
// c in the record's c * s_a: Q4_0 -8 s_a, Q5_0 -16 s_a, Q4_1 / Q5_1 + m_w s_a, Q8_0 none.
template <int F> constexpr float gemv_cs = F == FMT_Q4_0 ? 8.0f : F == FMT_Q5_0 ? 16.0f : F == FMT_Q8_0 ? 0.0f : 1.0f;

// x * (f16 value in the low / high half of h), one rounding (v_fma_mix_f32 with a zero addend).
template <int HI> __device__ __forceinline__ float mixmul(uint32_t h, float x) {
    float r;
    if constexpr (HI) asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(x));
    else asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(x));
    return r;
}
// f16 field at compile-time byte offset OFF of a register-resident byte stream, times x.
template <int OFF> __device__ __forceinline__ float mixmul_at(const uint32_t* w, float x) {
    static_assert(OFF % 2 == 0, "fp16 fields are 2-byte aligned");
    return mixmul<(OFF % 4) / 2>(w[OFF / 4], x);
}

// The 12-dword LDS record of one Q8_1 block (b[0] = f16 d | f16 s << 16, b[1..8] = qs):
//   planes: [0..3] l nibbles, [4..7] h nibbles (element pairs (4i+k, 16+4i+k) at nibbles 2k, 2k+1
//           of dword i), [11] initial accumulator bits 1.5*2^23 + 128*sum(h);
//   bytes:  [0..7] qs;
//   both:   [8] d_a, [9] c * s_a, [10] -1.5*2^23 * d_a (fp32).
template <int F> __device__ __forceinline__ void build_act_record(const uint32_t* b, uint32_t (&r)[12]) {
    const float d = h2f(b[0] & 0xFFFFu), s = h2f(b[0] >> 16);
    if constexpr (gemv_planes<F>) {
        int sh = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t a0 = b[1 + i], a1 = b[5 + i];
            r[i] = (a0 & 0x0F0F0F0Fu) | ((a1 << 4) & 0xF0F0F0F0u);
            r[4 + i] = ((a0 >> 4) & 0x0F0F0F0Fu) | (a1 & 0xF0F0F0F0u);
            sh = __builtin_amdgcn_sdot8((int)r[4 + i], 0x11111111, sh, false);
        }
        r[11] = ACC_BIAS + (uint32_t)(128 * sh);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) r[i] = b[1 + i];
        r[11] = ACC_BIAS;
    }
    r[8] = __float_as_uint(d);
    r[9] = __float_as_uint(gemv_cs<F> * s);
    r[10] = __float_as_uint(-(d * ACC_BIAS_F));
}
template <int F> __device__ __forceinline__ void make_act_record(const uint32_t (&b)[9], uint32_t* rec) {
    uint32_t r[12];
    build_act_record<F>(b, r);
    *reinterpret_cast<uint4*>(rec) = make_uint4(r[0], r[1], r[2], r[3]);
    *reinterpret_cast<uint4*>(rec + 4) = make_uint4(r[4], r[5], r[6], r[7]);
    *reinterpret_cast<uint4*>(rec + 8) = make_uint4(r[8], r[9], r[10], r[11]);
}

// Biased int32 dot (bits of 1.5*2^23 + sumi) of block BI of a register-resident unit with its
// activation record.
template <int F, int BI> __device__ __forceinline__ uint32_t block_dot(const uint32_t* w, const uint4 (&a)[3]) {
    using T = wfmt<F>;
    constexpr int base = BI * T::BB;
    if constexpr (gemv_planes<F>) {
        const uint32_t l[4] = {a[0].x, a[0].y, a[0].z, a[0].w};
        const uint32_t h[4] = {a[1].x, a[1].y, a[1].z, a[1].w};
        uint32_t L = a[2].w;
        int H = 0;
        static_for<4>([&](auto I) {
            constexpr int i = decltype(I)::value;
            const uint32_t q = ld32<base + T::QS + 4 * i>(w);
            L = __builtin_amdgcn_udot8(q, l[i], L, false);
            H = __builtin_amdgcn_sdot8((int)(q ^ 0x88888888u), (int)h[i], H, false);
        });
        return L + ((uint32_t)H << 4);
    } else {
        const wblock wb = decode_block<F, BI>(w);
        const uint32_t av[8] = {a[0].x, a[0].y, a[0].z, a[0].w, a[1].x, a[1].y, a[1].z, a[1].w};
        int s = (int)ACC_BIAS;
#pragma unroll
        for (int i = 0; i < 8; ++i) s = __builtin_amdgcn_sdot4((int)wb.q[i], (int)av[i], s, false);
        return (uint32_t)s;
    }
}

// The reference's per-block term from the biased dot (see header).
template <int F, int BI> __device__ __forceinline__ float block_term_rec(const uint32_t* w, uint32_t acc, const uint4& sc) {
    using T = wfmt<F>;
    constexpr int base = BI * T::BB;
    const float cf = __uint_as_float(acc);
    const float da = __uint_as_float(sc.x), cs = __uint_as_float(sc.y), nda = __uint_as_float(sc.z);
    if constexpr (F == FMT_Q4_0 || F == FMT_Q5_0) {
        const float t1 = __builtin_fmaf(da, cf, nda);  // d_a * sumi
        return mixmul_at<base>(w, t1 - cs);             // d_w * (d_a * sumi - c * s_a)
    } else if constexpr (F == FMT_Q8_0) {
        return mixmul_at<base>(w, __builtin_fmaf(da, cf, nda));  // (sumi * d_a) * d_w
    } else {
        const float fs = cf - ACC_BIAS_F;                             // exact: sumi
        const float t = mixmul_at<base>(w, da) * fs;                  // (d_w * d_a) * sumi
        return t + mixmul_at<base + T::MOFF>(w, cs);                  // + m_w * s_a
    }
}

// ------------------------------------------------------------------------------------------------
// Weight units on the tiled layout (LAY_TILED / LAY_TILED_ACT; tiled_fmt in qg_common.hpp), round 6: the
// decode GEMV of qg_gemvt.hip. A lane's unit is BPL = 4 blocks (one stage) of ONE weight row — the same bytes
// as a 4-block unit of the row layout, gathered from the stage run's planes: per k-slot q one 16-B piece of
// the row's QS plane entry (dword q of the 4 blocks), its qh dwords (Q5_x) and its f16 scales. In registers
// (UDW dwords, as the row layout's unit):
//   [b * QSD + i]  qs dword i of block b (QSD = 4; Q8_0 8: half 1 = dwords 4..7)
//   [OQH + b]      qh of block b (Q5_0 / Q5_1)
//   [OD + b / 2]   f16 d of blocks b (low half: even b)      [OM + b / 2] f16 m (Q4_1 / Q5_1)
// so every block's fields sit at compile-time register indices: no alignbyte, no address arithmetic.
template <int F, int BPL> struct gemvt_unit {
    using T = wfmt<F>;
    static constexpr int QSD = T::Q8 ? 8 : 4;
    static constexpr int OQH = BPL * QSD;
    static constexpr int OD = OQH + (T::QH >= 0 ? BPL : 0);
    static constexpr int OM = OD + BPL / 2;
    static constexpr int UDW = OM + (T::MOFF >= 0 ? BPL / 2 : 0);
    static_assert(UDW * 4 == BPL * T::BB, "the unit holds exactly its blocks' bytes");
};

template <int F, int BI, int BPL> __device__ __forceinline__ wblock decode_block_t(const uint32_t* w) {
    using T = wfmt<F>;
    using U = gemvt_unit<F, BPL>;
    wblock r;
    r.d = r.m = 0.0f;  // (the dot needs the codes only)
    if constexpr (T::Q8) {
#pragma unroll
        for (int i = 0; i < 8; ++i) r.q[i] = w[BI * 8 + i];
        return r;
    }
    uint32_t qh = 0;
    if constexpr (T::QH >= 0) qh = w[U::OQH + BI];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t v = w[BI * 4 + i];
        uint32_t lo = v & 0x0F0F0F0Fu, hi = (v >> 4) & 0x0F0F0F0Fu;
        if constexpr (T::QH >= 0) {
            lo |= spread4_bit4((qh >> (4 * i)) & 0xFu);
            hi |= spread4_bit4((qh >> (16 + 4 * i)) & 0xFu);
        }
        r.q[i] = lo;
        r.q[4 + i] = hi;
    }
    return r;
}

// block_dot / block_term_rec of a tiled-layout unit (same arithmetic, same results bit for bit)
template <int F, int BI, int BPL> __device__ __forceinline__ uint32_t block_dot_t(const uint32_t* w, const uint4 (&a)[3]) {
    if constexpr (gemv_planes<F>) {
        const uint32_t l[4] = {a[0].x, a[0].y, a[0].z, a[0].w};
        const uint32_t h[4] = {a[1].x, a[1].y, a[1].z, a[1].w};
        uint32_t L = a[2].w;
        int H = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t q = w[BI * 4 + i];
            L = __builtin_amdgcn_udot8(q, l[i], L, false);
            H = __builtin_amdgcn_sdot8((int)(q ^ 0x88888888u), (int)h[i], H, false);
        }
        return L + ((uint32_t)H << 4);
    } else {
        const wblock wb = decode_block_t<F, BI, BPL>(w);
        const uint32_t av[8] = {a[0].x, a[0].y, a[0].z, a[0].w, a[1].x, a[1].y, a[1].z, a[1].w};
        int s = (int)ACC_BIAS;
#pragma unroll
        for (int i = 0; i < 8; ++i) s = __builtin_amdgcn_sdot4((int)wb.q[i], (int)av[i], s, false);
        return (uint32_t)s;
    }
}
template <int F, int BI, int BPL> __device__ __forceinline__ float block_term_t(const uint32_t* w, uint32_t acc, const uint4& sc) {
    using U = gemvt_unit<F, BPL>;
    const float cf = __uint_as_float(acc);
    const float da = __uint_as_float(sc.x), cs = __uint_as_float(sc.y), nda = __uint_as_float(sc.z);
    const uint32_t dw = w[U::OD + BI / 2];
    if constexpr (F == FMT_Q4_0 || F == FMT_Q5_0) {
        return mixmul<BI & 1>(dw, __builtin_fmaf(da, cf, nda) - cs);
    } else if constexpr (F == FMT_Q8_0) {
        return mixmul<BI & 1>(dw, __builtin_fmaf(da, cf, nda));
    } else {
        const float fs = cf - ACC_BIAS_F;
        const float t = mixmul<BI & 1>(dw, da) * fs;
        return t + mixmul<BI & 1>(w[U::OM + BI / 2], cs);
    }
}

// ------------------------------------------------------------------------------------------------
// Load the 32 activation values of block g (AIN_F32: 128 B, AIN_F16_FUSED: 64 B; 16-B aligned).
template <int AIN> __device__ __forceinline__ void load_act_block(const uint8_t* __restrict__ X, int g, float (&v)[32]) {
    if constexpr (AIN == AIN_F32) {
        const float4* p = reinterpret_cast<const float4*>(X) + (long)g * 8;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float4 t = p[i];
            v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
        }
    } else {
        const uint4* p = reinterpret_cast<const uint4*>(X) + (long)g * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint4 t = p[i];
            const uint32_t w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[8 * i + 2 * j] = h2f(w[j] & 0xFFFFu);
                v[8 * i + 2 * j + 1] = h2f(w[j] >> 16);
            }
        }
    }
}

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
typedef uint32_t u32x8_a16 __attribute__((ext_vector_type(8), aligned(16)));
// a device-memory pointer from its two dwords
template <class T> __device__ __forceinline__ T* global_ptr(uint32_t lo, uint32_t hi) {
    typedef T __attribute__((address_space(1))) * G;
    return (T*)(G)((uint64_t)lo | (uint64_t)hi << 32);
}

// PRE: read the unit's LDS records into registers right after the staging barrier, before the
// first weight byte is used, so the LDS latency overlaps the weight stream and only VALU work
// remains once the weights land (MT <= 2: 12 * BPL * MT dwords of registers).
// ONEU > 1 (round 5): every lane owns at most ONEU units (K <= 32 * BPL * LPR * ONEU), all their weight loads
// issued before the activation staging, no unit loop: ONEU units of weights in flight per lane instead of the
// loop's two (the published K = 14336 decode shapes, VERDICT r04 missing #1).
// ONEU == 1: every lane owns at most one unit (K <= 32 * BPL * LPR): the kernel has no unit loop, so the
// waits for the weight loads sit at their first use, behind the record reads (with a loop in the
// kernel, hipcc's wait insertion falls back to vmcnt(0) before the first record read).
// Argument order: everything the first loads need (A, B, their batch strides, M, N, K) sits in the
// first 14 dwords, which the dispatch preloads into SGPRs (-amdgpu-kernarg-preload-count, Makefile);
// the rest (output pointer and strides, the sumi hook) is fetched by an s_load that is only waited
// for at the store, so no kernarg fetch sits in front of the weight stream.
// (The round-1..4 ablation bits and timeline stamps used to decompose this kernel live in
// profiles/tools_archive/qg_gemv_kernel_r04_knobs.hpp, not here.)
// The kernel body is shared by two entry points (below): the general one and the M = 1 one with the
// minimal argument list.
// TPW (tiles per workgroup, loop-free form only): the workgroup computes TPW consecutive row tiles of
// one product — the activations are staged and their records read ONCE for all of them, and every
// tile's weight unit is in flight before the staging barrier. Each row's arithmetic is unchanged, so
// outputs are bit-identical to TPW = 1 (used by the batched and grouped launches, whose grids have
// thousands of workgroups; the single launch keeps one tile per workgroup to fill the CUs).
// The largest M tile whose unit loop preloads the unit's records (0: per format — 4 for the byte-decode formats
// on their 512-thread workgroups, 2 for the nibble-plane ones: profiles/r06_tuning/r6l_ab_gemv_pre_mt4.txt, M = 4,
// K = 14336: Q5_0 19.18 -> 18.64 us, Q8_0 19.02 -> 18.27, but Q4_0 11.21 -> 12.32, Q4_1 12.00 -> 16.23)
#ifndef QG_GEMV_PRE_MT
#define QG_GEMV_PRE_MT 0
#endif
template <int F> constexpr int gemv_pre_mt = QG_GEMV_PRE_MT ? QG_GEMV_PRE_MT : (F == FMT_Q4_0 || F == FMT_Q4_1) ? 2 : 4;
#ifndef QG_GEMV_ACT2
#define QG_GEMV_ACT2 1  // (A/B builds) 0: M >= 2 loads each further activation block after the previous record
#endif
template <int F, int MT, int BPL, int LPR, int WGS, bool SUMI, int AIN, bool NT, bool PRE, int ONEU, int TPW = 1>
__device__ __forceinline__ void gemv_body(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B, long sA, long sB,
                                          int M, int N, int K, float* __restrict__ C, long sC, long ldc_m, long ldc_n,
                                          int32_t* __restrict__ sumi_out, int tile_in = -1) {
    static_assert(TPW == 1 || ONEU == 1, "several tiles per workgroup: the one-unit form only");
    constexpr int NUN = ONEU > 1 ? ONEU : 1;  // weight units in registers per lane (loop-free forms)
    using G = gemv_geom<F, BPL>;
    A = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(A) + blockIdx.y * sA);
    B += blockIdx.y * sB;
    C += blockIdx.y * sC;
    constexpr int RPW = 64 / LPR;
    constexpr int RPB = (WGS / 64) * RPW;  // rows per workgroup
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];

    const int nb = K / QK;
    const int U = nb / BPL;  // units per row
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int lir = lane % LPR;
    // XCD-aware tile order for grids of one dispatch round (<= 512 workgroups): workgroups are placed
    // round-robin over the 8 XCDs (b -> XCD b % 8), and XCD x takes a contiguous range of row tiles,
    // so the 64-B output pieces of neighbouring workgroups dirty whole lines of ONE XCD's L2 (the
    // end-of-kernel write-back is the GEMV's largest fixed cost after the launch;
    // profiles/r02_tuning/ab_xcd.txt: M=1 3.33 -> 3.29 us, M=2 3.66 -> 3.58). Larger grids keep
    // the linear order (N=32000: 12.55 us linear, 13.28 remapped).
    // (a grouped launch passes the workgroup's tile within its item, tile_in >= 0)
    // The grid's tile count is derived from N, which is preloaded, not read from gridDim.x: in the strided
    // batch that hidden argument lies past the preloaded dwords and cost a scalar-memory round trip ahead
    // of the first load. gemv_launch asserts grid.x == gemv_tiles(N, rows per workgroup) at every launch.
    const int ntile = gemv_tiles(N, RPB * TPW);
    const int tile = tile_in >= 0 ? tile_in : ntile <= 512 ? xcd_tile(blockIdx.x, ntile) : (int)blockIdx.x;
    int rows[TPW];
    bool rows_ok[TPW];
    const uint8_t* wrows[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        rows[t] = (tile * TPW + t) * RPB + (tid >> 6) * RPW + lane / LPR;
        rows_ok[t] = rows[t] < N;
        wrows[t] = B + (long)(rows_ok[t] ? rows[t] : 0) * ((long)U * G::UB);
    }
    const int row = rows[0];
    const bool row_ok = rows_ok[0];
    auto load_unit = [&](uint32_t (&dst)[G::UDW], int u, int t = 0) {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(wrows[t] + (long)((rows_ok[t] && u < U) ? u : 0) * G::UB);
        if constexpr (NT) {
#pragma unroll
            for (int v = 0; v + 4 <= G::UDW; v += 4) {
                const u32x4_a4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x4_a4*>(p + v));
                dst[v] = t.x; dst[v + 1] = t.y; dst[v + 2] = t.z; dst[v + 3] = t.w;
            }
            if constexpr (G::UDW % 4 == 2) {
                const u32x2_a4 t = __builtin_nontemporal_load(reinterpret_cast<const u32x2_a4*>(p + G::UDW - 2));
                dst[G::UDW - 2] = t.x; dst[G::UDW - 1] = t.y;
            }
        } else {
#pragma unroll
            for (int v = 0; v < G::UDW; ++v) dst[v] = p[v];
        }
    };
    // record of activation block blk = m * nb + b: unit (m * U + b / BPL) = blk / BPL, slot b % BPL
    auto rec_of = [&](int blk) { return (blk / BPL) * G::REC_DW + (blk % BPL) * 12; };
    uint32_t curs[NUN][G::UDW];
    uint32_t(&cur)[G::UDW] = curs[0];
    uint32_t more[TPW > 1 ? TPW - 1 : 1][G::UDW];  // tiles 1.. of the workgroup (TPW > 1)
    auto load_first = [&]() {
        load_unit(cur, lir);
#pragma unroll
        for (int j = 1; j < NUN; ++j) load_unit(curs[j], lir + j * LPR);
#pragma unroll
        for (int t = 1; t < TPW; ++t) load_unit(more[t - 1], lir, t);
    };

    // 1) activation block loads of this thread (one thread per block), the first before the
    //    weight stream; 2) the lane's first weight unit; 3) LDS records
    const int totb = M * nb;
    if constexpr (AIN == AIN_Q8_1) {
        // M >= 2: a thread's first TWO blocks are loaded before the weight stream (M = 4 at K = 14336 stages
        // 1792 blocks over 1024 threads: the second round no longer waits behind the first one's records)
        constexpr int NA = MT >= 2 && QG_GEMV_ACT2 ? 2 : 1;
        uint32_t ab[NA][9];
        auto load_ablk = [&](int g, uint32_t (&d)[9]) {
            const uint32_t* p = A + (long)g * 9;
#pragma unroll
            for (int i = 0; i < 9; ++i) d[i] = p[i];
        };
#pragma unroll
        for (int k = 0; k < NA; ++k)
            if (tid + k * WGS < totb) load_ablk(tid + k * WGS, ab[k]);
        load_first();
#pragma unroll
        for (int k = 0; k < NA; ++k)
            if (tid + k * WGS < totb) make_act_record<F>(ab[k], lds + rec_of(tid + k * WGS));
        for (int g = tid + NA * WGS; g < totb; g += WGS) {
            load_ablk(g, ab[0]);
            make_act_record<F>(ab[0], lds + rec_of(g));
        }
    } else {
        const uint8_t* X = reinterpret_cast<const uint8_t*>(A);
        float xv[32];
        if (tid < totb) load_act_block<AIN>(X, tid, xv);
        load_first();
        for (int g = tid; g < totb; g += WGS) {
            if (g != tid) load_act_block<AIN>(X, g, xv);
            uint32_t w[9];
            if constexpr (AIN == AIN_F32) quantize_q8_1_block<0>(xv, w);
            else quantize_q8_1_block_fp16_fused(xv, w);
            make_act_record<F>(w, lds + rec_of(g));
        }
    }
    __syncthreads();

    float acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = 0.0f;

    // one unit of this lane: activation records preloaded (PRE) or read per block
    uint4 pre[PRE ? BPL : 1][PRE ? MT : 1][3];
    auto read_pre = [&](int u) {
        if constexpr (PRE) {
#pragma unroll
            for (int bi = 0; bi < BPL; ++bi)
#pragma unroll
                for (int m = 0; m < MT; ++m) {
                    const uint32_t* rec = lds + (min(m, M - 1) * U + u) * G::REC_DW + bi * 12;
#pragma unroll
                    for (int x = 0; x < 3; ++x) pre[bi][m][x] = *reinterpret_cast<const uint4*>(rec + 4 * x);
                }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    auto dot_unit = [&](const uint32_t (&cur)[G::UDW], int u, int row, bool row_ok) {
        static_for<BPL>([&](auto BI) {
            constexpr int bi = decltype(BI)::value;
#pragma unroll
            for (int m = 0; m < MT; ++m) {
                if (m < M) {
                    uint4 a[3];
                    if constexpr (PRE) {
                        a[0] = pre[bi][m][0]; a[1] = pre[bi][m][1]; a[2] = pre[bi][m][2];
                    } else {
                        const uint32_t* rec = lds + (m * U + u) * G::REC_DW + bi * 12;
                        a[0] = *reinterpret_cast<const uint4*>(rec);
                        a[1] = *reinterpret_cast<const uint4*>(rec + 4);
                        a[2] = *reinterpret_cast<const uint4*>(rec + 8);
                    }
                    const uint32_t d = block_dot<F, bi>(cur, a);
                    if constexpr (SUMI) {
                        if (row_ok) sumi_out[((long)m * N + row) * nb + u * BPL + bi] = (int)(d - ACC_BIAS);
                    } else {
                        acc[m] += block_term_rec<F, bi>(cur, d, a[2]);
                    }
                }
            }
        });
    };
    auto do_unit = [&](int u) {
        read_pre(u);
        dot_unit(cur, u, row, row_ok);
    };
    const int iters = (U + LPR - 1) / LPR;
    if constexpr (TPW > 1) {
        // tiles 1.. after tile 0 (below): the records read once, each tile its own sum and store
        static_assert(!SUMI || TPW == 1, "parity hook: one tile per workgroup");
    }
    if constexpr (ONEU == 1) {
        if (lir < U) do_unit(lir);
    } else if constexpr (ONEU > 1) {
#pragma unroll
        for (int j = 0; j < NUN; ++j) {
            const int u = lir + j * LPR;
            if (u < U) {
                read_pre(u);
                dot_unit(curs[j], u, row, row_ok);
            }
        }
    } else {
        for (int j = 0; j < iters; ++j) {
            const int u = lir + j * LPR;
            uint32_t nxt[G::UDW];
            if (j + 1 < iters) load_unit(nxt, u + LPR);
            if (u < U) do_unit(u);
            if (j + 1 < iters) {
#pragma unroll
                for (int v = 0; v < G::UDW; ++v) cur[v] = nxt[v];
            }
        }
    }
    if constexpr (!SUMI) {
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m] = group_sum_last<LPR>(acc[m]);
        if (row_ok && lir == LPR - 1) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
                if (m < M) C[m * ldc_m + row * ldc_n] = acc[m];
        }
    }
    if constexpr (TPW > 1 && !SUMI) {
#pragma unroll
        for (int t = 1; t < TPW; ++t) {
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = 0.0f;
            if (lir < U) dot_unit(more[t - 1], lir, rows[t], rows_ok[t]);
#pragma unroll
            for (int m = 0; m < MT; ++m) acc[m] = group_sum_last<LPR>(acc[m]);
            if (rows_ok[t] && lir == LPR - 1) {
#pragma unroll
                for (int m = 0; m < MT; ++m)
                    if (m < M) C[m * ldc_m + rows[t] * ldc_n] = acc[m];
            }
        }
    }
}

template <int F, int MT, int BPL, int LPR, int WGS, bool SUMI, int AIN = AIN_Q8_1, bool NT = false, bool PRE = (MT <= 2),
          int ONEU = 0, int TPW = 1>
__global__ __launch_bounds__(WGS) void gemv_kernel(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                   long sA, long sB, int M, int N, int K, float* __restrict__ C,
                                                   long sC, long ldc_m, long ldc_n, int32_t* __restrict__ sumi_out) {
    gemv_body<F, MT, BPL, LPR, WGS, SUMI, AIN, NT, PRE, ONEU, TPW>(A, B, sA, sB, M, N, K, C, sC, ldc_m, ldc_n, sumi_out);
}

// M = 2..8, one product: (A, B, M, N, K, out, ldc_m, ldc_n) with 32-bit output strides = 10 dwords
// (the general entry preloads 14 and s_loads the rest).
template <int F, int MT, int BPL, int LPR, int WGS, bool SUMI, int AIN = AIN_Q8_1, bool PRE = (MT <= 2), int ONEU = 0>
__global__ __launch_bounds__(WGS) void gemvs_kernel(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B, int M,
                                                    int N, int K, void* __restrict__ out, int ldc_m, int ldc_n) {
    gemv_body<F, MT, BPL, LPR, WGS, SUMI, AIN, false, PRE, ONEU>(A, B, 0, 0, M, N, K, SUMI ? nullptr : (float*)out, 0,
                                                                     ldc_m, ldc_n, SUMI ? (int32_t*)out : nullptr);
}

// M = 1, one product, out[n] (activation- and weight-major coincide at M = 1): the minimal argument
// list (A, B, N, K, out) = 8 dwords, all preloaded into SGPRs. Each preloaded kernel-argument dword
// costs every wave's launch: the single-launch M = 1 GEMV took 0.11 us longer with the general
// entry's 13 preloaded dwords than with these 8 (profiles/tools_archive/gemv_direct_probe.hip,
// profiles/r02_tuning/gemv_abl*.txt). SUMI: out is the parity hook's int32 buffer.
template <int F, int BPL, int LPR, int WGS, bool SUMI, int AIN = AIN_Q8_1, int ONEU = 0>
__global__ __launch_bounds__(WGS) void gemv1_kernel(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B, int N,
                                                    int K, void* __restrict__ out) {
    gemv_body<F, 1, BPL, LPR, WGS, SUMI, AIN, false, true, ONEU>(A, B, 0, 0, 1, N, K, SUMI ? nullptr : (float*)out, 0, 0,
                                                                     1, SUMI ? (int32_t*)out : nullptr);
}

// Grouped GEMV (qg_gemm_w4a8_grouped): up to GEMV_GROUP_MAX independent products with their own A,
// B, C and N (and output row stride), one M and K, in ONE launch — e.g. a decoder layer's Q / K / V
// or gate / up projections. The item table travels by value in the kernel arguments (GemvItems in
// qg_kernels.hpp: no device allocation, capture-safe); blockIdx.y is the item, blockIdx.x its row
// tile, and workgroups past an item's rows exit at once (grid.x = the largest item's tiles). The
// item's pointers are ONE scalar load (32-B record); the outputs are bit-identical to the single
// launch (same body, same per-row summation). A first version located each workgroup's item in a
// tile prefix table (a lane-parallel vector load + ballot, or 64 scalar compares): 1.72 / 2.10 us per
// GEMV in a group of 64 vs 1.44 for the strided batch (the lookup sat in front of every workgroup's
// weight stream).
// Groups whose items all have the launch's row-tile count (grp.full) skip the early-exit test. (The
// round-4 item-per-XCD 1-D grid for uniform groups measured slower, 1.59 -> 1.64 us per GEMV; round 5:
// staging the activations of groups with one shared A from the preloaded header, before the item's
// descriptor returns, measured no gain — profiles/r05_tuning/r5b_ab_grouped.txt, 1.510 -> 1.516 us.)
// row tiles per workgroup of the loop-free launches (gemv_body TPW): grouped (QG_GEMVG_TPW) and strided
// batch (QG_GEMV_TPW). profiles/r04_tuning/r04d_bench_tpw*.json, 64 GEMVs (M = 1, N = K = 4096) per
// launch: grouped 1.606 -> 1.529 us per GEMV with 2 (one descriptor load and one activation staging per
// two tiles), strided batch 1.450 -> 1.452 (no descriptor to amortise: kept at 1)
#ifndef QG_GEMV_TPW
#define QG_GEMV_TPW 1
#endif
#ifndef QG_GEMVG_TPW
#define QG_GEMVG_TPW 2
#endif
// M >= 2 grouped / strided-batch launches whose items fit one round: 256-thread workgroups of two row
// tiles (profiles/r04_tuning/ab_mt_wgs_r4m.txt, 64 products per launch, N = K = 4096, vs the M = 1 rule:
// strided Q4_0 M = 2 1.72 -> 1.64 us, M = 4 2.78 -> 2.42, Q4_1 M = 3 3.54 -> 2.59; grouped Q4_0 M = 2
// 1.75 -> 1.61, M = 4 2.49 -> 2.41; Q5_x / Q8_0 within +-1 % except grouped Q8_0 M = 4 +2 %; one row tile
// per 256-thread workgroup is slower everywhere). 0: the M = 1 rule.
#ifndef QG_GEMV_MTGW
#define QG_GEMV_MTGW 256
#endif
#ifndef QG_GEMV_MTTPW
#define QG_GEMV_MTTPW 2
#endif
#ifndef QG_GEMVG_WDIV
#define QG_GEMVG_WDIV 2  // grouped launch workgroup size = the single launch's / QG_GEMVG_WDIV (below)
#endif
// The front end: M, K, the flags (GEMVG_FULL, GEMVG_XCD) and the launch's tile count (= grid.x) are leading
// scalars, preloaded into SGPRs by the dispatch, and the item's 32-B record is the kernel's first
// instruction, so ONE scalar-memory round trip precedes the first vector load. (With the whole GemvGroup as
// the only argument nothing was preloaded and three dependent round trips did: the hidden gridDim.x for the
// tile order, then full and N for the early exit, then the pointers with M and K —
// profiles/group_front/README.md.)
template <int F, int MT, int BPL, int LPR, int WGS, bool PRE, int ONEU, int TPW = 1>
__global__ __launch_bounds__(WGS) void gemvg_kernel(int M, int K, int flags, int tiles, const GemvItems items) {
    constexpr int RPB = (WGS / 64) * (64 / LPR) * TPW;  // rows per workgroup
    // the record as ONE 8-dword load (field by field, the compiler fetched N for the early exit first and
    // the pointers in a second round trip behind the branch)
    static_assert(sizeof(GemvItemDesc) == 32 && offsetof(GemvItemDesc, N) == 24 && offsetof(GemvItemDesc, ldc) == 28, "");
    const u32x8_a16 r = *reinterpret_cast<const u32x8_a16*>(&items.it[blockIdx.y]);
    GemvItemDesc d;  // (pointers rebuilt in the global address space: from a plain integer they would be flat)
    d.A = global_ptr<const void>(r[0], r[1]);
    d.B = global_ptr<const void>(r[2], r[3]);
    d.C = global_ptr<float>(r[4], r[5]);
    d.N = (int)r[6];
    d.ldc = (int)r[7];
    // the single launch's XCD-aware tile order (gemv_body) within the item: with grid.x a multiple of 8 the
    // workgroup's XCD is blockIdx.x % 8, so each XCD takes a contiguous range of its tiles
    const int tile = (flags & GEMVG_XCD) ? xcd_tile(blockIdx.x, tiles) : (int)blockIdx.x;
    if (!(flags & GEMVG_FULL) && tile * RPB >= d.N) return;  // past this item's rows (uniform)
    gemv_body<F, MT, BPL, LPR, WGS, false, AIN_Q8_1, false, PRE, ONEU, TPW>(
        reinterpret_cast<const uint32_t*>(d.A), reinterpret_cast<const uint8_t*>(d.B), 0, 0, M, d.N, K,
        d.C, 0, d.ldc, 1, nullptr, tile & INT32_MAX);  // (the mask: known >= 0, so the body's own tile order folds away)
}

// Loop-free multi-unit single launches (ONEU = 2 / 4, above): 1 = on, 0 = the unit loop (A/B builds).
#ifndef QG_GEMV_NU
#define QG_GEMV_NU 1
#endif
#ifndef QG_GEMV_NU_MT
#define QG_GEMV_NU_MT 1  // (A/B builds) the largest M tile that takes the multi-unit form
#endif

// Host side -------------------------------------------------------------------------------------

template <int F, int BPL> inline size_t gemv_lds_bytes(int M, int K) {
    return (size_t)M * (K / QK / BPL) * gemv_geom<F, BPL>::REC_DW * 4;
}

// Preconditions of the kernel for unit size BPL: whole units per row, 4-byte aligned operands
// (units and rows are then whole dwords), LDS records fit.
template <int F, int BPL>
inline bool gemv_shape_ok(const GemmArgs& g) {
    if (g.M < 1 || g.M > 8) return false;
    if (g.K % (QK * BPL) != 0) return false;
    const int aal = g.ain == AIN_Q8_1 ? 3 : 15;  // fused: 16-B vector loads of the FP32/FP16 rows
    if (((uintptr_t)g.B & 3) != 0 || ((uintptr_t)g.A & aal) != 0) return false;
    if (g.batch > 1 && ((g.sB & 3) != 0 || (g.sA & aal) != 0)) return false;
    if (g.sumi && g.ain != AIN_Q8_1) return false;
    if (g.M > 2 && gemv_lds_bytes<F, BPL>(g.M, g.K) > 96 * 1024) return false;
    return true;
}

// Shape classes whose affine groups take the strided batch's kernel (group_affine_mode() == 1; 2: every class),
// by measurement: tools/ab_group_front.py (64 products per step on distinct weight copies in grouped launches
// of `count` items, mode 0 vs mode 2 in one process, interleaved rounds of 100 replays after one uncounted;
// us per GEMV, grouped -> affine), profiles/group_front/ab_group_front*.txt. Enabled where affine beats grouped
// by more than the grouped arm's run-to-run spread (0.1 .. 0.9 % of its median; 2 - 3 % at K <= 2048):
//  * the loop-free one-unit form at M = 1, items of at most 16 rows per compute unit (small_n: N <= 4096 on a
//    whole MI355X, what was measured), 8 items or more. N = K = 4096 x 64: Q4_0 1.515 -> 1.475, Q4_1 1.676 -> 1.662, Q5_0 1.831
//    -> 1.798, Q5_1 2.009 -> 1.971, Q8_0 2.760 -> 2.751; x 32: Q4_0 1.533 -> 1.489, Q5_1 2.023 -> 1.995; x 16:
//    Q4_0 1.595 -> 1.565, Q8_0 2.896 -> 2.830; x 8: Q4_0 1.765 -> 1.715, Q4_1 1.942 -> 1.872, Q8_0 3.099 ->
//    2.964. N = 1024 x 64 0.424 -> 0.420, N = 2048 x 16 0.922 -> 0.876, K = 256 x 64 0.195 -> 0.183, K = 2048
//    x 8 1.033 -> 1.019, Q8_0 K = 2048 x 64 1.454 -> 1.440. One point of the class is a tie: Q4_0 K = 2048 x
//    64, 0.747 -> 0.741 inside a 2.9 % spread. (The strided kernel takes ONE row tile per workgroup where the
//    grouped one takes two, so its grid has twice the workgroups.)
// Not enabled:
//  * fewer than 8 items of that class: the sign follows how the two grids fill the last dispatch round (Q4_0
//    N = K = 4096 x 2 1.020x, x 3 0.971x, x 4 1.006x, x 5 1.003x, x 6 1.020x; Q8_0 x 3 1.050x);
//  * M >= 2 in the one-unit form (both kernels: 256 threads, two tiles): Q4_0 N = K = 4096 x 64 M = 2 0.992x,
//    M = 4 1.000x, x 8 M = 2 0.982x, x 3 0.983x; Q8_0 M = 2 1.019x;
//  * larger items: N = 14336 x 2 1.065x (M = 2 1.177x, M = 4 1.032x, Q8_0 1.150x), x 8
//    1.049x, N = 11008 x 2 1.065x, N = 32000 x 2 1.029x, but N = 8192 x 2 0.972x, N = 14336 x 64 0.989x, N =
//    32000 x 64 0.996x — mixed, so the class stays off;
//  * the unit loop: M = 1 ties (K = 8192 0.998x, K = 14336 1.006x, Q8_0 1.000x). M >= 2 gains where the grouped
//    kernel runs its 256-thread workgroups, Q4_0 only (N = 4096 x 64: K = 8192 M = 2 1.063x, M = 4 2.076x, K =
//    11008 M = 2 1.259x, K = 14336 M = 2 1.460x, M = 3 2.264x, M = 4 2.906x; Q8_0 M = 2 1.000x, Q5_1 M = 4 1.003x,
//    N = 8192 0.993x): left off here, with the merge's own gate for that class (fuse_class_enabled).
inline bool group_affine_class_enabled(bool one, int MT, bool small_n, int count, int mode) {
    if (mode == 2) return true;
    return one && MT == 1 && small_n && count >= 8;
}

// gemv_body's ONEU for rows of `units` units on `lpr` lanes: 1, one unit per lane; 2 / 4, the loop-free multi-unit form
// of Q4_0 M = 1 single launches; 0, the unit loop. gemv_pick and the expert-indexed launch (qg_moe.hip) both ask here.
// profiles/r05_tuning/r5zd_ab.txt, unit loop -> multi-unit: Q4_0 M = 1 K = 14336 7.69 -> 7.46 us, K = 11008
// 6.32 -> 6.17, K = 8192 5.02 -> 4.78; slower for M = 2..4 (8.93 -> 9.45 at M = 2), Q4_1 (8.02 -> 9.50) and
// Q8_0 (12.37 -> 12.53), which keep the loop
template <int F, int MT> constexpr bool gemv_nu_ok = QG_GEMV_NU && MT <= QG_GEMV_NU_MT && F == FMT_Q4_0;
template <int F, int MT> inline int gemv_unit_form(int units, int lpr) {
    if (units <= lpr) return 1;
    const int per_lane = (units + lpr - 1) / lpr;
    return !gemv_nu_ok<F, MT> ? 0 : per_lane <= 2 ? 2 : per_lane <= 4 ? 4 : 0;
}

// The smaller workgroups of many-product launches (grouped, strided batch, expert slots) whose rows fit one round of
// full-size ones: (threads, row tiles) = (wgs / wdiv, tpw) at M = 1, the caller's knobs, and (QG_GEMV_MTGW, QG_GEMV_MTTPW)
// at M >= 2; wgs == 0: no such form. Whether the rows fit the round (device_cus()) is the caller's test.
struct GemvSmallWg { int wgs, tpw; };
constexpr GemvSmallWg gemv_small_wg(int wgs, int mt, int wdiv, int tpw) {
    const bool mtw = QG_GEMV_MTGW > 0 && mt >= 2;
    const GemvSmallWg s = mtw ? GemvSmallWg{QG_GEMV_MTGW < wgs ? QG_GEMV_MTGW : wgs, QG_GEMV_MTTPW} : GemvSmallWg{wgs / wdiv, tpw};
    return s.wgs < wgs && s.wgs >= 64 ? s : GemvSmallWg{0, 0};
}

// A strided batch of loop-free GEMVs whose N fits one round of full-size workgroups runs half-size
// ones, as the grouped launch (profiles/r04_tuning/ab_batched_wgs_r4b.txt, 64 products per launch,
// N = K = 4096: Q4_0 M = 1 1.526 -> 1.478 us per GEMV, M = 2 1.772 -> 1.641, M = 4 3.32 -> 2.76,
// N = 1024 0.436 -> 0.421; Q5_0 / Q8_0 M = 1 within +-0.7 %)
#ifndef QG_GEMVB_WDIV
#define QG_GEMVB_WDIV 2
#endif

// One instantiation as a GemvPick (qg_kernels.hpp): the kernel's address next to the constants that made it, so what
// gemv_run prints cannot differ from what it launches; `done` is this instantiation's lds_opt_in mask.
template <int SIG, int F, int MT, int BPL, int LPR, int WGS, bool SUMI, int AIN, bool NT, bool PRE, int ONEU, int TPW>
GemvPick gemv_pick_of() {
    static_assert(SIG != GEMV_SIG_M1 || (MT == 1 && PRE), "gemv1_kernel is the M = 1 tile with PRE");
    static std::atomic<unsigned long long> done;
    GemvPick p = {};
    if constexpr (SIG == GEMV_SIG_M1) p.fn = (const void*)gemv1_kernel<F, BPL, LPR, WGS, SUMI, AIN, ONEU>;
    else if constexpr (SIG == GEMV_SIG_SHORT) p.fn = (const void*)gemvs_kernel<F, MT, BPL, LPR, WGS, SUMI, AIN, PRE, ONEU>;
    else if constexpr (SIG == GEMV_SIG_FULL) p.fn = (const void*)gemv_kernel<F, MT, BPL, LPR, WGS, SUMI, AIN, NT, PRE, ONEU, TPW>;
    else p.fn = (const void*)gemvg_kernel<F, MT, BPL, LPR, WGS, PRE, ONEU, TPW>;
    p.lds_done = &done; p.sig = SIG; p.family = SIG == GEMV_SIG_GROUP ? "gemvg" : "gemv";
    p.F = F; p.MT = MT; p.BPL = BPL; p.LPR = LPR; p.WGS = WGS; p.AIN = AIN; p.NT = NT; p.PRE = PRE; p.ONEU = ONEU; p.TPW = TPW;
    p.rpw = (WGS / 64) * (64 / LPR) * TPW;
    return p;
}

// The row GEMV's kernel, grid and LDS for one call: every rule that chooses among the instantiations of (F, MT, BPL, LPR,
// WGS, PRE) — gemv_form's answer, qg_gemv_impl.hpp — is here and nowhere else. gemv_run (qg_gemv.hip) describes, fills
// or launches what it is handed.
template <int F, int MT, int BPL, int LPR, int WGS, bool SUMI, int AIN, bool NT, bool PRE>
GemvPick gemv_pick(const GemmArgs& g) {
    constexpr int RPB = (WGS / 64) * (64 / LPR);
    constexpr bool NU_OK = gemv_nu_ok<F, MT>;
    // PRE beyond MT = 2 only in the loop-free forms (with the unit loop it spills at MT = 4); the short entry's loop
    // up to gemv_pre_mt<F>
    constexpr std::bool_constant<PRE> pre{};
    constexpr std::bool_constant<(PRE && MT <= 2)> pre2{};
    constexpr ic<0> i0{}; constexpr ic<1> i1{}; constexpr ic<WGS> wgs{};
    auto k = [](auto sig, auto gw, auto pr, auto oneu, auto tpw) { return gemv_pick_of<sig, F, MT, BPL, LPR, gw, SUMI, AIN, NT, pr, oneu, tpw>(); };
    const int nu = gemv_unit_form<F, MT>(g.K / QK / BPL, LPR);
    const bool one = nu == 1;
    GemvPick p = {};
    if constexpr (!SUMI && AIN == AIN_Q8_1 && !NT && MT <= 4) {  // (AUTO sends only M <= 4 to the GEMV)
        if (g.group) {  // grouped launch (qg_gemm_w4a8_grouped): blockIdx.y = item
            const GemvGroup& grp = *static_cast<const GemvGroup*>(g.group);
            // An affine group (qg_group_affine.hpp) is a strided batch: it takes the kernel and grid
            // qg_gemm_w4a8_strided_batched launches for the same items (below), whose arguments all sit in
            // SGPRs — no descriptor load ahead of the weight stream. Same body, same bits.
            affine::Strides as;
            const int amode = group_affine_mode();
            if (amode && g.affine >= 0 && grp.count >= 2 && group_affine_class_enabled(one, MT, g.N <= 16 * device_cus(), grp.count, amode) &&
                affine::group_affine(grp.it, grp.count, 3, 15, &as)) {
                GemmArgs b = g;
                b.group = nullptr; b.batch = grp.count;
                b.A = grp.it[0].A; b.B = grp.it[0].B; b.C = grp.it[0].C;
                b.N = grp.it[0].N; b.ldc_m = grp.it[0].ldc; b.ldc_n = 1;
                b.sA = (long)as.a; b.sB = (long)as.b; b.sC = (long)(as.c / 4);
                p = gemv_pick<F, MT, BPL, LPR, WGS, SUMI, AIN, NT, PRE>(b);
                p.family = "gemvb"; p.affine = 1;
                return p;
            }
            int nmax = 0, nmin = INT32_MAX;
            for (int i = 0; i < grp.count; ++i) nmax = std::max(nmax, grp.it[i].N), nmin = std::min(nmin, grp.it[i].N);
            auto kg = [&](auto gw, auto tp) { return one ? k(ic<GEMV_SIG_GROUP>{}, gw, pre, i1, tp) : k(ic<GEMV_SIG_GROUP>{}, gw, pre2, i0, i1); };
            p = kg(wgs, ic<QG_GEMVG_TPW>{});
            // workgroups of WGS / QG_GEMVG_WDIV threads while the largest item's rows fit one round of
            // full-size workgroups (<= 256): twice as many resident per CU, so one workgroup's descriptor
            // load and activation staging overlap another's weight stream (profiles/r04_tuning/
            // ab_grouped_wgs_r4g2.txt, 64 items per launch, N = K = 4096: Q4_0 M = 1 1.541 -> 1.509 us per
            // GEMV, M = 2 1.853 -> 1.688, M = 4 2.705 -> 2.494, Q8_0 2.885 -> 2.767; N = 11008 (344 tiles)
            // 3.92 -> 4.01 with them, so larger items keep full-size workgroups)
            constexpr GemvSmallWg SG = gemv_small_wg(WGS, MT, QG_GEMVG_WDIV, QG_GEMVG_TPW);
            if constexpr (SG.wgs > 0)
                if (gemv_tiles(nmax, p.rpw) <= device_cus()) p = kg(ic<SG.wgs>{}, ic<SG.tpw>{});
            // grid.x = the largest item's tiles; full: the smallest item has as many (an empty group: never)
            p.grid = dim3(gemv_tiles(nmax, p.rpw), grp.count);
            p.full = p.grid.x == (unsigned)gemv_tiles(nmin, p.rpw);
            p.flags = (p.full ? GEMVG_FULL : 0) | (p.grid.x <= 512 ? GEMVG_XCD : 0);
        }
    }
    // M = 1, one product, unit output stride: the minimal-argument entry (gemv1_kernel), which alone takes Q4_0's
    // loop-free multi-unit forms (no gemv1_kernel from the M tiles that cannot launch it)
    const bool single = !NT && g.batch == 1;
    if constexpr (MT == 1 && PRE && !NT) if (!p.fn && g.M == 1 && single && g.ldc_n == 1) {
        p = one ? k(ic<GEMV_SIG_M1>{}, wgs, pre, i1, i1) : k(ic<GEMV_SIG_M1>{}, wgs, pre, i0, i1);
        if constexpr (NU_OK) {
            if (nu == 2) p = k(ic<GEMV_SIG_M1>{}, wgs, pre, ic<2>{}, i1);
            if (nu == 4) p = k(ic<GEMV_SIG_M1>{}, wgs, pre, ic<4>{}, i1);
        }
    }
    // one product with 32-bit output strides: the short-argument entry (gemvs_kernel). It takes the multi-unit forms only
    // when NU_OK && MT > 1, otherwise its loop or the one-unit form
    if (!p.fn && single && g.ldc_m <= INT32_MAX && g.ldc_n <= INT32_MAX) {
        p = one ? k(ic<GEMV_SIG_SHORT>{}, wgs, pre, i1, i1)
                : k(ic<GEMV_SIG_SHORT>{}, wgs, std::bool_constant<(PRE && MT <= gemv_pre_mt<F>)>{}, i0, i1);
        if constexpr (NU_OK && MT > 1) {
            if (nu == 2) p = k(ic<GEMV_SIG_SHORT>{}, wgs, pre2, ic<2>{}, i1);
            if (nu == 4) p = k(ic<GEMV_SIG_SHORT>{}, wgs, pre2, ic<4>{}, i1);
        }
    }
    // the general entry (gemv_kernel): a strided batch of loop-free GEMVs takes QG_GEMV_TPW row tiles per workgroup (same
    // per-row arithmetic), and half-size workgroups (QG_GEMVB_WDIV, above) while N fits one round of full-size ones
    if (!p.fn) {
        constexpr bool tpw_ok = !SUMI && !NT && QG_GEMV_TPW > 1;
        const bool many = one && g.batch > 1;
        p = many ? k(ic<GEMV_SIG_FULL>{}, wgs, pre, i1, ic<(tpw_ok ? QG_GEMV_TPW : 1)>{})
          : one  ? k(ic<GEMV_SIG_FULL>{}, wgs, pre, i1, i1)
                 : k(ic<GEMV_SIG_FULL>{}, wgs, pre2, i0, i1);
        constexpr GemvSmallWg SB = gemv_small_wg(WGS, MT, QG_GEMVB_WDIV, QG_GEMV_TPW);
        if constexpr (SB.wgs > 0 && !SUMI && !NT)
            if (many && gemv_tiles(g.N, RPB) <= device_cus()) p = k(ic<GEMV_SIG_FULL>{}, ic<SB.wgs>{}, pre, i1, ic<SB.tpw>{});
    }
    if (p.sig != GEMV_SIG_GROUP) p.grid = dim3((g.N + p.rpw - 1) / p.rpw, g.batch);  // (gemv_run checks it: gemv_tiles)
    p.lds = gemv_lds_bytes<F, BPL>(g.M, g.K);
    p.one = one ? 1 : 0; p.a = g;
    return p;
}

template <int F, int MT, int BPL, int LPR, int WGS, bool SUMI, int AIN = AIN_Q8_1, bool NT = false, bool PRE = (MT <= 2)>
hipError_t gemv_launch(const GemmArgs& g, hipStream_t st) {
    if (g.group && (SUMI || AIN != AIN_Q8_1 || NT || MT > 4)) return hipErrorInvalidValue;  // no grouped form here
    return gemv_run(gemv_pick<F, MT, BPL, LPR, WGS, SUMI, AIN, NT, PRE>(g), st);
}

}  // namespace qg
