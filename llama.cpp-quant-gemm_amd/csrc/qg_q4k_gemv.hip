// qg_q4k_gemv.hip — the Q4_K decode GEMV (M <= 8 activation rows), family "q4k_gemv".
//
// C[m * ldc + n] = sum_sb [ d * sum_j d_a * float(sc_j * sumi_j) - dmin * sum_j float(m_j) * s_a ]   (qg_q4k.hpp)
//
// Work decomposition ("Q4_K"):
//  * A lane's unit is one chunk of a super-block: its 16-B header (d, dmin, scales) and the chunk's 32 qs bytes
//    = sub-blocks 2i and 2i + 1, three global_load_dwordx4, always 16-B aligned (QG_Q4K_NT below: without the
//    nontemporal hint). LPR lanes share a weight row and stride over its K / 64 units, the next one in flight while
//    the current one computes; 64 / LPR rows per wave. At K = 4096 a wave is one row, a CU holds 16 waves and the
//    kernel has no unit loop (ONE).
//    (The first version gave a lane whole super-blocks, 9 loads: one wave per SIMD and no overlap of the dot
//    with the weight stream — 6.79 us against 3.30 for Q4_0 at M = 1, N = K = 4096; profiles/q4k/README.md.)
//  * The workgroup stages the M activation rows once into LDS, one thread per Q8_1 block: per (token,
//    super-block) the 8 blocks' qs dwords (64), then their (d_a, s_a) as fp32 pairs (16), 4 pad dwords. The
//    thread's first block is loaded before the weight stream, so the staging waits only on it.
//  * qs dword t of the chunk needs no nibble shuffling: v & 0x0F0F0F0F is four elements of sub-block 2i,
//    (v >> 4) & 0x0F0F0F0F the same four positions of sub-block 2i + 1; both feed v_dot4 against the matching
//    activation dwords, 8 dot4 per sub-block, exact int32 sumi. The chunk is masked once and reused by every
//    token.
//  * sc_j * sumi_j in int32 (below 2^24: the conversion is exact), one fp32 dot accumulator and one min
//    accumulator per (token, unit); d and dmin are applied once per unit.
//  * Per-lane partials (unit order) are reduced across the row's LPR lanes with DPP row ops (group_sum_last),
//    fixed order: two launches give identical bits.
//  * XCD-aware tile order on grids of one dispatch round (xcd_tile), as the row GEMV.
//  * SUMI: the same instantiation stores each sub-block's int32 dot in place of the epilogue.
// Argument order: everything (11 dwords) is preloaded into SGPRs by the dispatch (csrc/Makefile).
#include "qg_kq_launch.hpp"
#include "qg_q4k.hpp"

namespace qg {
namespace {

constexpr int Q4K_UNIT_DW = 12;  // header (4) + one chunk's qs (8)

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

// ONE: every lane owns at most one unit (K <= 64 LPR): no unit loop in the kernel, so the wait for the weight
// loads sits at their first use, behind the activation records (the row GEMV's ONEU form).
template <int MT, int LPR, int WGS, bool SUMI, bool ONE>
__global__ __launch_bounds__(WGS) void q4k_gemv_kernel(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                      int M, int N, int K, void* __restrict__ out, long ldc) {
    constexpr int RPW = 64 / LPR;
    constexpr int RPB = (WGS / 64) * RPW;  // rows per workgroup
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];

    const int nb = K / QK, nsb = K / SB_ELEMS;
    const int U = 4 * nsb;  // units per row
    const int tid = threadIdx.x, lane = tid & 63, lir = lane % LPR;
    const int tile = gridDim.x <= 512 ? xcd_tile(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    const int row = tile * RPB + (tid >> 6) * RPW + lane / LPR;
    const bool row_ok = row < N;
    const uint8_t* wrow = B + (long)(row_ok ? row : 0) * ((long)nsb * Q4K_BYTES);
    // (units past the row's end are clamped to its last one: loaded, never used)
    auto load_unit = [&](uint32_t (&dst)[Q4K_UNIT_DW], int u) {
        const int uc = min(u, U - 1);
        const uint8_t* sbp = wrow + (long)(uc >> 2) * Q4K_BYTES;
        const u32x4 h = q4k_wload(reinterpret_cast<const u32x4*>(sbp));
        const u32x4* qp = reinterpret_cast<const u32x4*>(sbp + 16 + 32 * (uc & 3));
        const u32x4 q0 = q4k_wload(qp), q1 = q4k_wload(qp + 1);
        dst[0] = h.x; dst[1] = h.y; dst[2] = h.z; dst[3] = h.w;
        dst[4] = q0.x; dst[5] = q0.y; dst[6] = q0.z; dst[7] = q0.w;
        dst[8] = q1.x; dst[9] = q1.y; dst[10] = q1.z; dst[11] = q1.w;
    };

    // 1) this thread's first activation block, 2) the lane's first unit, 3) the LDS records
    const int totb = M * nb;
    auto load_ablk = [&](int g, uint32_t (&d)[9]) {
        const uint32_t* p = A + (long)g * 9;
#pragma unroll
        for (int i = 0; i < 9; ++i) d[i] = p[i];
    };
    auto put_ablk = [&](int g, const uint32_t (&d)[9]) {
        const int m = g / nb, b = g - m * nb;
        uint32_t* rec = lds + (m * nsb + (b >> 3)) * Q4K_REC_DW;
        uint32_t* qs = rec + (b & 7) * 8;
        *reinterpret_cast<uint4*>(qs) = make_uint4(d[1], d[2], d[3], d[4]);
        *reinterpret_cast<uint4*>(qs + 4) = make_uint4(d[5], d[6], d[7], d[8]);
        *reinterpret_cast<uint2*>(rec + 64 + (b & 7) * 2) =
            make_uint2(__float_as_uint(h2f(d[0] & 0xFFFFu)), __float_as_uint(h2f(d[0] >> 16)));
    };
    uint32_t ab[9];
    if (tid < totb) load_ablk(tid, ab);
    uint32_t cur[Q4K_UNIT_DW];
    load_unit(cur, lir);
    if (tid < totb) put_ablk(tid, ab);
    for (int g = tid + WGS; g < totb; g += WGS) {
        load_ablk(g, ab);
        put_ablk(g, ab);
    }
    __syncthreads();

    float acc[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = 0.0f;
    int32_t* sumi_out = SUMI ? static_cast<int32_t*>(out) : nullptr;

    auto do_unit = [&](const uint32_t (&w)[Q4K_UNIT_DW], int u) {
        const int sb = u >> 2, i = u & 3;
        uint32_t lo[8], hi[8];
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const uint32_t v = w[4 + t];
            lo[t] = v & 0x0F0F0F0Fu;
            hi[t] = (v >> 4) & 0x0F0F0F0Fu;
        }
        // sc / m of sub-blocks 2i, 2i + 1: bytes 2i, 2i + 1 of the eight (chunks 0, 1 in the first dword)
        const q4k_scales s = q4k_unpack_scales(w[1], w[2], w[3]);
        const int sh = (i & 1) * 16;
        const uint32_t scw = (i < 2 ? s.sc[0] : s.sc[1]) >> sh, mnw = (i < 2 ? s.mn[0] : s.mn[1]) >> sh;
        const int sc0 = (int)(scw & 0xFFu), sc1 = (int)((scw >> 8) & 0xFFu);
        const float m0 = (float)(mnw & 0xFFu), m1 = (float)((mnw >> 8) & 0xFFu);
        const float d = h2f(w[0] & 0xFFFFu), dmin = h2f(w[0] >> 16);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < M) {
                const uint32_t* rec = lds + (m * nsb + sb) * Q4K_REC_DW;
                uint32_t a[16];
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const uint4 t = *reinterpret_cast<const uint4*>(rec + 16 * i + 4 * x);
                    a[4 * x] = t.x; a[4 * x + 1] = t.y; a[4 * x + 2] = t.z; a[4 * x + 3] = t.w;
                }
                const int s0 = dot_block(lo, a), s1 = dot_block(hi, a + 8);
                if constexpr (SUMI) {
                    if (row_ok) {
                        int32_t* o = sumi_out + ((long)m * N + row) * nb + 8 * sb + 2 * i;
                        o[0] = s0;
                        o[1] = s1;
                    }
                } else {
                    const uint4 ds = *reinterpret_cast<const uint4*>(rec + 64 + 4 * i);  // d_a, s_a of 2i, 2i + 1
                    const float fd = __uint_as_float(ds.x) * (float)(sc0 * s0) + __uint_as_float(ds.z) * (float)(sc1 * s1);
                    const float fm = m0 * __uint_as_float(ds.y) + m1 * __uint_as_float(ds.w);
                    acc[m] += d * fd - dmin * fm;
                }
            }
        }
    };

    if constexpr (ONE) {
        if (lir < U) do_unit(cur, lir);
    } else {
        const int iters = (U + LPR - 1) / LPR;
        for (int j = 0; j < iters; ++j) {
            const int u = lir + j * LPR;
            uint32_t nxt[Q4K_UNIT_DW];
            if (j + 1 < iters) load_unit(nxt, u + LPR);
            if (u < U) do_unit(cur, u);
            if (j + 1 < iters) {
#pragma unroll
                for (int v = 0; v < Q4K_UNIT_DW; ++v) cur[v] = nxt[v];
            }
        }
    }
    if constexpr (!SUMI) {
        float* C = static_cast<float*>(out);
#pragma unroll
        for (int m = 0; m < MT; ++m) acc[m] = group_sum_last<LPR>(acc[m]);
        if (row_ok && lir == LPR - 1) {
#pragma unroll
            for (int m = 0; m < MT; ++m)
                if (m < M) C[m * ldc + row] = acc[m];
        }
    }
}

// instantiation choice, launch and eligibility: qg_kq_launch.hpp
struct q4k_gemv_fmt {
    static constexpr int REC_DW = Q4K_REC_DW;
    static constexpr size_t LDS_MAX = 160 * 1024;
    static constexpr uintptr_t WMASK = 15;  // the 16-B loads
    template <int MT, int LPR, int WGS, bool SUMI, bool ONE> static auto kernel() {
        return q4k_gemv_kernel<MT, LPR, WGS, SUMI, ONE>;
    }
    static void describe(const GemmArgs& g, int MT, int LPR, int WGS, int one, int grid, size_t lds) {
        describe_kernel(g, "q4k_gemv MT=%d LPR=%d WGS=%d ONE=%d NT=%d grid=%d lds=%zu", MT, LPR, WGS, one, QG_Q4K_NT, grid,
                        lds);
    }
};

}  // namespace

bool q4k_gemv_eligible(const GemmArgs& g) { return kq_gemv_eligible<q4k_gemv_fmt>(g); }
hipError_t launch_q4k_gemv(const GemmArgs& g, hipStream_t st) { return kq_gemv_launch<q4k_gemv_fmt>(g, st); }

}  // namespace qg
