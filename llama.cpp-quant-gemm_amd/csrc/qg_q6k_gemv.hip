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

// raw dwords of a unit: the ql and qh pieces (9 each: 32 bytes + the realignment dword), the half's scales (3), d (1)
constexpr int Q6K_UNIT_DW = 22;

template <int MT, int LPR, int WGS, bool SUMI, bool ONE>
__global__ __launch_bounds__(WGS) void q6k_gemv_kernel(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B,
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
    const uint8_t* wrow = B + (long)(row_ok ? row : 0) * ((long)nsb * Q6K_BYTES);
    // (units past the row's end are clamped to its last one: loaded, never used)
    auto load_unit = [&](uint32_t (&dst)[Q6K_UNIT_DW], int u) {
        const int uc = min(u, U - 1);
        const int h = (uc >> 1) & 1, par = uc & 1;
        const uint8_t* sbp = wrow + (long)(uc >> 2) * Q6K_BYTES;
        uint32_t l[9], hq[9], s3[3], d1[1];
        q6k_load<8>(sbp + 64 * h + 32 * par, l);
        q6k_load<8>(sbp + Q6K_QH + 32 * h, hq);
        q6k_load<2>(sbp + Q6K_SC + 8 * h, s3);
        q6k_load<0>(sbp + Q6K_D, d1);
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            dst[i] = l[i];
            dst[9 + i] = hq[i];
        }
        dst[18] = s3[0]; dst[19] = s3[1]; dst[20] = s3[2];
        dst[21] = d1[0];
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
        uint32_t* rec = lds + (m * nsb + (b >> 3)) * Q6K_REC_DW;
        uint32_t* qs = rec + (b & 7) * 8;
        *reinterpret_cast<uint4*>(qs) = make_uint4(d[1], d[2], d[3], d[4]);
        *reinterpret_cast<uint4*>(qs + 4) = make_uint4(d[5], d[6], d[7], d[8]);
        rec[64 + (b & 7)] = __float_as_uint(h2f(d[0] & 0xFFFFu));
#if QG_Q6K_ASUM
        int a0 = 0, a1 = 0;  // 32 x the exact sums of the block's first and last 16 bytes
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a0 = __builtin_amdgcn_sdot4(0x20202020, (int)d[1 + i], a0, false);
            a1 = __builtin_amdgcn_sdot4(0x20202020, (int)d[5 + i], a1, false);
        }
        *reinterpret_cast<uint2*>(rec + 72 + 2 * (b & 7)) = make_uint2((uint32_t)a0, (uint32_t)a1);
#endif
    };
    uint32_t ab[9];
    if (tid < totb) load_ablk(tid, ab);
    uint32_t cur[Q6K_UNIT_DW];
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

    auto do_unit = [&](const uint32_t (&w)[Q6K_UNIT_DW], int u) {
        const int sb = u >> 2, h = (u >> 1) & 1, par = u & 1;
        // the parity of this super-block's address: all its pieces sit at multiples of 4 past it
        const uint32_t sh = (uint32_t)((uintptr_t)(wrow + (long)sb * Q6K_BYTES) & 3);
        uint32_t raw[9], ql[8], qh[8], scw[2];
#pragma unroll
        for (int i = 0; i < 9; ++i) raw[i] = w[i];
        q6k_realign<8>(raw, sh, ql);
#pragma unroll
        for (int i = 0; i < 9; ++i) raw[i] = w[9 + i];
        q6k_realign<8>(raw, sh, qh);
        const uint32_t sraw[3] = {w[18], w[19], w[20]};
        q6k_realign<2>(sraw, sh, scw);
        const float d = h2f((w[21] >> (8 * sh)) & 0xFFFFu);
        uint32_t q[2][8];  // blocks c = par and c = par + 2
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            q[0][j] = q6k_signed((ql[j] & 0x0F0F0F0Fu) | ((qh[j] << (4 - 2 * par)) & 0x30303030u));
            q[1][j] = q6k_signed(((ql[j] >> 4) & 0x0F0F0F0Fu) | ((qh[j] >> (2 * par)) & 0x30303030u));
        }
        // scales 8h + 2c, 8h + 2c + 1 of c = par (scale dword 0) and c = par + 2 (dword 1): bytes 2 par, 2 par + 1
        const int s16 = 16 * par;
        const int sc[2][2] = {{(int)(int8_t)(scw[0] >> s16), (int)(int8_t)(scw[0] >> (s16 + 8))},
                              {(int)(int8_t)(scw[1] >> s16), (int)(int8_t)(scw[1] >> (s16 + 8))}};
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < M) {
                const uint32_t* rec = lds + (m * nsb + sb) * Q6K_REC_DW;
                int isum[2];
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    const int blk = 4 * h + par + 2 * x;
                    const uint4 a0 = *reinterpret_cast<const uint4*>(rec + blk * 8);
                    const uint4 a1 = *reinterpret_cast<const uint4*>(rec + blk * 8 + 4);
                    int s0 = __builtin_amdgcn_sdot4((int)q[x][0], (int)a0.x, 0, false);
                    s0 = __builtin_amdgcn_sdot4((int)q[x][1], (int)a0.y, s0, false);
                    s0 = __builtin_amdgcn_sdot4((int)q[x][2], (int)a0.z, s0, false);
                    s0 = __builtin_amdgcn_sdot4((int)q[x][3], (int)a0.w, s0, false);
                    int s1 = __builtin_amdgcn_sdot4((int)q[x][4], (int)a1.x, 0, false);
                    s1 = __builtin_amdgcn_sdot4((int)q[x][5], (int)a1.y, s1, false);
                    s1 = __builtin_amdgcn_sdot4((int)q[x][6], (int)a1.z, s1, false);
                    s1 = __builtin_amdgcn_sdot4((int)q[x][7], (int)a1.w, s1, false);
#if QG_Q6K_ASUM
                    const uint2 as = *reinterpret_cast<const uint2*>(rec + 72 + 2 * blk);
                    s0 -= (int)as.x;
                    s1 -= (int)as.y;
#endif
                    isum[x] = sc[x][0] * s0 + sc[x][1] * s1;
                }
                if constexpr (SUMI) {
                    if (row_ok) {
                        int32_t* o = sumi_out + ((long)m * N + row) * nb + 8 * sb + 4 * h + par;
                        o[0] = isum[0];
                        o[2] = isum[1];
                    }
                } else {
                    const float da0 = __uint_as_float(rec[64 + 4 * h + par]), da1 = __uint_as_float(rec[66 + 4 * h + par]);
                    acc[m] += d * (da0 * (float)isum[0] + da1 * (float)isum[1]);
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
            uint32_t nxt[Q6K_UNIT_DW];
            if (j + 1 < iters) load_unit(nxt, u + LPR);
            if (u < U) do_unit(cur, u);
            if (j + 1 < iters) {
#pragma unroll
                for (int v = 0; v < Q6K_UNIT_DW; ++v) cur[v] = nxt[v];
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
struct q6k_gemv_fmt {
    static constexpr int REC_DW = Q6K_REC_DW;
    static constexpr size_t LDS_MAX = 160 * 1024;
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
