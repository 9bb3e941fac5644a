// qg_q6k_gemv_body.inc — the body of the Q6_K decode GEMV, included as text into q6k_gemv_kernel (qg_q6k_gemv.hip,
// where the work decomposition is described) and q6k_moe_body (qg_moe.hip) and
// q6k_moeb_kernel (qg_moe_batch.hip) and q6k_glu_product[_staged] (qg_moe_glu.hip) and q6k_down_stage /
// q6k_down_product (qg_moe_down.hip). Text and not a function they
// call: the compiler sees the same tokens in the same function as before, so the shipped code objects do not move
// (DESIGN.md 3c).
// Expects in scope: A, B (the operands), M, N, K, out, ldc, the template parameters or constants MT, LPR, WGS, SUMI,
// ONE, and three macros, the lines in which the includers differ:
//   QG_KQ_DECLARE_TILE  the declaration of `const int tile` in the kernel, nothing where tile is a parameter
//   QG_KQ_ABLK(g)       the address of activation block g = m * K/32 + b in staging: `A + (long)g * 9` for dense rows,
//                       the gathered row of tile position m in the expert-grouped GEMV (qg_moe_batch.hip)
//   QG_KQ_OUT(m)        the output of token m at this lane's row: `C[m * ldc + row]`, the slot's row there
// and four the shipped includers leave undefined:
//   QG_KQ_A_STAGED      defined: the LDS records already hold the activation row (an earlier pass of the same
//                       workgroup staged it and a barrier has passed); the body loads its first unit and goes on
//   QG_KQ_STAGE_ONLY    defined: the inclusion is the staging prologue alone, the M activation rows into the records
//                       and its barrier: no weights, no row, no product (B, N, out, MT, SUMI, ONE are not needed)
//   QG_KQ_ROW           the lane's output row, where it is not `tile * RPB + (tid >> 6) * RPW + lane / LPR` (a
//                       workgroup whose waves share rows; tile is then not needed)
//   QG_KQ_RECS          the first LDS record of the activation row(s) the product reads, where that is not the start
//                       of the dynamic LDS (with QG_KQ_A_STAGED: the row of another slot)
    constexpr int RPW = 64 / LPR;
    constexpr int RPB = (WGS / 64) * RPW;  // rows per workgroup
#ifdef QG_KQ_RECS
    const uint32_t* const lds = QG_KQ_RECS;
#else
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
#endif

    const int nb = K / QK, nsb = K / SB_ELEMS;
    const int U = 4 * nsb;  // units per row
    const int tid = threadIdx.x, lane = tid & 63, lir = lane % LPR;
#ifndef QG_KQ_STAGE_ONLY
#ifdef QG_KQ_ROW
    const int row = QG_KQ_ROW;
#else
    QG_KQ_DECLARE_TILE
    const int row = tile * RPB + (tid >> 6) * RPW + lane / LPR;
#endif
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
#endif

#ifdef QG_KQ_A_STAGED
    uint32_t cur[Q6K_UNIT_DW];
    load_unit(cur, lir);
#else
    // 1) this thread's first activation block, 2) the lane's first unit, 3) the LDS records
    const int totb = M * nb;
    auto load_ablk = [&](int g, uint32_t (&d)[9]) {
        const uint32_t* p = QG_KQ_ABLK(g);
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
#ifndef QG_KQ_STAGE_ONLY
    uint32_t cur[Q6K_UNIT_DW];
    load_unit(cur, lir);
#endif
    if (tid < totb) put_ablk(tid, ab);
    for (int g = tid + WGS; g < totb; g += WGS) {
        load_ablk(g, ab);
        put_ablk(g, ab);
    }
    __syncthreads();
#endif

#ifndef QG_KQ_STAGE_ONLY
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
                if (m < M) QG_KQ_OUT(m) = acc[m];
        }
    }
#endif
