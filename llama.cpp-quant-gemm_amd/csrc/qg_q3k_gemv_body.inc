// qg_q3k_gemv_body.inc — the body of the Q3_K decode GEMV, included as text into q3k_gemv_kernel (qg_q3k_gemv.hip,
// where the work decomposition is described) and q3k_moe_body (qg_moe.hip). Text and not a function they call, as the
// K-quant bodies (DESIGN.md 3c): one instantiation per (K, M) form, the same tokens in the single call and in the
// expert entry, so a slot's bits are the single call's.
// Expects in scope: A, B (the operands), M, N, K, out, ldc, the template parameters or constants MT, LPR, WGS, SUMI,
// ONE, and three macros, the lines in which the includers differ:
//   QG_KQ_DECLARE_TILE  the declaration of `const int tile` in the kernel, nothing where tile is a parameter
//   QG_KQ_ABLK(g)       the address of activation block g = m * K/32 + b: `A + (long)g * 9` for dense rows
//   QG_KQ_OUT(m)        the output of token m at this lane's row: `C[m * ldc + row]`
    constexpr int RPW = 64 / LPR;
    constexpr int RPB = (WGS / 64) * RPW;  // rows per workgroup
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];

    const int nb = K / QK, nsb = K / SB_ELEMS;
    const int U = 4 * nsb;  // units per row
    const int tid = threadIdx.x, lane = tid & 63, lir = lane % LPR;
    QG_KQ_DECLARE_TILE
    const int row = tile * RPB + (tid >> 6) * RPW + lane / LPR;
    const bool row_ok = row < N;
    const uint8_t* wrow = B + (long)(row_ok ? row : 0) * ((long)nsb * Q3K_BYTES);
    // unit u = blocks 4h + par and 4h + par + 2 of super-block u / 4 (h = (u / 2) % 2, par = u % 2): qs[32h .. 32h + 31],
    // hmask[0 .. 31], scales[12] and d (units past the row's end are clamped to its last one: loaded, never used)
    auto load_unit = [&](uint32_t (&dst)[Q3K_UNIT_DW], int u) {
        const int uc = min(u, U - 1);
        const int h = (uc >> 1) & 1;
        const uint8_t* sbp = wrow + (long)(uc >> 2) * Q3K_BYTES;
        uint32_t qv[9], hm[9], s4[4];
        q6k_load<8>(sbp + Q3K_QS + 32 * h, qv);
        q6k_load<8>(sbp, hm);
        q6k_load<3>(sbp + Q3K_SC, s4);
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            dst[i] = qv[i];
            dst[9 + i] = hm[i];
        }
        dst[18] = s4[0]; dst[19] = s4[1]; dst[20] = s4[2]; dst[21] = s4[3];
    };

    // 1) this thread's first activation block, 2) the lane's first unit, 3) the LDS records
    const int totb = M * nb;
    auto load_ablk = [&](int g, uint32_t (&d)[9]) {
        const uint32_t* p = QG_KQ_ABLK(g);
#pragma unroll
        for (int i = 0; i < 9; ++i) d[i] = p[i];
    };
    auto put_ablk = [&](int g, const uint32_t (&d)[9]) {
        const int m = g / nb, b = g - m * nb;
        uint32_t* rec = lds + (m * nsb + (b >> 3)) * Q3K_REC_DW;
        uint32_t* qs = rec + (b & 7) * 8;
        *reinterpret_cast<uint4*>(qs) = make_uint4(d[1], d[2], d[3], d[4]);
        *reinterpret_cast<uint4*>(qs + 4) = make_uint4(d[5], d[6], d[7], d[8]);
        rec[64 + (b & 7)] = __float_as_uint(h2f(d[0] & 0xFFFFu));
    };
    uint32_t ab[9];
    if (tid < totb) load_ablk(tid, ab);
    uint32_t cur[Q3K_UNIT_DW];
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

    auto do_unit = [&](const uint32_t (&w)[Q3K_UNIT_DW], int u) {
        const int sb = u >> 2, h = (u >> 1) & 1, par = u & 1;
        // the parity of this super-block's address: all its pieces sit at multiples of 4 past it
        const uint32_t sh = (uint32_t)((uintptr_t)(wrow + (long)sb * Q3K_BYTES) & 3);
        uint32_t raw[9], qv[8], hm[8], sw[3];
#pragma unroll
        for (int i = 0; i < 9; ++i) raw[i] = w[i];
        q6k_realign<8>(raw, sh, qv);
#pragma unroll
        for (int i = 0; i < 9; ++i) raw[i] = w[9 + i];
        q6k_realign<8>(raw, sh, hm);
        const uint32_t sraw[4] = {w[18], w[19], w[20], w[21]};
        q6k_realign<3>(sraw, sh, sw);
        const float d = h2f((w[21] >> (8 * sh)) & 0xFFFFu);  // the two bytes behind the scales
        // the biased scales of groups 8h .. 8h + 3 (L[0]) and 8h + 4 .. 8h + 7 (L[1]), one per byte: the half's nibble
        // of scales[0..7] and its bit pairs of scales[8..11]
        const uint32_t hs = sw[2] >> (4 * h);
        const uint32_t L[2] = {((sw[0] >> (4 * h)) & 0x0F0F0F0Fu) | ((hs << 4) & 0x30303030u),
                               ((sw[1] >> (4 * h)) & 0x0F0F0F0Fu) | ((hs << 2) & 0x30303030u)};
        // block x (j = par + 2x) has the groups 8h + 2j, + 1: bytes 2 par, 2 par + 1 of L[x]; their tables
        uint32_t tlo[2][2], thi[2][2];
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const uint32_t p = (L[x] >> (16 * par + 8 * k)) & 0xFFu;
                tlo[x][k] = q3k_table_lo(p);
                thi[x][k] = q3k_table_hi(p);
            }
        // the pre-scaled weights (4 - u) s of the two blocks, in the order of the activation block's dwords; decoded
        // once and reused by every token. hmask bit 4h + j sits at bit 0 (x = 0) and bit 2 (x = 1) of t's bytes.
        uint32_t q[2][8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint32_t t = hm[i] >> (4 * h + par);
            const uint32_t u0 = ((qv[i] >> (2 * par)) & 0x03030303u) | ((t << 2) & 0x04040404u);
            const uint32_t u1 = ((qv[i] >> (2 * par + 4)) & 0x03030303u) | (t & 0x04040404u);
            q[0][i] = q3k_lookup(u0, tlo[0][i >> 2], thi[0][i >> 2]);
            q[1][i] = q3k_lookup(u1, tlo[1][i >> 2], thi[1][i >> 2]);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < M) {
                const uint32_t* rec = lds + (m * nsb + sb) * Q3K_REC_DW;
                int isum[2];
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    const int blk = 4 * h + par + 2 * x;
                    const uint4 a0 = *reinterpret_cast<const uint4*>(rec + blk * 8);
                    const uint4 a1 = *reinterpret_cast<const uint4*>(rec + blk * 8 + 4);
                    int s = __builtin_amdgcn_sdot4((int)q[x][0], (int)a0.x, 0, false);
                    s = __builtin_amdgcn_sdot4((int)q[x][1], (int)a0.y, s, false);
                    s = __builtin_amdgcn_sdot4((int)q[x][2], (int)a0.z, s, false);
                    s = __builtin_amdgcn_sdot4((int)q[x][3], (int)a0.w, s, false);
                    s = __builtin_amdgcn_sdot4((int)q[x][4], (int)a1.x, s, false);
                    s = __builtin_amdgcn_sdot4((int)q[x][5], (int)a1.y, s, false);
                    s = __builtin_amdgcn_sdot4((int)q[x][6], (int)a1.z, s, false);
                    s = __builtin_amdgcn_sdot4((int)q[x][7], (int)a1.w, s, false);
                    isum[x] = -s;  // the operand is (-q) s
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
            uint32_t nxt[Q3K_UNIT_DW];
            if (j + 1 < iters) load_unit(nxt, u + LPR);
            if (u < U) do_unit(cur, u);
            if (j + 1 < iters) {
#pragma unroll
                for (int v = 0; v < Q3K_UNIT_DW; ++v) cur[v] = nxt[v];
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
