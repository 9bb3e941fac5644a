// qg_q6k_mmq_body.inc — the weight loads and the K loop of the Q6_K MFMA prefill, included as text into
// q6k_mmq_kernel (qg_q6k_mmq.hip, where the work decomposition is described) and q6k_moe_mmq_kernel
// (qg_moe_prefill.hip). Text and not a function both call: the compiler sees the same tokens in the same function as
// before, so the shipped code objects do not move (DESIGN.md 3c). It leaves the wave's partial tile in acc[TT][4].
// Expects in scope: TT, RG, KS, NBUF, NR, NT, SUMI; nb, nsb, ks, r16, q, n0, N; wq, wh[4] (the lane's operand and
// header rows), stage (the slice's LDS buffers); load_tile(dst, sb, t) and store_tile(src, buf), the includer's
// activation loads; and, used by the SUMI branch alone, m0, M, out.
    struct wregs {
        uint32_t ql[4][3];  // 8 bytes at 32 i + 8q of ql (+ the realignment dword)
        uint32_t qh[2][3];  // 8 bytes at 32 h + 8q of qh
        uint32_t hd[4][5];  // scales[16] and d of the result lane's four rows
    };
    auto load_weights = [&](wregs& w, int sb) {
        const uint8_t* sbp = wq + (long)sb * Q6K_BYTES + 8 * q;
#pragma unroll
        for (int i = 0; i < 4; ++i) q6k_load<2>(sbp + 32 * i, w.ql[i]);
#pragma unroll
        for (int h = 0; h < 2; ++h) q6k_load<2>(sbp + Q6K_QH + 32 * h, w.qh[h]);
#pragma unroll
        for (int e = 0; e < 4; ++e) q6k_load<4>(wh[e] + (long)sb * Q6K_BYTES + Q6K_SC, w.hd[e]);
    };

    float acc[TT][4];
#pragma unroll
    for (int t = 0; t < TT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t][e] = 0.0f;
    const v4i zero = {0, 0, 0, 0};
    // the A operand of the s0 MFMA keeps lanes q < 2 (elements 0..15 of the block), that of the s1 MFMA the others
    const uint32_t keep0 = q < 2 ? 0xFFFFFFFFu : 0u, keep1 = ~keep0;

    const int iters = (nsb + KS - 1) / KS;  // the same for every wave
    uint32_t tl[NR + NT];
    wregs wc;
    {
        const int sb0 = min(ks, nsb - 1);
        load_tile(tl, sb0, 0);
        load_weights(wc, sb0);
    }
    for (int it = 0; it < iters; ++it) {
        const int sb = it * KS + ks;
        const bool valid = sb < nsb;  // wave-uniform
        const int sbl = min(sb, nsb - 1);  // the super-block wc holds
        const int sbn = min(sb + KS, nsb - 1);
        // realign by the parity of each row's super-block address (every piece sits at a multiple of 4 past it)
        uint32_t cl[8][2];  // the signed codes of blocks 0..7, this lane's 8 elements
        {
            const uint32_t sh = (uint32_t)((uintptr_t)(wq + (long)sbl * Q6K_BYTES) & 3);
            uint32_t l[4][2], hq[2][2];
#pragma unroll
            for (int i = 0; i < 4; ++i) q6k_realign<2>(wc.ql[i], sh, l[i]);
#pragma unroll
            for (int h = 0; h < 2; ++h) q6k_realign<2>(wc.qh[h], sh, hq[h]);
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    cl[4 * h + 0][x] = q6k_codes<0>(l[2 * h][x], l[2 * h + 1][x], hq[h][x]);
                    cl[4 * h + 1][x] = q6k_codes<1>(l[2 * h][x], l[2 * h + 1][x], hq[h][x]);
                    cl[4 * h + 2][x] = q6k_codes<2>(l[2 * h][x], l[2 * h + 1][x], hq[h][x]);
                    cl[4 * h + 3][x] = q6k_codes<3>(l[2 * h][x], l[2 * h + 1][x], hq[h][x]);
                }
        }
        uint32_t sc[4][4];
        float d[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t sh = (uint32_t)((uintptr_t)(wh[e] + (long)sbl * Q6K_BYTES) & 3);
            q6k_realign<4>(wc.hd[e], sh, sc[e]);
            d[e] = h2f((wc.hd[e][4] >> (8 * sh)) & 0xFFFFu);
        }
        static_for<TT>([&](auto T) {
            constexpr int t = decltype(T)::value;
            // this tile into the slice's LDS buffer (step parity: TT is 1 or even, so the parity is t's, or it's at
            // TT = 1), the next one (and after the last, the next super-block's weights) in flight, then the barrier
            // between the writes and the operand reads
            uint32_t* buf = stage + (NBUF > 1 ? ((TT == 1 ? it : t) & 1) * Q6K_TILE_DW : 0);
            store_tile(tl, buf);
            if constexpr (t + 1 < TT) {
                load_tile(tl, min(sb, nsb - 1), t + 1);
            } else {
                if (it + 1 < iters) {
                    load_tile(tl, sbn, 0);
                    load_weights(wc, sbn);
                }
            }
            __syncthreads();
            if (valid) {
                const uint32_t* tok = buf + r16 * Q6K_TOK_DW;
                static_for<8>([&](auto J) {
                    constexpr int j = decltype(J)::value;
                    const uint32_t b0 = tok[9 * j + 1 + 2 * q], b1 = tok[9 * j + 2 + 2 * q];
                    const long bfr = (long)(((unsigned long)b1 << 32) | b0);
                    const long a0 = (long)(((unsigned long)(cl[j][1] & keep0) << 32) | (cl[j][0] & keep0));
                    const long a1 = (long)(((unsigned long)(cl[j][1] & keep1) << 32) | (cl[j][0] & keep1));
                    const v4i c0 = __builtin_amdgcn_mfma_i32_16x16x32_i8(a0, bfr, zero, 0, 0, 0);
                    const v4i c1 = __builtin_amdgcn_mfma_i32_16x16x32_i8(a1, bfr, zero, 0, 0, 0);
                    float da = 0.0f;
                    if constexpr (!SUMI) da = h2f(tok[9 * j] & 0xFFFFu);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int isum = q6k_scale<2 * j>(sc[e]) * c0[e] + q6k_scale<2 * j + 1>(sc[e]) * c1[e];
                        if constexpr (SUMI) {
                            const int m = m0 + 16 * t + r16, n = n0 + 4 * q + e;
                            if (m < M && n < N) static_cast<int32_t*>(out)[((long)m * N + n) * nb + 8 * sb + j] = isum;
                        } else {
                            acc[t][e] = __builtin_fmaf(d[e] * da, (float)isum, acc[t][e]);
                        }
                    }
                    // a block's two MFMAs and their epilogue stay together: scheduled freely, hipcc issues the
                    // tile's MFMAs first and holds all their results
                    __builtin_amdgcn_sched_barrier(0);
                });
            }
        });
    }
