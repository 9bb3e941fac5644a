// qg_q3k_mmq_body.inc — the weight loads and the K loop of the Q3_K MFMA prefill, included as text into
// q3k_mmq_kernel (qg_q3k_mmq.hip, where the work decomposition is described). Its own text, as the K-quant bodies
// (DESIGN.md 3c), so that an expert-grouped launch can include it later. It leaves the wave's partial tile in
// acc[TT][4]: lane (r16, q) holds weight row r16 x tokens 4q .. 4q + 3 of each tile.
// Expects in scope: TT, RG, KS, NBUF, NR, NT, SUMI; nb, nsb, ks, r16, q, n0, N; wq (the lane's weight row), stage
// (the slice's LDS buffers); load_tile(dst, sb, t) and store_tile(src, buf), the includer's activation loads; and,
// used by the SUMI branch alone, m0, M, out.
    struct wregs {
        uint32_t hm[3];     // hmask[8q .. 8q + 7] (+ the realignment dword)
        uint32_t qs[2][3];  // qs[32h + 8q .. + 7]
        uint32_t hd[4];     // scales[12] and d
    };
    auto load_sblock = [&](wregs& w, int sb) {
        const uint8_t* sbp = wq + (long)sb * Q3K_BYTES;
        q6k_load<2>(sbp + 8 * q, w.hm);
        q6k_load<2>(sbp + Q3K_QS + 8 * q, w.qs[0]);
        q6k_load<2>(sbp + Q3K_QS + 32 + 8 * q, w.qs[1]);
        q6k_load<3>(sbp + Q3K_SC, w.hd);
    };

    float acc[TT][4];
#pragma unroll
    for (int t = 0; t < TT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t][e] = 0.0f;
    const v4i zero = {0, 0, 0, 0};
    const uint32_t gsh = 8 * (q >> 1);  // lanes q < 2 hold elements 0..15 of a block (group 2b), the others group 2b + 1

    const int iters = (nsb + KS - 1) / KS;  // the same for every wave
    uint32_t tl[NR + NT];
    wregs wc;
    {
        const int sb0 = min(ks, nsb - 1);
        load_tile(tl, sb0, 0);
        load_sblock(wc, sb0);
    }
    for (int it = 0; it < iters; ++it) {
        const int sb = it * KS + ks;
        const bool valid = sb < nsb;  // wave-uniform
        const int sbl = min(sb, nsb - 1);  // the super-block wc holds
        const int sbn = min(sb + KS, nsb - 1);
        long bfr[8];  // (4 - u) s of this lane's 8 elements of blocks 0..7
        float nd;     // -d: the operand carries (-q) s
        {
            // realign by the parity of the super-block's address (every piece sits at a multiple of 4 past it)
            const uint32_t sh = (uint32_t)((uintptr_t)(wq + (long)sbl * Q3K_BYTES) & 3);
            uint32_t hm[2], qv[2][2], sw[3];
            q6k_realign<2>(wc.hm, sh, hm);
            q6k_realign<2>(wc.qs[0], sh, qv[0]);
            q6k_realign<2>(wc.qs[1], sh, qv[1]);
            q6k_realign<3>(wc.hd, sh, sw);
            nd = -h2f((wc.hd[3] >> (8 * sh)) & 0xFFFFu);
            const q3k_scales s = q3k_unpack_scales(sw[0], sw[1], sw[2]);
            static_for<8>([&](auto Bk) {
                constexpr int b = decltype(Bk)::value, h = b >> 2, j = b & 3;
                // group 2b + (q >> 1): byte 2 (b & 1) + (q >> 1) of scale dword b / 2
                const uint32_t p = (s.sc[b >> 1] >> (16 * (b & 1) + gsh)) & 0xFFu;
                const uint32_t lo = q3k_table_lo(p), hi = q3k_table_hi(p);
                uint32_t wv[2];
#pragma unroll
                for (int x = 0; x < 2; ++x) {
                    // hmask bit b to bit 2 of each byte
                    uint32_t hb;
                    if constexpr (b >= 2) hb = hm[x] >> (b - 2);
                    else hb = hm[x] << (2 - b);
                    const uint32_t u = ((qv[h][x] >> (2 * j)) & 0x03030303u) | (hb & 0x04040404u);
                    wv[x] = q3k_lookup(u, lo, hi);
                }
                bfr[b] = (long)(((unsigned long)wv[1] << 32) | wv[0]);
            });
        }
        static_for<TT>([&](auto T) {
            constexpr int t = decltype(T)::value;
            // this tile into the slice's LDS buffer (step parity: TT is 1 or even, so the parity is t's, or it's at
            // TT = 1), the next one (and after the last, the next super-block's weights) in flight, then the barrier
            // between the writes and the operand reads
            uint32_t* buf = stage + (NBUF > 1 ? ((TT == 1 ? it : t) & 1) * Q3K_TILE_DW : 0);
            store_tile(tl, buf);
            if constexpr (t + 1 < TT) {
                load_tile(tl, min(sb, nsb - 1), t + 1);
            } else {
                if (it + 1 < iters) {
                    load_tile(tl, sbn, 0);
                    load_sblock(wc, sbn);
                }
            }
            __syncthreads();
            if (valid) {
                const uint32_t* tok = buf + r16 * Q3K_TOK_DW;    // the operand: token r16
                const uint32_t* res = buf + 4 * q * Q3K_TOK_DW;  // the results: tokens 4q .. 4q + 3
                static_for<8>([&](auto J) {
                    constexpr int j = decltype(J)::value;
                    const uint32_t a0 = tok[9 * j + 1 + 2 * q], a1 = tok[9 * j + 2 + 2 * q];
                    const long afr = (long)(((unsigned long)a1 << 32) | a0);
                    const v4i c = __builtin_amdgcn_mfma_i32_16x16x32_i8(afr, bfr[j], zero, 0, 0, 0);  // -isum_j
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if constexpr (SUMI) {
                            const int m = m0 + 16 * t + 4 * q + e, n = n0 + r16;
                            if (m < M && n < N) static_cast<int32_t*>(out)[((long)m * N + n) * nb + 8 * sb + j] = -c[e];
                        } else {
                            const float da = h2f(res[e * Q3K_TOK_DW + 9 * j] & 0xFFFFu);
                            acc[t][e] = __builtin_fmaf(nd * da, (float)c[e], acc[t][e]);
                        }
                    }
                    // a pair of MFMAs and their epilogues stay together: scheduled freely, hipcc issues the tile's
                    // 8 MFMAs first and holds all their results
                    if constexpr (j % 2 == 1) __builtin_amdgcn_sched_barrier(0);
                });
            }
        });
    }
