// qg_mxfp4_mmq_body.inc — the weight loads and the K loop of the MXFP4 MFMA prefill, included as text into
// mxfp4_mmq_kernel (qg_mxfp4_mmq.hip, where the work decomposition is described). Its own text, as the K-quant bodies
// (DESIGN.md 3c), so that an expert-grouped launch can include it later. It leaves the wave's partial tile in
// acc[TT][4]: lane (r16, q) holds weight row r16 x tokens 4q .. 4q + 3 of each tile.
// Expects in scope: TT, RG, KS, NBUF, NR, NT, SUMI; nb, ngrp, ks, r16, q, n0, N; wq (the lane's weight row), stage
// (the slice's LDS buffers); load_tile(dst, g, t) and store_tile(src, buf), the includer's activation loads; and,
// used by the SUMI branch alone, m0, M, out.
    struct wregs {
        uint32_t qs[8][3];  // the three dwords of each block's cover that hold this lane's 8 qs bytes
        uint32_t e[8];      // the cover's first dword: it holds e
    };
    // group g = blocks 8g .. 8g + 7; blocks past the row's end are clamped to its last one: loaded, never used
    auto load_blocks = [&](wregs& w, int g) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t* pa = mxfp4_cover(wq + (long)min(8 * g + j, nb - 1) * MXFP4_BYTES);
            w.e[j] = pa[0];
            // qs bytes 8 (q & 1) .. + 7 sit at bytes s + 1 + 8 (q & 1) .. of the cover: inside its dwords 0..2 or 2..4
            const uint32_t* pq = pa + 2 * (q & 1);
#pragma unroll
            for (int i = 0; i < 3; ++i) w.qs[j][i] = pq[i];
        }
    };

    float acc[TT][4];
#pragma unroll
    for (int t = 0; t < TT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t][e] = 0.0f;
    const v4i zero = {0, 0, 0, 0};
    const uint32_t nib = 4 * (q >> 1);  // lanes q < 2 hold elements 0..15 (low nibbles), the others 16..31

    const int iters = (ngrp + KS - 1) / KS;  // the same for every wave
    uint32_t tl[NR + NT];
    wregs wc;
    {
        const int g0 = min(ks, ngrp - 1);
        load_tile(tl, g0, 0);
        load_blocks(wc, g0);
    }
    for (int it = 0; it < iters; ++it) {
        const int sb = it * KS + ks;
        const bool valid = sb < ngrp;       // wave-uniform
        const int sbl = min(sb, ngrp - 1);  // the group wc holds
        const int sbn = min(sb + KS, ngrp - 1);
        long bfr[8];   // kv of this lane's 8 elements of blocks 0..7
        float sc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t s = (uint32_t)((uintptr_t)(wq + (long)min(8 * sbl + j, nb - 1) * MXFP4_BYTES) & 3);
            sc[j] = mxfp4_scale((wc.e[j] >> (8 * s)) & 0xFFu);
            const uint32_t x0 = mxfp4_align(wc.qs[j][0], wc.qs[j][1], s + 1) >> nib;
            const uint32_t x1 = mxfp4_align(wc.qs[j][1], wc.qs[j][2], s + 1) >> nib;
            bfr[j] = (long)(((unsigned long)mxfp4_kv4(x1) << 32) | mxfp4_kv4(x0));
        }
        static_for<TT>([&](auto T) {
            constexpr int t = decltype(T)::value;
            // this tile into the slice's LDS buffer (step parity: TT is 1 or even, so the parity is t's, or it's at
            // TT = 1), the next one (and after the last, the next group's weights) in flight, then the barrier
            // between the writes and the operand reads
            uint32_t* buf = stage + (NBUF > 1 ? ((TT == 1 ? it : t) & 1) * MXFP4_TILE_DW : 0);
            store_tile(tl, buf);
            if constexpr (t + 1 < TT) {
                load_tile(tl, sbl, t + 1);
            } else {
                if (it + 1 < iters) {
                    load_tile(tl, sbn, 0);
                    load_blocks(wc, sbn);
                }
            }
            __syncthreads();
            if (valid) {
                const uint32_t* tok = buf + r16 * MXFP4_TOK_DW;       // the operand: token r16
                const uint32_t* res = buf + 4 * q * MXFP4_TOK_DW;     // the results: tokens 4q .. 4q + 3
                static_for<8>([&](auto J) {
                    constexpr int j = decltype(J)::value;
                    if (8 * sb + j < nb) {  // wave-uniform: the last group of a row may be partial
                        const uint32_t a0 = tok[9 * j + 1 + 2 * q], a1 = tok[9 * j + 2 + 2 * q];
                        const long afr = (long)(((unsigned long)a1 << 32) | a0);
                        const v4i c = __builtin_amdgcn_mfma_i32_16x16x32_i8(afr, bfr[j], zero, 0, 0, 0);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            if constexpr (SUMI) {
                                const int m = m0 + 16 * t + 4 * q + e, n = n0 + r16;
                                if (m < M && n < N) static_cast<int32_t*>(out)[((long)m * N + n) * nb + 8 * sb + j] = c[e];
                            } else {
                                const float da = h2f(res[e * MXFP4_TOK_DW + 9 * j] & 0xFFFFu);
                                acc[t][e] = __builtin_fmaf(da * sc[j], (float)c[e], acc[t][e]);
                            }
                        }
                    }
                    // a pair of MFMAs and their epilogues stay together: scheduled freely, hipcc issues the tile's
                    // 8 MFMAs first and holds all their results
                    if constexpr (j % 2 == 1) __builtin_amdgcn_sched_barrier(0);
                });
            }
        });
    }
