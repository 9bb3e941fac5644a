// qg_q4k_mmq_body.inc — the weight loads and the K loop of the Q4_K MFMA prefill, included as text into
// q4k_mmq_kernel (qg_q4k_mmq.hip, where the work decomposition is described) and q4k_moe_mmq_kernel
// (qg_moe_prefill.hip). Text and not a function both call: the compiler sees the same tokens in the same function as
// before, so the shipped code objects do not move (DESIGN.md 3c). It leaves the wave's partial tile in acc[TT][4].
// Expects in scope: TT, RG, KS, NBUF, NR, NT, SUMI; nb, nsb, ks, r16, q, n0, N; wq, wh[4] (the lane's operand and
// header rows), stage (the slice's LDS buffers); load_tile(dst, sb, t) and store_tile(src, buf), the includer's
// activation loads; and, used by the SUMI branch alone, m0, M, out.
    struct wregs {
        uint2 qs[4];
        uint4 hd[4];
    };
    auto load_weights = [&](wregs& w, int sb) {
#pragma unroll
        for (int i = 0; i < 4; ++i) w.qs[i] = *reinterpret_cast<const uint2*>(wq + (long)sb * Q4K_BYTES + 32 * i);
#pragma unroll
        for (int e = 0; e < 4; ++e) w.hd[e] = *reinterpret_cast<const uint4*>(wh[e] + (long)sb * Q4K_BYTES);
    };

    float acc[TT][4];
#pragma unroll
    for (int t = 0; t < TT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t][e] = 0.0f;
    const v4i zero = {0, 0, 0, 0};

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
        const int sbn = min(sb + KS, nsb - 1);
        long afr[8];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint2 v = wc.qs[i];
            const uint32_t l0 = v.x & 0x0F0F0F0Fu, l1 = v.y & 0x0F0F0F0Fu;
            const uint32_t h0 = (v.x >> 4) & 0x0F0F0F0Fu, h1 = (v.y >> 4) & 0x0F0F0F0Fu;
            afr[2 * i] = (long)(((unsigned long)l1 << 32) | l0);
            afr[2 * i + 1] = (long)(((unsigned long)h1 << 32) | h0);
        }
        q4k_scales s[4];
        float d[4], dmin[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            s[e] = q4k_unpack_scales(wc.hd[e].y, wc.hd[e].z, wc.hd[e].w);
            d[e] = h2f(wc.hd[e].x & 0xFFFFu);
            dmin[e] = h2f(wc.hd[e].x >> 16);
        }
        static_for<TT>([&](auto T) {
            constexpr int t = decltype(T)::value;
            // this tile into the slice's LDS buffer (step parity: TT is 1 or even, so the parity is t's, or it's at
            // TT = 1), the next one (and after the last, the next super-block's weights) in flight, then the barrier
            // between the writes and the operand reads
            uint32_t* buf = stage + (NBUF > 1 ? ((TT == 1 ? it : t) & 1) * Q4K_TILE_DW : 0);
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
                const uint32_t* tok = buf + r16 * Q4K_TOK_DW;
                static_for<8>([&](auto J) {
                    constexpr int j = decltype(J)::value;
                    const uint32_t b0 = tok[9 * j + 1 + 2 * q], b1 = tok[9 * j + 2 + 2 * q];
                    const long bfr = (long)(((unsigned long)b1 << 32) | b0);
                    const v4i c = __builtin_amdgcn_mfma_i32_16x16x32_i8(afr[j], bfr, zero, 0, 0, 0);
                    if constexpr (SUMI) {
                        const int m = m0 + 16 * t + r16;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int n = n0 + 4 * q + e;
                            if (m < M && n < N) static_cast<int32_t*>(out)[((long)m * N + n) * nb + 8 * sb + j] = c[e];
                        }
                    } else {
                        const uint32_t ds = tok[9 * j];
                        const float da = h2f(ds & 0xFFFFu), sa = h2f(ds >> 16);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float dsc = d[e] * (float)q4k_byte<j>(s[e].sc);
                            const float dm = -(dmin[e] * (float)q4k_byte<j>(s[e].mn));
                            acc[t][e] = __builtin_fmaf(dsc * da, (float)c[e], acc[t][e]);
                            acc[t][e] = __builtin_fmaf(dm, sa, acc[t][e]);
                        }
                    }
                    // a chunk's two MFMAs and their epilogues stay together: scheduled freely, hipcc issues the
                    // tile's 8 MFMAs first and holds all their results
                    if constexpr (j % 2 == 1) __builtin_amdgcn_sched_barrier(0);
                });
            }
        });
    }
