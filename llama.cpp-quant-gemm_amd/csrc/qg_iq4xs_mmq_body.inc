// qg_iq4xs_mmq_body.inc — the weight loads and the K loop of the IQ4_XS MFMA prefill, included as text into
// iq4xs_mmq_kernel (qg_iq4xs_mmq.hip, where the work decomposition is described). Its own text, as the K-quant bodies
// (DESIGN.md 3c), so that an expert-grouped launch can include it later. It leaves the wave's partial tile in
// acc[TT][4]: lane (r16, q) holds weight row r16 x tokens 4q .. 4q + 3 of each tile.
// Expects in scope: TT, RG, KS, NBUF, NR, NT, SUMI; nb, nsb, ks, r16, q, n0, N; wq (the lane's weight row), stage
// (the slice's LDS buffers); load_tile(dst, sb, t) and store_tile(src, buf), the includer's activation loads; and,
// used by the SUMI branch alone, m0, M, out.
    struct wregs {
        uint2 hd;     // d | scales_h << 16, scales_l
        uint2 qs[8];  // sub-block j: qs bytes 16j + 8 (q & 1) .. + 7
    };
    auto load_sblock = [&](wregs& w, int sb) {
        const uint2* p = reinterpret_cast<const uint2*>(wq + (long)sb * IQ4XS_BYTES);
        w.hd = p[0];
#pragma unroll
        for (int j = 0; j < 8; ++j) w.qs[j] = p[1 + 2 * j + (q & 1)];
    };

    float acc[TT][4];
#pragma unroll
    for (int t = 0; t < TT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[t][e] = 0.0f;
    const v4i zero = {0, 0, 0, 0};
    const uint32_t nib = 4 * (q >> 1);  // lanes q < 2 hold elements 0..15 (low nibbles), the others 16..31

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
        const int sbn = min(sb + KS, nsb - 1);
        long bfr[8];  // kv of this lane's 8 elements of sub-blocks 0..7
#pragma unroll
        for (int j = 0; j < 8; ++j)
            bfr[j] = (long)(((unsigned long)iq4xs_kv4(wc.qs[j].y >> nib) << 32) | iq4xs_kv4(wc.qs[j].x >> nib));
        const iq4xs_scales s = iq4xs_unpack_scales(wc.hd.x, wc.hd.y);
        const float d = h2f(wc.hd.x & 0xFFFFu);
        static_for<TT>([&](auto T) {
            constexpr int t = decltype(T)::value;
            // this tile into the slice's LDS buffer (step parity: TT is 1 or even, so the parity is t's, or it's at
            // TT = 1), the next one (and after the last, the next super-block's weights) in flight, then the barrier
            // between the writes and the operand reads
            uint32_t* buf = stage + (NBUF > 1 ? ((TT == 1 ? it : t) & 1) * IQ4XS_TILE_DW : 0);
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
                const uint32_t* tok = buf + r16 * IQ4XS_TOK_DW;    // the operand: token r16
                const uint32_t* res = buf + 4 * q * IQ4XS_TOK_DW;  // the results: tokens 4q .. 4q + 3
                float inner[4] = {0.0f, 0.0f, 0.0f, 0.0f};         // sum_j d_a * float((ls_j - 32) * sumi_j)
                static_for<8>([&](auto J) {
                    constexpr int j = decltype(J)::value;
                    const uint32_t a0 = tok[9 * j + 1 + 2 * q], a1 = tok[9 * j + 2 + 2 * q];
                    const long afr = (long)(((unsigned long)a1 << 32) | a0);
                    const v4i c = __builtin_amdgcn_mfma_i32_16x16x32_i8(afr, bfr[j], zero, 0, 0, 0);
                    const int ls = iq4xs_ls<j>(s);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        if constexpr (SUMI) {
                            const int m = m0 + 16 * t + 4 * q + e, n = n0 + r16;
                            if (m < M && n < N) static_cast<int32_t*>(out)[((long)m * N + n) * nb + 8 * sb + j] = c[e];
                        } else {
                            const float da = h2f(res[e * IQ4XS_TOK_DW + 9 * j] & 0xFFFFu);
                            inner[e] = __builtin_fmaf(da, (float)(ls * c[e]), inner[e]);
                        }
                    }
                    // a pair of MFMAs and their epilogues stay together: scheduled freely, hipcc issues the tile's
                    // 8 MFMAs first and holds all their results
                    if constexpr (j % 2 == 1) __builtin_amdgcn_sched_barrier(0);
                });
                if constexpr (!SUMI) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[t][e] = __builtin_fmaf(d, inner[e], acc[t][e]);
                }
            }
        });
    }
