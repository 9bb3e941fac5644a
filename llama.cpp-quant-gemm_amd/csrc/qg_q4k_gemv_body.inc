// qg_q4k_gemv_body.inc — the body of the Q4_K decode GEMV, included as text into q4k_gemv_kernel (qg_q4k_gemv.hip,
// where the work decomposition is described) and q4k_moe_body (qg_moe.hip) and
// q4k_moeb_kernel (qg_moe_batch.hip) and q4k_glu_product[_staged] (qg_moe_glu.hip) and q4k_down_stage /
// q4k_down_product (qg_moe_down.hip). Text and not a function they
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
#endif

#ifdef QG_KQ_A_STAGED
    uint32_t cur[Q4K_UNIT_DW];
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
        uint32_t* rec = lds + (m * nsb + (b >> 3)) * Q4K_REC_DW;
        uint32_t* qs = rec + (b & 7) * 8;
        *reinterpret_cast<uint4*>(qs) = make_uint4(d[1], d[2], d[3], d[4]);
        *reinterpret_cast<uint4*>(qs + 4) = make_uint4(d[5], d[6], d[7], d[8]);
        *reinterpret_cast<uint2*>(rec + 64 + (b & 7) * 2) =
            make_uint2(__float_as_uint(h2f(d[0] & 0xFFFFu)), __float_as_uint(h2f(d[0] >> 16)));
    };
    uint32_t ab[9];
    if (tid < totb) load_ablk(tid, ab);
#ifndef QG_KQ_STAGE_ONLY
    uint32_t cur[Q4K_UNIT_DW];
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
                if (m < M) QG_KQ_OUT(m) = acc[m];
        }
    }
#endif
