// qg_mxfp4_gemv_body.inc — the body of the MXFP4 decode GEMV, included as text into mxfp4_gemv_kernel
// (qg_mxfp4_gemv.hip, where the work decomposition is described) and mxfp4_moe_body (qg_moe.hip) and
// mxfp4_glu_product[_staged] (qg_moe_glu.hip) and mxfp4_down_stage / mxfp4_down_product (qg_moe_down.hip). Text and
// not a function they call, as the K-quant bodies (DESIGN.md 3c): one instantiation per (K, M) form, the same tokens
// in the single call and in the expert entries, so a slot's bits are the single call's.
// Expects in scope: A, B (the operands), M, N, K, out, ldc, the template parameters or constants MT, LPR, WGS, SUMI,
// ONE, and three macros, the lines in which the includers differ:
//   QG_KQ_DECLARE_TILE  the declaration of `const int tile` in the kernel, nothing where tile is a parameter
//   QG_KQ_ABLK(g)       the address of activation block g = m * K/32 + b: `A + (long)g * 9` for dense rows
//   QG_KQ_OUT(m)        the output of token m at this lane's row: `C[m * ldc + row]`
// and four the shipped includers leave undefined (the meaning they have in qg_q4k_gemv_body.inc):
//   QG_KQ_A_STAGED      defined: the LDS records already hold the activation row (an earlier pass of the same
//                       workgroup staged it and a barrier has passed); the body loads its first unit and goes on
//   QG_KQ_STAGE_ONLY    defined: the inclusion is the staging prologue alone, the M dense activation rows into the
//                       records and its barrier: no weights, no row, no product (B, N, out, MT, SUMI, ONE are not needed)
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

    const int nb = K / QK;                        // blocks per row
    const int U = (nb + MXFP4_UB - 1) / MXFP4_UB;  // units per row: MXFP4_UB consecutive blocks each (1 as shipped)
    const int tid = threadIdx.x, lane = tid & 63, lir = lane % LPR;
#ifndef QG_KQ_STAGE_ONLY
#ifdef QG_KQ_ROW
    const int row = QG_KQ_ROW;
#else
    QG_KQ_DECLARE_TILE
    const int row = tile * RPB + (tid >> 6) * RPW + lane / LPR;
#endif
    const bool row_ok = row < N;
    const uint8_t* wrow = B + (long)(row_ok ? row : 0) * ((long)nb * MXFP4_BYTES);
    // (blocks past the row's end are clamped to its last one: loaded, never used)
    auto load_unit = [&](uint32_t (&dst)[MXFP4_UNIT_DW], int u) {
#pragma unroll
        for (int x = 0; x < MXFP4_UB; ++x) {
            uint32_t c[MXFP4_COVER_DW];
            mxfp4_load<0, MXFP4_COVER_DW>(wrow + (long)min(MXFP4_UB * u + x, nb - 1) * MXFP4_BYTES, c);
#pragma unroll
            for (int i = 0; i < MXFP4_COVER_DW; ++i) dst[MXFP4_COVER_DW * x + i] = c[i];
        }
    };
#endif

#ifdef QG_KQ_A_STAGED
    uint32_t cur[MXFP4_UNIT_DW];
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
        uint32_t* rec = lds + (long)g * MXFP4_REC_DW;
        *reinterpret_cast<uint4*>(rec) = make_uint4(d[1], d[2], d[3], d[4]);
        *reinterpret_cast<uint4*>(rec + 4) = make_uint4(d[5], d[6], d[7], d[8]);
        rec[8] = __float_as_uint(h2f(d[0] & 0xFFFFu));
    };
    uint32_t ab[9];
    if (tid < totb) load_ablk(tid, ab);
#ifndef QG_KQ_STAGE_ONLY
    uint32_t cur[MXFP4_UNIT_DW];
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

    auto do_block = [&](const uint32_t* w, int u) {  // block u of the row, its cover in w[0..4]
        // the block's offset into its cover: e is byte s of the stream, qs dword j starts at byte s + 1 + 4j
        const uint32_t s = (uint32_t)((uintptr_t)(wrow + (long)u * MXFP4_BYTES) & 3);
        const float sc = mxfp4_scale((w[0] >> (8 * s)) & 0xFFu);
        uint32_t q[8];  // kv of elements 4i .. 4i + 3, decoded once and reused by every token
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t x = mxfp4_align(w[j], w[j + 1], s + 1);
            q[j] = mxfp4_kv4(x);
            q[4 + j] = mxfp4_kv4(x >> 4);
        }
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < M) {
                const uint32_t* rec = lds + (long)(m * nb + u) * MXFP4_REC_DW;
                const uint4 a0 = *reinterpret_cast<const uint4*>(rec);
                const uint4 a1 = *reinterpret_cast<const uint4*>(rec + 4);
                int sumi = __builtin_amdgcn_sdot4((int)q[0], (int)a0.x, 0, false);
                sumi = __builtin_amdgcn_sdot4((int)q[1], (int)a0.y, sumi, false);
                sumi = __builtin_amdgcn_sdot4((int)q[2], (int)a0.z, sumi, false);
                sumi = __builtin_amdgcn_sdot4((int)q[3], (int)a0.w, sumi, false);
                sumi = __builtin_amdgcn_sdot4((int)q[4], (int)a1.x, sumi, false);
                sumi = __builtin_amdgcn_sdot4((int)q[5], (int)a1.y, sumi, false);
                sumi = __builtin_amdgcn_sdot4((int)q[6], (int)a1.z, sumi, false);
                sumi = __builtin_amdgcn_sdot4((int)q[7], (int)a1.w, sumi, false);
                if constexpr (SUMI) {
                    if (row_ok) sumi_out[((long)m * N + row) * nb + u] = sumi;
                } else {
                    acc[m] += (__uint_as_float(rec[8]) * sc) * (float)sumi;
                }
            }
        }
    };

    auto do_unit = [&](const uint32_t (&w)[MXFP4_UNIT_DW], int u) {
#pragma unroll
        for (int x = 0; x < MXFP4_UB; ++x)
            if (MXFP4_UB * u + x < nb) do_block(w + MXFP4_COVER_DW * x, MXFP4_UB * u + x);
    };

    if constexpr (ONE) {
        if (lir < U) do_unit(cur, lir);
    } else {
        const int iters = (U + LPR - 1) / LPR;
        for (int j = 0; j < iters; ++j) {
            const int u = lir + j * LPR;
            uint32_t nxt[MXFP4_UNIT_DW];
            if (j + 1 < iters) load_unit(nxt, u + LPR);
            if (u < U) do_unit(cur, u);
            if (j + 1 < iters) {
#pragma unroll
                for (int v = 0; v < MXFP4_UNIT_DW; ++v) cur[v] = nxt[v];
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
