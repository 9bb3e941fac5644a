// qg_iq4xs_gemv_body.inc — the body of the IQ4_XS decode GEMV, included as text into iq4xs_gemv_kernel
// (qg_iq4xs_gemv.hip, where the work decomposition is described) and iq4xs_moe_body (qg_moe.hip). Text and not a
// function they call, as the K-quant bodies (DESIGN.md 3c): one instantiation per (K, M) form, the same tokens in the
// single call and in the expert entry, so a slot's bits are the single call's.
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
    const uint8_t* wrow = B + (long)(row_ok ? row : 0) * ((long)nsb * IQ4XS_BYTES);
    // unit u = sub-blocks 2i, 2i + 1 of super-block u / 4 (i = u % 4): the header and four 8-B pieces of qs, all at
    // multiples of 8 inside the super-block (units past the row's end are clamped to its last one: loaded, never used)
    auto load_unit = [&](uint32_t (&dst)[IQ4XS_UNIT_DW], int u) {
        const int uc = min(u, U - 1);
        const uint2* sbp = reinterpret_cast<const uint2*>(wrow + (long)(uc >> 2) * IQ4XS_BYTES);
        const uint2 h = sbp[0];
        const uint2* qp = sbp + 1 + 4 * (uc & 3);
        dst[0] = h.x; dst[1] = h.y;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const uint2 v = qp[x];
            dst[2 + 2 * x] = v.x; dst[3 + 2 * x] = v.y;
        }
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
        uint32_t* rec = lds + (m * nsb + (b >> 3)) * IQ4XS_REC_DW;
        uint32_t* qs = rec + (b & 7) * 8;
        *reinterpret_cast<uint4*>(qs) = make_uint4(d[1], d[2], d[3], d[4]);
        *reinterpret_cast<uint4*>(qs + 4) = make_uint4(d[5], d[6], d[7], d[8]);
        rec[64 + (b & 7)] = __float_as_uint(h2f(d[0] & 0xFFFFu));
    };
    uint32_t ab[9];
    if (tid < totb) load_ablk(tid, ab);
    uint32_t cur[IQ4XS_UNIT_DW];
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

    auto do_unit = [&](const uint32_t (&w)[IQ4XS_UNIT_DW], int u) {
        const int sb = u >> 2, i = u & 3;
        // kv of sub-block 2i + s: q[s][t] elements 4t .. 4t + 3 (low nibbles), q[s][4 + t] elements 16 + 4t .. (high),
        // the order of the activation block's dwords; decoded once and reused by every token
        uint32_t q[2][8];
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const uint32_t v = w[2 + 4 * s + t];
                q[s][t] = iq4xs_kv4(v);
                q[s][4 + t] = iq4xs_kv4(v >> 4);
            }
        // ls - 32 of sub-blocks 2i, 2i + 1: the two nibbles of scales_l[i], bits 4i .. 4i + 3 of scales_h (the two of
        // the unit alone; iq4xs_unpack_scales would assemble all eight)
        const uint32_t sl = w[1] >> (8 * i), sh = w[0] >> (16 + 4 * i);
        const int ls0 = (int)((sl & 15u) | ((sh & 3u) << 4)) - 32;
        const int ls1 = (int)(((sl >> 4) & 15u) | (((sh >> 2) & 3u) << 4)) - 32;
        const float d = h2f(w[0] & 0xFFFFu);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
            if (m < M) {
                const uint32_t* rec = lds + (m * nsb + sb) * IQ4XS_REC_DW;
                uint32_t a[16];
#pragma unroll
                for (int x = 0; x < 4; ++x) {
                    const uint4 t = *reinterpret_cast<const uint4*>(rec + 16 * i + 4 * x);
                    a[4 * x] = t.x; a[4 * x + 1] = t.y; a[4 * x + 2] = t.z; a[4 * x + 3] = t.w;
                }
                const int s0 = dot_block(q[0], a), s1 = dot_block(q[1], a + 8);
                if constexpr (SUMI) {
                    if (row_ok) {
                        int32_t* o = sumi_out + ((long)m * N + row) * nb + 8 * sb + 2 * i;
                        o[0] = s0;
                        o[1] = s1;
                    }
                } else {
                    const uint2 da = *reinterpret_cast<const uint2*>(rec + 64 + 2 * i);  // d_a of 2i, 2i + 1
                    const float fd = __uint_as_float(da.x) * (float)(ls0 * s0) + __uint_as_float(da.y) * (float)(ls1 * s1);
                    acc[m] += d * fd;
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
            uint32_t nxt[IQ4XS_UNIT_DW];
            if (j + 1 < iters) load_unit(nxt, u + LPR);
            if (u < U) do_unit(cur, u);
            if (j + 1 < iters) {
#pragma unroll
                for (int v = 0; v < IQ4XS_UNIT_DW; ++v) cur[v] = nxt[v];
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
