// qg_api.hip — the C-ABI (include/qg/qg.h): validation, dispatch, error reporting.
//
// Every entry point validates, picks a kernel family and enqueues on the caller's stream, so
// callers may capture it into a hipGraph. Validation is one ordered precheck (below) plus what is specific
// to an entry; the quantized product has one entry, run_product. The library's workspaces live in
// qg_workspace.hip, the capture-time merge of GEMVs in qg_capture_fuse.hip.
#include <string.h>

#include <cmath>

#include <initializer_list>

#include "../../include/qg/qg.h"
#include "qg_kernels.hpp"
#include "qg_moe_batch.hpp"
#include "qg_moe_down.hpp"
#include "qg_moe_glu.hpp"
#include "qg_moe_prefill.hpp"
#include "qg_mxfp4.hpp"
#include "qg_q4k.hpp"
#include "qg_q6k.hpp"

using namespace qg;

namespace qg {
int block_bytes(int t) {
    switch (t) {
        case QG_TYPE_Q4_0: return 18;
        case QG_TYPE_Q4_1: return 20;
        case QG_TYPE_Q5_0: return 22;
        case QG_TYPE_Q5_1: return 24;
        case QG_TYPE_Q8_0: return 34;
        case QG_TYPE_Q8_1: return 36;
        case QG_TYPE_Q4_K: return 144;
        case QG_TYPE_Q6_K: return 210;
        case QG_TYPE_MXFP4: return MXFP4_BYTES;
    }
    return 0;
}
}  // namespace qg

namespace {
thread_local int g_last_hip = 0;

int hip_status(hipError_t e) {
    if (e == hipSuccess) return QG_OK;
    g_last_hip = (int)e;
    return QG_ERR_HIP;
}

bool is_weight_type(int t) {
    return t == QG_TYPE_Q4_0 || t == QG_TYPE_Q4_1 || t == QG_TYPE_Q5_0 || t == QG_TYPE_Q5_1 || t == QG_TYPE_Q8_0;
}

// The super-block types (256 elements: Q4_K, Q6_K): taken by the entries that go through run_product with
// sb_ok; every other entry tests is_weight_type alone and so keeps refusing them.
bool is_q4k_type(int t) { return t == QG_TYPE_Q4_K; }
bool is_q6k_type(int t) { return t == QG_TYPE_Q6_K; }
bool is_sb_type(int t) { return is_q4k_type(t) || is_q6k_type(t); }

// MXFP4 (32 elements in 17 bytes): a route of its own beside the 32-element families and the super-block types,
// taken by the same entries as the latter (run_product with sb_ok) and by qg_gemm_w4a8_moe; is_weight_type does not
// know it, so every entry that tests that alone refuses it.
bool is_mxfp4_type(int t) { return t == QG_TYPE_MXFP4; }
// the types with a route of their own: their kernels, their K granule, their weight alignment
bool is_routed_type(int t) { return is_sb_type(t) || is_mxfp4_type(t); }

int block_elems(int t) { return is_sb_type(t) ? 256 : block_bytes(t) ? 32 : 0; }

// Weight pointer alignment of a routed type: Q4_K's 144-B super-blocks are read with 16-B loads; a Q6_K
// super-block is 210 B, so its fp16 field's 2 B is all a row guarantees and the kernels realign every load; an
// MXFP4 block is 17 B of bytes, so there is no requirement at all.
uintptr_t sb_weight_mask(int t) { return is_mxfp4_type(t) ? 0u : is_q6k_type(t) ? 1u : 15u; }

// ---- the one ordered precheck ------------------------------------------------------------------------------
// The order every entry documents (qg.h): a negative size is QG_ERR_INVALID_ARG; K not a positive multiple of
// the granule is QG_ERR_BAD_K; a weight type the entry does not take is QG_ERR_UNSUPPORTED; an empty call (a
// size of 0) is a no-op, whatever its pointers; a null required pointer is QG_ERR_INVALID_ARG; a pointer
// below its alignment (mask: the low bits that must be zero) is QG_ERR_ALIGN. Nothing is enqueued on any of
// these. QG_GO: go on with what is specific to the entry.
constexpr int QG_GO = 1;  // no status: every qg_status is <= 0
struct PtrReq { const void* p; uintptr_t mask; };

int precheck(std::initializer_list<int64_t> sizes, int64_t K, int granule, bool type_ok,
             std::initializer_list<PtrReq> ptrs) {
    for (const int64_t s : sizes) if (s < 0) return QG_ERR_INVALID_ARG;
    if (K <= 0 || K % granule != 0) return QG_ERR_BAD_K;
    if (!type_ok) return QG_ERR_UNSUPPORTED;
    for (const int64_t s : sizes) if (s == 0) return QG_OK;
    for (const PtrReq& r : ptrs) if (!r.p) return QG_ERR_INVALID_ARG;
    for (const PtrReq& r : ptrs) if (((uintptr_t)r.p & r.mask) != 0) return QG_ERR_ALIGN;
    return QG_GO;
}

// The element-count entries (qg_quantize, qg_dequantize, qg_quantize_q8_1_f16_fused) keep their own order: a
// negative count is QG_ERR_BAD_K, and a count of 0 is a no-op only after the type check.
int precheck_count(int64_t k, int granule, bool type_ok, std::initializer_list<PtrReq> ptrs) {
    if (k < 0 || k % granule != 0) return QG_ERR_BAD_K;
    if (!type_ok) return QG_ERR_UNSUPPORTED;
    if (k == 0) return QG_OK;
    return precheck({}, k, granule, true, ptrs);
}

// the output of a product: C, or the debug hook's sumi
const void* out_ptr(const GemmArgs& g) { return g.C ? (const void*)g.C : (const void*)g.sumi; }

// ---- GemmArgs in one place ---------------------------------------------------------------------------------
// The activation-major product C[M][N] = A[M][K] . B[N][K]^T with dense output rows.
GemmArgs product_args(const void* A, const void* B, float* C, int M, int N, int K, int wtype) {
    GemmArgs g;
    g.A = A; g.B = B; g.C = C; g.M = M; g.N = N; g.K = K; g.wtype = wtype;
    g.ldc_m = N; g.ldc_n = 1;
    return g;
}

// The reference's weight-major form out[mw][nt] = sum_b dot(W[mw][b], A[nt][b]) (M weight rows, N tokens) ->
// activation-major (m = nt, n = mw) with output strides ldc_m = 1, ldc_n = Ntok.
GemmArgs weight_major_args(int wtype, const void* W, const void* A, float* out, int M, int N, int K) {
    GemmArgs g = product_args(A, W, out, N, M, K, wtype);
    g.ldc_m = 1; g.ldc_n = N;
    return g;
}

// The shape alone (qg_debug_config*, qg_select_algo, qg_gemm_w4a8_workspace_size): 256-B aligned stand-in
// pointers, so the shape decides, as for a real call on aligned buffers.
GemmArgs query_args(int M, int N, int K, int wtype, int sumi = 0) {
    GemmArgs g = product_args((const void*)256, (const void*)256, sumi ? nullptr : (float*)256, M, N, K, wtype);
    if (sumi) g.sumi = (int32_t*)256;
    return g;
}

// Crossover from profiles/tools_archive/mmq_probe.hip (profiles/r01_tuning/mmq_probe_smallm.txt): the dot4 GEMV
// wins up to M = 4 (its LDS activation reads grow with M), the MFMA kernel from M = 5 on.
int select_algo(const GemmArgs& g) {
    if (g.M <= 4 && gemv_eligible(g)) return QG_ALGO_GEMV;
    if (mfma_eligible(g)) return QG_ALGO_MFMA;
    if (gemv_eligible(g)) return QG_ALGO_GEMV;
    // odd K / 32 (rows off dword alignment) or 2-B aligned weights at prefill sizes: the MFMA kernel
    // on a zero-padded copy (qg_repack.hip); below that one wave per weight row (qg_ragged.hip)
    // instead of the byte-load generic kernel's one wave per output
    if (repack_eligible(g)) return QG_ALGO_MFMA;
    if (ragged_eligible(g)) return QG_ALGO_RAGGED;
    return QG_ALGO_GENERIC;
}

// The 32-element families (Q4_0 .. Q8_0) after the precheck.
int run_q32(GemmArgs& g, int algo, hipStream_t st) {
    if (g.batch < 0) return QG_ERR_INVALID_ARG;
    if (g.batch == 0) return QG_OK;
    if (g.batch > 1 && (((uintptr_t)g.sB & 1) != 0 || (g.sA & 3) != 0)) return QG_ERR_ALIGN;
    const bool auto_algo = algo == QG_ALGO_AUTO;
    if (auto_algo) algo = select_algo(g);
    if (algo == QG_ALGO_GEMV) {
        if (!gemv_eligible(g) || (g.batch > 1 && (g.sB % 16 != 0))) {
            if (g.batch == 1) return QG_ERR_UNSUPPORTED;
            algo = QG_ALGO_GENERIC;  // batch strides break the vector-load alignment: per-item path
        } else {
            if (g.batch > 65535) return QG_ERR_INVALID_ARG;
            // under stream capture, consecutive independent GEMVs become one grouped node (qg_capture_fuse.hip)
            return hip_status(launch_or_merge_gemv(g, st));
        }
    }
    // MFMA on a shape the kernel cannot address directly (odd K / 32, 2-B aligned weights): through
    // the zero-padded repack; without a workspace (stream capture) the automatic choice falls back
    if (algo == QG_ALGO_MFMA && !mfma_eligible(g) && repack_eligible(g)) {
        const hipError_t e = launch_repack_mfma(g, st);
        if (e != hipErrorNotReady) return hip_status(e);
        if (!auto_algo) return QG_ERR_UNSUPPORTED;
        algo = ragged_eligible(g) ? QG_ALGO_RAGGED : QG_ALGO_GENERIC;
    }
    // MFMA and generic kernels take one product per launch: enqueue the batch item by item.
    auto item = [&](int i) {
        GemmArgs gi = g;
        gi.batch = 1;
        gi.A = (const uint8_t*)g.A + (long)i * g.sA;
        gi.B = (const uint8_t*)g.B + (long)i * g.sB;
        if (g.C) gi.C = g.C + (long)i * g.sC;
        return gi;
    };
    // Every item is checked before the first is enqueued (a batch stride can break the MFMA
    // kernel's 16-B alignment for later items only): an explicit MFMA request fails with nothing
    // launched, an automatic choice falls back to the generic kernel for the whole batch.
    if (algo == QG_ALGO_MFMA || algo == QG_ALGO_RAGGED) {
        auto ok = [&](const GemmArgs& gi) { return algo == QG_ALGO_MFMA ? mfma_eligible(gi) : ragged_eligible(gi); };
        bool all_ok = true;
        for (int i = 0; i < g.batch && all_ok; ++i) all_ok = ok(item(i));
        if (!all_ok) {
            if (!auto_algo) return QG_ERR_UNSUPPORTED;
            algo = QG_ALGO_GENERIC;
        }
    }
    const auto launch = algo == QG_ALGO_MFMA ? launch_mfma : algo == QG_ALGO_RAGGED ? launch_ragged
                        : algo == QG_ALGO_GENERIC ? launch_generic : nullptr;
    if (!launch) return QG_ERR_INVALID_ARG;
    for (int i = 0; i < g.batch; ++i) {
        const int rc = hip_status(launch(item(i), st));
        if (rc != QG_OK) return rc;
    }
    return QG_OK;
}

// The super-block products (qg_q4k.hpp, qg_q6k.hpp): the decode GEMV up to M = 8, the MFMA prefill from M = 9 on.
// Interleaved A/B of Q4_K against a build with the threshold at 4 | 5 (profiles/q4k/ab_q4k_variants.txt,
// N = K = 4096): M = 5 GEMV 5.82 us, MFMA 7.43; M = 8 GEMV 7.31, MFMA 7.45 — the GEMV keeps M <= 8; Q6_K keeps the
// threshold ("Q6_K", 3b). The GEMV's LDS records bound M * K (gemv_eligible); beyond that AUTO takes the
// MFMA kernel at any M. Never through launch_or_merge_gemv: a captured super-block GEMV is a plain kernel node.
#ifndef QG_Q4K_GEMV_MAXM  // (A/B builds: the largest M AUTO sends to the decode GEMV)
#define QG_Q4K_GEMV_MAXM 8
#endif
#ifndef QG_Q6K_GEMV_MAXM
#define QG_Q6K_GEMV_MAXM 8
#endif
// MXFP4 keeps the threshold (profiles/mxfp4/ab_mxfp4_threshold.txt, N = K = 4096, each kernel forced): M = 5 GEMV
// 5.95 us, MFMA 12.04; M = 8 GEMV 6.99, MFMA 12.08.
#ifndef QG_MXFP4_GEMV_MAXM
#define QG_MXFP4_GEMV_MAXM 8
#endif
struct SbRoute {
    bool (*gemv_eligible)(const GemmArgs&);
    hipError_t (*launch_gemv)(const GemmArgs&, hipStream_t);
    bool (*mmq_eligible)(const GemmArgs&);
    hipError_t (*launch_mmq)(const GemmArgs&, hipStream_t);
    int maxm;
};
constexpr SbRoute SB_ROUTES[] = {  // Q4_K, Q6_K
    {q4k_gemv_eligible, launch_q4k_gemv, q4k_mmq_eligible, launch_q4k_mmq, QG_Q4K_GEMV_MAXM},
    {q6k_gemv_eligible, launch_q6k_gemv, q6k_mmq_eligible, launch_q6k_mmq, QG_Q6K_GEMV_MAXM},
};
// The third route: MXFP4 (qg_mxfp4.hpp), the same two families and the same rules, its kernels' own.
constexpr SbRoute MXFP4_ROUTE = {mxfp4_gemv_eligible, launch_mxfp4_gemv, mxfp4_mmq_eligible, launch_mxfp4_mmq,
                                 QG_MXFP4_GEMV_MAXM};
// the route of a routed type (is_routed_type holds)
const SbRoute& sb_route(int t) { return is_mxfp4_type(t) ? MXFP4_ROUTE : SB_ROUTES[is_q6k_type(t) ? 1 : 0]; }

int select_algo_sb(const GemmArgs& g) {
    const SbRoute& r = sb_route(g.wtype);
    return g.M <= r.maxm && r.gemv_eligible(g) ? QG_ALGO_GEMV : QG_ALGO_MFMA;
}

// A super-block type, or MXFP4, after the precheck.
int run_sb(GemmArgs& g, int algo, hipStream_t st) {
    const SbRoute& r = sb_route(g.wtype);
    if (algo == QG_ALGO_RAGGED || algo == QG_ALGO_GENERIC) return QG_ERR_UNSUPPORTED;
    if (algo == QG_ALGO_AUTO) algo = select_algo_sb(g);
    if (algo == QG_ALGO_GEMV) return r.gemv_eligible(g) ? hip_status(r.launch_gemv(g, st)) : QG_ERR_UNSUPPORTED;
    if (algo == QG_ALGO_MFMA) return r.mmq_eligible(g) ? hip_status(r.launch_mmq(g, st)) : QG_ERR_UNSUPPORTED;
    return QG_ERR_INVALID_ARG;
}

// The quantized product: one precheck, then the 32-element families or the route of a super-block type or of MXFP4
// by the weight type. sb_ok = false: the entries that refuse the routed types (qg.h) -- such a type is then
// one like any other they do not take, checked at the 32-element granule.
int run_product(GemmArgs& g, int algo, hipStream_t st, bool sb_ok = true) {
    const bool ksb = sb_ok && is_routed_type(g.wtype);
    // 32-element families: fp16 fields, 2-byte alignment is the floor; super-block types: 4-B activation records,
    // weights by the type (sb_weight_mask)
    const int rc = precheck({g.M, g.N}, g.K, ksb ? block_elems(g.wtype) : 32, ksb || is_weight_type(g.wtype),
                            {{g.A, ksb ? 3u : 0u}, {g.B, ksb ? sb_weight_mask(g.wtype) : 1u}, {out_ptr(g), 0}});
    if (rc != QG_GO) return rc;
    if (!ksb) return run_q32(g, algo, st);
    return run_sb(g, algo, st);
}

// what QG_ALGO_AUTO dispatches to (qg_select_algo): the same routing
int select_product_algo(const GemmArgs& g) {
    const bool ksb = is_routed_type(g.wtype);
    if (!(ksb || is_weight_type(g.wtype)) || g.K <= 0 || g.K % block_elems(g.wtype) != 0) return -1;
    if (!ksb) return select_algo(g);
    return select_algo_sb(g);
}

// The tiled weight layout (qg_tile_weights): the MFMA small-batch decode for M = 3..4 and M = 2 at K/32 > 256
// (qg_gemvm.hip), the tiled decode GEMV for the rest of M <= 4 (qg_gemvt.hip, round 6), the
// MFMA kernels beyond (LAY_TILED; odd K/32 through its activation windows). Shapes neither
// takes (ldc past INT32_MAX, activation windows of 2 GiB or more, K/32 whose records exceed the LDS at
// M <= 4 where the MFMA kernel rejects the shape too) return QG_ERR_UNSUPPORTED: the tiled layout has no
// generic kernel.
int run_tiled(GemmArgs& g, hipStream_t st) {
    const int rc = precheck({g.M, g.N}, g.K, 32, is_weight_type(g.wtype), {{g.A, 15}, {g.B, 15}, {out_ptr(g), 0}});
    if (rc != QG_GO) return rc;
#ifndef QG_TILED_GEMVM  // (A/B builds: 0 = the round-6 tiled decode GEMV for every M <= 4)
#define QG_TILED_GEMVM 1
#endif
    if (QG_TILED_GEMVM && gemvm_eligible(g)) return hip_status(launch_gemvm(g, st));  // M = 3..4 (2 at long K)
    if (gemvt_eligible(g)) return hip_status(launch_gemvt(g, st));  // M <= 4: the tiled decode GEMV
    if (!mfma_eligible(g)) return QG_ERR_UNSUPPORTED;
    return hip_status(launch_mfma(g, st));
}

// The tiled entries (lay = LAY_TILED, LAY_TILED_ACT): the product with an output row stride, the sumi hook
// and the configuration query.
int tiled_product(int lay, const void* A, const void* B_tiled, float* C, int M, int N, int K, int64_t ldc, int wtype,
                  qg_stream_t stream) {
    if (ldc < N || (M > 1 && ldc <= 0)) return QG_ERR_INVALID_ARG;
    GemmArgs g = product_args(A, B_tiled, C, M, N, K, wtype);
    g.ldc_m = (long)ldc;
    g.lay = lay;
    return run_tiled(g, (hipStream_t)stream);
}

int tiled_sumi(int lay, const void* A, const void* B_tiled, int32_t* sumi, int M, int N, int K, int wtype,
               qg_stream_t stream) {
    GemmArgs g = product_args(A, B_tiled, nullptr, M, N, K, wtype);
    g.sumi = sumi;
    g.lay = lay;
    return run_tiled(g, (hipStream_t)stream);
}

// qg_debug_config*: the leaf launcher names the kernel into buf and launches nothing
int describe_product(int lay, int M, int N, int K, int wtype, int algo, int sumi, char* buf, size_t len) {
    if (!buf || len == 0) return QG_ERR_INVALID_ARG;
    buf[0] = 0;
    GemmArgs g = query_args(M, N, K, wtype, sumi);
    g.lay = lay;
    g.describe = buf; g.describe_len = len;
    return lay == LAY_ROWS ? run_product(g, algo, nullptr) : run_tiled(g, nullptr);
}

int weight_major(int wtype, const void* W, const void* A, float* out, int M, int N, int K, qg_stream_t s) {
    GemmArgs g = weight_major_args(wtype, W, A, out, M, N, K);
    return run_product(g, QG_ALGO_AUTO, (hipStream_t)s, false);
}

int run_w16(int wtype, const float* A, const void* B, float* C, int M, int N, int K, hipStream_t st,
            void* ws = nullptr, size_t ws_bytes = 0, char* describe = nullptr, size_t describe_len = 0) {
    const int rc = precheck({M, N}, K, 32, true, {{A, 3}, {B, 1}, {C, 0}});
    if (rc != QG_GO) return rc;
    GemmArgs g = product_args(A, B, C, M, N, K, wtype);
    g.ws = ws; g.ws_bytes = ws_bytes;
    g.describe = describe; g.describe_len = describe_len;
    return hip_status(launch_w16(g, st));
}

// Dims as extract_dims_from_tensor (include/llama_adapter.h:49-61): K = act->ne[0], M = act->ne[1],
// N = w->ne[1]; output [N, M] in ggml ne-order, i.e. row-major C[M][N]. Rows must be dense (the
// kernels' layout); batched views (ne[2..3] > 1) are out of scope. k_mult: K granularity.
size_t row_bytes(int type, int64_t K) {
    if (type == QG_TYPE_F32) return (size_t)K * 4;
    if (type == QG_TYPE_F16) return (size_t)K * 2;
    const int be = block_elems(type);  // 256 for the super-block types
    return be ? (size_t)(K / be) * (size_t)block_bytes(type) : 0;
}

int view_dims(const qg_tensor_view* act, const qg_tensor_view* w, const qg_tensor_view* out, int64_t& M, int64_t& N,
              int64_t& K, int k_mult = 32) {
    for (int d = 2; d < 4; ++d)
        if ((act->ne[d] != 1 && act->ne[d] != 0) || (w->ne[d] != 1 && w->ne[d] != 0) || (out->ne[d] != 1 && out->ne[d] != 0))
            return QG_ERR_UNSUPPORTED;
    K = act->ne[0];
    M = act->ne[1];
    N = w->ne[1];
    if (w->ne[0] != K || out->ne[0] != N || out->ne[1] != M) return QG_ERR_INVALID_ARG;
    if (K <= 0 || K % k_mult != 0) return QG_ERR_BAD_K;
    if (M > INT32_MAX || N > INT32_MAX || K > INT32_MAX) return QG_ERR_UNSUPPORTED;
    if ((M > 1 && act->nb[1] != row_bytes(act->type, K)) || (N > 1 && w->nb[1] != row_bytes(w->type, K)) ||
        out->nb[0] != sizeof(float) || (M > 1 && out->nb[1] != (size_t)N * sizeof(float)))
        return QG_ERR_UNSUPPORTED;
    return QG_OK;
}

// kernel_type of the FP32-activation _from_view entries: NULL or one of the reference's names (all one kernel here)
bool baseline_kernel_type(const char* kt) {
    return !kt || strcmp(kt, "naive") == 0 || strcmp(kt, "tiled") == 0 || strcmp(kt, "auto") == 0;
}

size_t fused_workspace_bytes(int M, int K) { return M > 0 && K > 0 ? (size_t)M * (size_t)(K / 32) * 36 : 0; }

// FP32 / FP16 activations (g.ain != AIN_Q8_1), dense rows of K elements. Small M: quantization
// fused into the GEMV prologue, one launch. Larger M: quantize into the caller's workspace, then
// the Q8_1 product (same bytes, so the same results); without a workspace, fused GEMV launches
// over row chunks (the weights are streamed once per chunk).
int run_fused(GemmArgs g, void* ws, size_t ws_bytes, hipStream_t st) {
    const bool ksb = is_routed_type(g.wtype);
    const size_t es = g.ain == AIN_F32 ? 4 : 2;
    const int rc = precheck({g.M, g.N}, g.K, ksb ? block_elems(g.wtype) : 32, ksb || is_weight_type(g.wtype),
                            {{g.A, ksb ? 3 : es - 1}, {g.B, ksb ? sb_weight_mask(g.wtype) : 1u}, {g.C, 0}});
    if (rc != QG_GO) return rc;
    const bool vec_ok = ((uintptr_t)g.A & 15) == 0;
    const bool ws_ok = ws && ws_bytes >= fused_workspace_bytes(g.M, g.K);
    // the super-block types and MXFP4 have no fused prologue: only FP32 rows through the caller's workspace, then the Q8_1 product on it
    if (ksb && (g.ain != AIN_F32 || !ws_ok)) return QG_ERR_UNSUPPORTED;
    if (!ksb && g.M <= 4 && vec_ok && gemv_eligible(g)) return hip_status(launch_gemv(g, st));
    if (ws_ok) {
        if (((uintptr_t)ws & 3) != 0) return QG_ERR_ALIGN;
        const int64_t nblocks = (int64_t)g.M * (g.K / 32);
        const hipError_t e = g.ain == AIN_F32 ? launch_quantize(QG_TYPE_Q8_1, 0, (const float*)g.A, ws, nblocks, st)
                                              : launch_quantize_f16_fused(g.A, ws, nblocks, st);
        if (e != hipSuccess) return hip_status(e);
        GemmArgs q = g;
        q.ain = AIN_Q8_1;
        q.A = ws;
        return run_product(q, QG_ALGO_AUTO, st);
    }
    if (!vec_ok) return QG_ERR_ALIGN;
    for (int rows : {8, 4, 2, 1}) {
        GemmArgs c = g;
        c.M = rows < g.M ? rows : g.M;
        if (!gemv_eligible(c)) continue;
        const long row_bytes = (long)g.K * (long)es;
        const int full = g.M / c.M, rem = g.M - full * c.M;
        if (full > 65535) return QG_ERR_UNSUPPORTED;
        c.batch = full;
        c.sA = (long)c.M * row_bytes;
        c.sB = 0;
        c.sC = (long)c.M * g.ldc_m;
        hipError_t e = launch_gemv(c, st);
        if (e != hipSuccess || rem == 0) return hip_status(e);
        c.batch = 1;
        c.A = (const uint8_t*)g.A + (long)full * c.sA;
        c.C = g.C + (long)full * c.sC;
        c.M = rem;
        return hip_status(launch_gemv(c, st));
    }
    return QG_ERR_UNSUPPORTED;
}

// ---- mul_mat_id: the three expert entries, the fused gate / up entry and the down entry with the expert sum -----
// A call of qg_gemm_w4a8_moe, _moe_prefill, _moe_batch, _moe_glu or _moe_down under the names of qg.h (ws: the entries
// with a plan; B_up, glu_op: _moe_glu, whose B is B_gate; weights, w_stride: _moe_down, whose C has a row per token), a
// qg_moe*_config query of one (describe: name the launch there and launch nothing), and what moe_front adds.
struct MoeCall {
    const void* A; int a_rows;
    const void* B; int n_expert;
    const int32_t* ids; int64_t ids_stride;
    float* C; int64_t ldc;  // after moe_front: the floats between slots, never 0
    int T, n_used, N, K, wtype;
    void* ws; size_t ws_bytes;
    hipStream_t st;
    char* describe; size_t describe_len;
    long estride;  // moe_front: bytes between experts
    int slots;     // moe_front: T * n_used
    const void* B_up; int glu_op;
    const float* weights; int64_t w_stride;
    // qg_gemm_w4a8_moe_glu_bias, _moe_down_bias, _moe_prefill_bias, _moe_batch_bias (biased; the one bias of the last three
    // is bias_gate). After moe_front: bias_stride never 0
    bool biased;
    const float* bias_gate; const float* bias_up; int64_t bias_stride;
    float alpha, limit;
};

// Bytes of a plan's workspace whose tile region is sized for tiles of min_r rows (qg_moe_plan.hpp).
size_t moe_ws_bytes(int64_t T, int64_t n_used, int64_t n_expert, int min_r) {
    if (T <= 0 || n_used <= 0 || n_expert <= 0) return 0;
    return (size_t)moe_plan_layout((long)(T * n_used), (long)n_expert, min_r).total * sizeof(int32_t);
}

// What the entries check alike, in the order qg.h documents. rows_ok: the entry takes the 32-element types
// (otherwise one of them is a type it does not take, checked at the 32-element granule as in run_product). min_r: 0,
// or the entry runs a plan in a workspace sized for tiles of min_r rows. up: the entry has a second weights pointer,
// B_up, checked beside B with the same mask. down: the entry is qg_gemm_w4a8_moe_down: weights stands beside the other
// pointers (null allowed, 4 B otherwise), w_stride beside ids_stride, and the grid's y is the token, so T is what 65535
// bounds (slots stays 0). c.biased: the entry is one of the four _bias ones: it takes MXFP4 beside the super-block types,
// its bias pointers stand beside the other pointers (null allowed, 4 B otherwise), bias_stride and the OAI op's alpha
// and limit beside ids_stride.
//   1. the precheck; 2. a_rows, ids_stride, n_expert, ldc: QG_ERR_INVALID_ARG;
//   3. the workspace: null QG_ERR_INVALID_ARG, off 16 B QG_ERR_ALIGN, too small QG_ERR_INVALID_ARG;
//   4. QG_ERR_UNSUPPORTED: more than 65535 slots (the grid's y, and the plan's bound), more than 4096 experts in a plan,
//      an expert stride off the kernel's weight alignment.
// QG_GO: ldc, estride and slots are set; go on with what only the entry refuses. ids is never read here.
int moe_front(MoeCall& c, bool rows_ok, int min_r, bool up = false, bool down = false) {
    // (MXFP4 is a type of qg_gemm_w4a8_moe and the four _bias entries: elsewhere it is refused as the 32-element types are)
    const bool ksb = is_sb_type(c.wtype) || ((rows_ok || c.biased) && is_mxfp4_type(c.wtype));
    const uintptr_t wmask = ksb ? sb_weight_mask(c.wtype) : 3u;
    const int rc = precheck({c.T, c.n_used, c.N}, c.K, ksb ? block_elems(c.wtype) : 32, ksb || (rows_ok && is_weight_type(c.wtype)),
                            {{c.A, 3}, {c.B, wmask}, {up ? c.B_up : c.B, wmask}, {c.ids, 3},
                             {down && c.weights ? c.weights : c.A, 3}, {c.C, 0},
                             {c.biased && c.bias_gate ? c.bias_gate : c.A, 3}, {c.biased && c.bias_up ? c.bias_up : c.A, 3}});
    if (rc != QG_GO) return rc;
    if ((c.a_rows != 1 && c.a_rows != c.n_used) || c.ids_stride < c.n_used || c.n_expert < 1 || c.ldc < 0 ||
        (c.ldc > 0 && c.ldc < c.N) || (down && c.weights && c.w_stride < c.n_used))
        return QG_ERR_INVALID_ARG;
    if (c.biased) {
        if (c.bias_stride < 0 || (c.bias_stride > 0 && c.bias_stride < c.N)) return QG_ERR_INVALID_ARG;
        if (c.glu_op == QG_GLU_SWIGLU_OAI && !(std::isfinite(c.alpha) && std::isfinite(c.limit) && c.limit > 0.0f))
            return QG_ERR_INVALID_ARG;
        if (!c.bias_stride) c.bias_stride = c.N;
    }
    if (min_r) {
        if (!c.ws) return QG_ERR_INVALID_ARG;
        if (((uintptr_t)c.ws & (MOE_WS_ALIGN - 1)) != 0) return QG_ERR_ALIGN;
        if (c.ws_bytes < moe_ws_bytes(c.T, c.n_used, c.n_expert, min_r)) return QG_ERR_INVALID_ARG;
    }
    const int64_t slots = (int64_t)c.T * c.n_used;
    if ((down ? c.T : slots) > MOE_MAX_SLOTS || (min_r && c.n_expert > MOE_MAX_EXPERTS)) return QG_ERR_UNSUPPORTED;
    c.slots = down ? 0 : (int)slots;
    if (!c.ldc) c.ldc = c.N;
    c.estride = (long)c.N * (long)(c.K / block_elems(c.wtype)) * block_bytes(c.wtype);
    return ((uintptr_t)c.estride & wmask) != 0 ? QG_ERR_UNSUPPORTED : QG_GO;
}

// the fields MoeArgs and MoePlanArgs have in common
template <class KernArgs> KernArgs moe_kernel_args(const MoeCall& c) {
    KernArgs a;
    a.A = c.A; a.B = c.B; a.ids = c.ids; a.C = c.C;
    a.ids_stride = (long)c.ids_stride; a.ldc = (long)c.ldc; a.estride = c.estride;
    a.a_rows = c.a_rows; a.n_used = c.n_used; a.n_expert = c.n_expert; a.N = c.N; a.K = c.K; a.slots = c.slots;
    return a;
}

// AUTO at M = 1 sends this (N, K, type) to the type's decode GEMV: the body the two decode entries run per slot
bool moe_gemv_route(const MoeCall& c) {
    const GemmArgs q = product_args(c.A, c.B, c.C, 1, c.N, c.K, c.wtype);
    return is_routed_type(c.wtype) ? select_algo_sb(q) == QG_ALGO_GEMV : select_algo(q) == QG_ALGO_GEMV && gemv_eligible(q);
}

// qg_gemm_w4a8_moe, qg_moe_config. Its own refusals: a shape off the decode GEMV, LDS records beyond 160 KiB.
int run_moe(MoeCall& c) {
    const int rc = moe_front(c, true, 0);
    if (rc != QG_GO) return rc;
    if (!moe_gemv_route(c) || !moe_lds_ok(c.wtype, c.K)) return QG_ERR_UNSUPPORTED;
    MoeArgs a = moe_kernel_args<MoeArgs>(c);
    a.arow = (long)(c.K / 32) * 36;
    return hip_status(launch_moe(a, c.wtype, c.st, c.describe, c.describe_len));
}

// qg_gemm_w4a8_moe_prefill, qg_moe_prefill_config and qg_debug_moe_prefill_plan (which stops after the plan): Q4_K / Q6_K.
int moe_prefill_args(MoeCall& c, MoePlanArgs& a) {
    const int rc = moe_front(c, false, MOE_PREFILL_MIN_R);
    if (rc != QG_GO) return rc;
    a = moe_kernel_args<MoePlanArgs>(c);
    a.ws = (int32_t*)c.ws;
    return QG_GO;
}

int run_moe_prefill(MoeCall& c) {
    MoePlanArgs a;
    const int rc = moe_prefill_args(c, a);
    if (rc != QG_GO) return rc;
    return hip_status(launch_moe_prefill(a, c.wtype, c.st, c.describe, c.describe_len));
}

// qg_gemm_w4a8_moe_batch, qg_moe_batch_config: Q4_K / Q6_K. Its own refusals: a shape off the decode GEMV, K whose
// records of two rows exceed the LDS (moe_batch_rows), a tile bound beyond 65535.
int run_moe_batch(MoeCall& c) {
    const int rc = moe_front(c, false, MOE_BATCH_MIN_R);
    if (rc != QG_GO) return rc;
    const int R = moe_batch_rows(c.slots, c.n_expert, c.K, c.wtype);
    if (!moe_gemv_route(c) || R == 0 || moe_max_tiles(c.slots, c.n_expert, R) > 65535) return QG_ERR_UNSUPPORTED;
    MoePlanArgs a = moe_kernel_args<MoePlanArgs>(c);
    a.ws = (int32_t*)c.ws;
    return hip_status(launch_moe_batch(a, c.wtype, c.st, c.describe, c.describe_len));
}

// qg_gemm_w4a8_moe_prefill_bias, qg_moe_prefill_bias_config: Q4_K / Q6_K / MXFP4 (c.biased; the one bias is bias_gate),
// run_moe_prefill's refusals.
MoeBiasArgs moe_bias_args(const MoeCall& c) {
    MoeBiasArgs a;
    static_cast<MoePlanArgs&>(a) = moe_kernel_args<MoePlanArgs>(c);
    a.ws = (int32_t*)c.ws;
    a.bias = c.bias_gate; a.bias_stride = (long)c.bias_stride;
    return a;
}

int run_moe_prefill_bias(MoeCall& c) {
    c.biased = true; c.bias_up = nullptr; c.glu_op = QG_GLU_REGLU;
    const int rc = moe_front(c, false, MOE_PREFILL_MIN_R);
    if (rc != QG_GO) return rc;
    return hip_status(launch_moe_prefill_bias(moe_bias_args(c), c.wtype, c.st, c.describe, c.describe_len));
}

// qg_gemm_w4a8_moe_batch_bias, qg_moe_batch_bias_config: Q4_K / Q6_K / MXFP4 (c.biased), run_moe_batch's refusals.
int run_moe_batch_bias(MoeCall& c) {
    c.biased = true; c.bias_up = nullptr; c.glu_op = QG_GLU_REGLU;
    const int rc = moe_front(c, false, MOE_BATCH_MIN_R);
    if (rc != QG_GO) return rc;
    const int R = moe_batch_rows(c.slots, c.n_expert, c.K, c.wtype);
    if (!moe_gemv_route(c) || R == 0 || moe_max_tiles(c.slots, c.n_expert, R) > 65535) return QG_ERR_UNSUPPORTED;
    return hip_status(launch_moe_batch_bias(moe_bias_args(c), c.wtype, c.st, c.describe, c.describe_len));
}

// qg_gemm_w4a8_moe_glu, qg_moe_glu_config: Q4_K / Q6_K. Its own refusals: a glu_op it does not have, a shape off the
// decode GEMV (the bound on the LDS records is part of that route for the super-block types).
int run_moe_glu(MoeCall& c) {
    const int rc = moe_front(c, false, 0, true);
    if (rc != QG_GO) return rc;
    if ((c.glu_op != QG_GLU_REGLU && c.glu_op != QG_GLU_SWIGLU) || !moe_gemv_route(c)) return QG_ERR_UNSUPPORTED;
    MoeGluArgs a;
    a.A = c.A; a.B_gate = c.B; a.B_up = c.B_up; a.ids = c.ids; a.C = c.C;
    a.ids_stride = (long)c.ids_stride; a.ldc = (long)c.ldc; a.estride = c.estride; a.arow = (long)(c.K / 32) * 36;
    a.n_used = c.n_used; a.n_expert = c.n_expert; a.N = c.N; a.K = c.K; a.slots = c.slots; a.glu_op = c.glu_op;
    return hip_status(launch_moe_glu(a, c.wtype, c.st, c.describe, c.describe_len));
}

// qg_gemm_w4a8_moe_down, qg_moe_down_config: Q4_K / Q6_K, a_rows = n_used. Its own refusals: a shape off the decode
// GEMV, the records of the token's n_used activation rows and its n_used x RPB products beyond the LDS.
int run_moe_down(MoeCall& c) {
    c.a_rows = c.n_used;
    const int rc = moe_front(c, false, 0, false, true);
    if (rc != QG_GO) return rc;
    if (!moe_gemv_route(c) || moe_down_form(c.n_used, c.K, c.wtype).lds > MAX_LDS_BYTES) return QG_ERR_UNSUPPORTED;
    MoeDownArgs a;
    a.A = c.A; a.B = c.B; a.ids = c.ids; a.weights = c.weights; a.C = c.C;
    a.ids_stride = (long)c.ids_stride; a.w_stride = (long)c.w_stride; a.ldc = (long)c.ldc; a.estride = c.estride;
    a.arow = (long)(c.K / 32) * 36;
    a.n_used = c.n_used; a.n_expert = c.n_expert; a.N = c.N; a.K = c.K; a.T = c.T;
    return hip_status(launch_moe_down(a, c.wtype, c.st, c.describe, c.describe_len));
}

// qg_gemm_w4a8_moe_glu_bias, qg_moe_glu_bias_config: Q4_K / Q6_K / MXFP4 (c.biased). run_moe_glu's refusals with the
// third op among the known ones.
int run_moe_glu_bias(MoeCall& c) {
    c.biased = true;
    const int rc = moe_front(c, false, 0, true);
    if (rc != QG_GO) return rc;
    if ((c.glu_op != QG_GLU_REGLU && c.glu_op != QG_GLU_SWIGLU && c.glu_op != QG_GLU_SWIGLU_OAI) || !moe_gemv_route(c))
        return QG_ERR_UNSUPPORTED;
    MoeGluBiasArgs a;
    a.A = c.A; a.B_gate = c.B; a.B_up = c.B_up; a.ids = c.ids; a.C = c.C;
    a.ids_stride = (long)c.ids_stride; a.ldc = (long)c.ldc; a.estride = c.estride; a.arow = (long)(c.K / 32) * 36;
    a.n_used = c.n_used; a.n_expert = c.n_expert; a.N = c.N; a.K = c.K; a.slots = c.slots; a.glu_op = c.glu_op;
    a.bias_gate = c.bias_gate; a.bias_up = c.bias_up; a.bias_stride = (long)c.bias_stride; a.alpha = c.alpha; a.limit = c.limit;
    return hip_status(launch_moe_glu_bias(a, c.wtype, c.st, c.describe, c.describe_len));
}

// qg_gemm_w4a8_moe_down_bias, qg_moe_down_bias_config: Q4_K / Q6_K / MXFP4 (c.biased), run_moe_down's refusals.
int run_moe_down_bias(MoeCall& c) {
    c.a_rows = c.n_used;
    c.biased = true; c.bias_up = nullptr; c.glu_op = QG_GLU_REGLU;
    const int rc = moe_front(c, false, 0, false, true);
    if (rc != QG_GO) return rc;
    if (!moe_gemv_route(c) || moe_down_form(c.n_used, c.K, c.wtype).lds > MAX_LDS_BYTES) return QG_ERR_UNSUPPORTED;
    MoeDownBiasArgs a;
    a.A = c.A; a.B = c.B; a.ids = c.ids; a.weights = c.weights; a.C = c.C;
    a.ids_stride = (long)c.ids_stride; a.w_stride = (long)c.w_stride; a.ldc = (long)c.ldc; a.estride = c.estride;
    a.arow = (long)(c.K / 32) * 36;
    a.n_used = c.n_used; a.n_expert = c.n_expert; a.N = c.N; a.K = c.K; a.T = c.T;
    a.bias = c.bias_gate; a.bias_stride = (long)c.bias_stride;
    return hip_status(launch_moe_down_bias(a, c.wtype, c.st, c.describe, c.describe_len));
}

// A bias view of the two _bias view entries -> pointer and stride: F32, ne = [N, n_expert], nb[0] = 4, nb[1] a
// multiple of 4 and >= 4 N. Null: no bias. stride: 0 until a view has set it; two views must agree.
int bias_view(const qg_tensor_view* v, const MoeCall& c, const float*& p, int64_t& stride) {
    p = nullptr;
    if (!v) return QG_GO;
    auto one = [](int64_t x) { return x == 1 || x == 0; };
    if (v->type != QG_TYPE_F32) return QG_ERR_UNSUPPORTED;
    if (v->ne[0] != c.N || v->ne[1] != c.n_expert) return QG_ERR_INVALID_ARG;
    if (!one(v->ne[2]) || !one(v->ne[3]) || v->nb[0] != sizeof(float) || v->nb[1] % sizeof(float) != 0 ||
        v->nb[1] < (size_t)c.N * sizeof(float))
        return QG_ERR_UNSUPPORTED;
    const int64_t st = (int64_t)(v->nb[1] / sizeof(float));
    if (stride && stride != st) return QG_ERR_UNSUPPORTED;
    if (!v->data) return QG_ERR_INVALID_ARG;
    p = (const float*)v->data;
    stride = st;
    return QG_GO;
}

// qg_moe*_config: the shape alone, as qg_debug_config: 256-B aligned stand-in pointers (a workspace of any size among
// them), one activation row per token.
int moe_config(int (*run)(MoeCall&), int T, int n_used, int n_expert, int N, int K, int wtype, char* buf, size_t len) {
    if (!buf || len == 0) return QG_ERR_INVALID_ARG;
    buf[0] = 0;
    MoeCall c{(const void*)256, 1, (const void*)256, n_expert, (const int32_t*)256, n_used, (float*)256, 0, T, n_used, N, K,
              wtype, (void*)256, SIZE_MAX, nullptr, buf, len};
    c.B_up = c.B;
    return run(c);
}

// The views of ggml_mul_mat_id -> the operands and sizes of an expert entry's call (qg.h, qg_mul_mat_id_from_view).
int mul_mat_id_view(const qg_tensor_view* as, const qg_tensor_view* b, const qg_tensor_view* ids, const qg_tensor_view* out,
                    MoeCall& c) {
    if (!as || !b || !ids || !out) return QG_ERR_INVALID_ARG;
    if (b->type != QG_TYPE_Q8_1 || ids->type != QG_TYPE_I32 || out->type != QG_TYPE_F32 ||
        !(is_weight_type(as->type) || is_routed_type(as->type)))
        return QG_ERR_UNSUPPORTED;
    auto one = [](int64_t v) { return v == 1 || v == 0; };
    if (!one(as->ne[3]) || !one(b->ne[3]) || !one(ids->ne[2]) || !one(ids->ne[3]) || !one(out->ne[3])) return QG_ERR_UNSUPPORTED;
    const int64_t K = as->ne[0], N = as->ne[1], n_expert = as->ne[2], a_rows = b->ne[1], T = b->ne[2], n_used = ids->ne[0];
    if (b->ne[0] != K || ids->ne[1] != T || out->ne[0] != N || out->ne[1] != n_used || out->ne[2] != T)
        return QG_ERR_INVALID_ARG;
    if (K <= 0 || K % block_elems(as->type) != 0) return QG_ERR_BAD_K;
    if (T > INT32_MAX || n_used > INT32_MAX || N > INT32_MAX || K > INT32_MAX || n_expert > INT32_MAX || a_rows > INT32_MAX)
        return QG_ERR_UNSUPPORTED;
    // dense weight rows and experts, dense activation rows and tokens, ids rows a whole number of int32 apart, output
    // rows a whole number of floats apart with the token's slots one after another
    const size_t wrow = row_bytes(as->type, K), arow = row_bytes(QG_TYPE_Q8_1, K);
    if ((N > 1 && as->nb[1] != wrow) || (n_expert > 1 && as->nb[2] != (size_t)N * wrow) ||
        (a_rows > 1 && b->nb[1] != arow) || (T > 1 && b->nb[2] != (size_t)a_rows * arow) ||
        (n_used > 1 && ids->nb[0] != sizeof(int32_t)) || (T > 1 && ids->nb[1] % sizeof(int32_t) != 0) ||
        out->nb[0] != sizeof(float) || (n_used > 1 && T > 1 && out->nb[2] != (size_t)n_used * out->nb[1]))
        return QG_ERR_UNSUPPORTED;
    const size_t slot_bytes = n_used > 1 ? out->nb[1] : T > 1 ? out->nb[2] : (size_t)N * sizeof(float);
    if (slot_bytes % sizeof(float) != 0) return QG_ERR_UNSUPPORTED;
    c = {b->data, (int)a_rows, as->data, (int)n_expert, (const int32_t*)ids->data,
         T > 1 ? (int64_t)(ids->nb[1] / sizeof(int32_t)) : n_used, (float*)out->data, (int64_t)(slot_bytes / sizeof(float)),
         (int)T, (int)n_used, (int)N, (int)K, as->type};
    return QG_GO;
}

// qg_mul_mat_id_from_view*: the views, then the entry
int mul_mat_id_from_view(int (*run)(MoeCall&), const qg_tensor_view* as, const qg_tensor_view* b, const qg_tensor_view* ids,
                         const qg_tensor_view* out, void* ws, size_t ws_bytes, qg_stream_t stream) {
    MoeCall c;
    const int rc = mul_mat_id_view(as, b, ids, out, c);
    if (rc != QG_GO) return rc;
    c.ws = ws; c.ws_bytes = ws_bytes; c.st = (hipStream_t)stream;
    return run(c);
}
// The views of qg_mul_mat_id_down_from_view -> the call of the down entry (stream apart).
int mul_mat_id_down_view(const qg_tensor_view* as, const qg_tensor_view* b, const qg_tensor_view* ids,
                         const qg_tensor_view* weights, const qg_tensor_view* out, MoeCall& c) {
    if (!out) return QG_ERR_INVALID_ARG;
    // as, b and ids go through the checks of qg_mul_mat_id_from_view beside a dense stand-in [N, n_used, T] for its
    // output (this entry's has a row per token): every refusal of that entry's, then what is this entry's own
    const int64_t n_used = ids ? ids->ne[0] : 0;
    auto one = [](int64_t v) { return v == 1 || v == 0; };
    if (!one(out->ne[2])) return QG_ERR_UNSUPPORTED;
    qg_tensor_view slots = *out;
    slots.ne[1] = n_used; slots.ne[2] = out->ne[1];
    slots.nb[1] = (size_t)(out->ne[0] > 0 ? out->ne[0] : 0) * sizeof(float); slots.nb[2] = (size_t)n_used * slots.nb[1];
    const int rc = mul_mat_id_view(as, b, ids, &slots, c);
    if (rc != QG_GO) return rc;
    if (c.a_rows != c.n_used) return QG_ERR_UNSUPPORTED;
    if (c.T > 1 && out->nb[1] % sizeof(float) != 0) return QG_ERR_UNSUPPORTED;
    c.ldc = c.T > 1 ? (int64_t)(out->nb[1] / sizeof(float)) : c.N;
    c.weights = nullptr; c.w_stride = c.n_used;
    if (weights) {
        // F32 [n_used, T] or [1, n_used, T]: the router's weights as ggml keeps them
        const int d = weights->ne[0] == 1 && weights->ne[1] == c.n_used && weights->ne[2] == c.T ? 1 : 0;
        if (weights->type != QG_TYPE_F32) return QG_ERR_UNSUPPORTED;
        if (weights->ne[d] != c.n_used || weights->ne[d + 1] != c.T) return QG_ERR_INVALID_ARG;
        if (!one(weights->ne[d + 2]) || (d == 0 && !one(weights->ne[3]))) return QG_ERR_UNSUPPORTED;
        if ((c.n_used > 1 && weights->nb[d] != sizeof(float)) || (c.T > 1 && weights->nb[d + 1] % sizeof(float) != 0))
            return QG_ERR_UNSUPPORTED;
        c.weights = (const float*)weights->data;
        if (!c.weights) return QG_ERR_INVALID_ARG;
        if (c.T > 1) c.w_stride = (int64_t)(weights->nb[d + 1] / sizeof(float));
    }
    c.ws = nullptr; c.ws_bytes = 0;
    return QG_GO;
}
}  // namespace

extern "C" {

int qg_gemm_w4a8_moe(const void* A_q8_1, int a_rows, const void* B_experts, int n_expert, const int32_t* ids,
                     int64_t ids_stride, float* C, int64_t ldc, int T, int n_used, int N, int K, int wtype,
                     qg_stream_t stream) {
    MoeCall c{A_q8_1, a_rows, B_experts, n_expert, ids, ids_stride, C, ldc, T, n_used, N, K, wtype, nullptr, 0,
              (hipStream_t)stream};
    return run_moe(c);
}

int qg_moe_config(int T, int n_used, int N, int K, int wtype, char* buf, size_t len) {
    return moe_config(run_moe, T, n_used, 1, N, K, wtype, buf, len);
}

int qg_mul_mat_id_from_view(const qg_tensor_view* as, const qg_tensor_view* b, const qg_tensor_view* ids,
                            qg_tensor_view* out, qg_stream_t stream) {
    return mul_mat_id_from_view(run_moe, as, b, ids, out, nullptr, 0, stream);
}

size_t qg_gemm_w4a8_moe_prefill_workspace_size(int T, int n_used, int n_expert) {
    return moe_ws_bytes(T, n_used, n_expert, MOE_PREFILL_MIN_R);
}

int qg_gemm_w4a8_moe_prefill(const void* A_q8_1, int a_rows, const void* B_experts, int n_expert, const int32_t* ids,
                             int64_t ids_stride, float* C, int64_t ldc, int T, int n_used, int N, int K, int wtype,
                             void* workspace, size_t workspace_bytes, qg_stream_t stream) {
    MoeCall c{A_q8_1, a_rows, B_experts, n_expert, ids, ids_stride, C, ldc, T, n_used, N, K, wtype, workspace,
              workspace_bytes, (hipStream_t)stream};
    return run_moe_prefill(c);
}

int qg_moe_prefill_config(int T, int n_used, int n_expert, int N, int K, int wtype, char* buf, size_t len) {
    return moe_config(run_moe_prefill, T, n_used, n_expert, N, K, wtype, buf, len);
}

int qg_debug_moe_prefill_plan(const int32_t* ids, int64_t ids_stride, int T, int n_used, int n_expert, int a_rows, int N,
                              int K, int wtype, int32_t* counts, int32_t* sorted, void* workspace, size_t workspace_bytes,
                              qg_stream_t stream) {
    if (T > 0 && n_used > 0 && N > 0 && (!counts || !sorted)) return QG_ERR_INVALID_ARG;
    // A, B and C are stand-ins: the plan reads none of them
    MoeCall c{(const void*)256, a_rows, (const void*)256, n_expert, ids, ids_stride, (float*)256, 0, T, n_used, N, K, wtype,
              workspace, workspace_bytes, (hipStream_t)stream};
    MoePlanArgs a;
    const int rc = moe_prefill_args(c, a);
    if (rc != QG_GO) return rc;
    hipError_t e = launch_moe_plan(a, moe_prefill_tt(a, wtype), c.st);
    const MoePlanLayout L = moe_plan_layout(a.slots, n_expert);
    if (e == hipSuccess)
        e = hipMemcpyAsync(counts, a.ws + L.counts, sizeof(int32_t) * ((size_t)n_expert + 1), hipMemcpyDeviceToDevice, c.st);
    if (e == hipSuccess)
        e = hipMemcpyAsync(sorted, a.ws + L.sorted, sizeof(int32_t) * (size_t)a.slots, hipMemcpyDeviceToDevice, c.st);
    return hip_status(e);
}

int qg_mul_mat_id_from_view_ws(const qg_tensor_view* as, const qg_tensor_view* b, const qg_tensor_view* ids,
                               qg_tensor_view* out, void* workspace, size_t workspace_bytes, qg_stream_t stream) {
    return mul_mat_id_from_view(run_moe_prefill, as, b, ids, out, workspace, workspace_bytes, stream);
}

size_t qg_gemm_w4a8_moe_batch_workspace_size(int T, int n_used, int n_expert) {
    return moe_ws_bytes(T, n_used, n_expert, MOE_BATCH_MIN_R);
}

int qg_gemm_w4a8_moe_batch(const void* A_q8_1, int a_rows, const void* B_experts, int n_expert, const int32_t* ids,
                           int64_t ids_stride, float* C, int64_t ldc, int T, int n_used, int N, int K, int wtype,
                           void* workspace, size_t workspace_bytes, qg_stream_t stream) {
    MoeCall c{A_q8_1, a_rows, B_experts, n_expert, ids, ids_stride, C, ldc, T, n_used, N, K, wtype, workspace,
              workspace_bytes, (hipStream_t)stream};
    return run_moe_batch(c);
}

int qg_moe_batch_config(int T, int n_used, int n_expert, int N, int K, int wtype, char* buf, size_t len) {
    return moe_config(run_moe_batch, T, n_used, n_expert, N, K, wtype, buf, len);
}

int qg_mul_mat_id_from_view_batch(const qg_tensor_view* as, const qg_tensor_view* b, const qg_tensor_view* ids,
                                  qg_tensor_view* out, void* workspace, size_t workspace_bytes, qg_stream_t stream) {
    return mul_mat_id_from_view(run_moe_batch, as, b, ids, out, workspace, workspace_bytes, stream);
}

int qg_gemm_w4a8_moe_glu(const void* A_q8_1, const void* B_gate, const void* B_up, int n_expert, const int32_t* ids,
                         int64_t ids_stride, float* C, int64_t ldc, int T, int n_used, int N, int K, int wtype, int glu_op,
                         qg_stream_t stream) {
    MoeCall c{A_q8_1, 1, B_gate, n_expert, ids, ids_stride, C, ldc, T, n_used, N, K, wtype, nullptr, 0, (hipStream_t)stream};
    c.B_up = B_up; c.glu_op = glu_op;
    return run_moe_glu(c);
}

int qg_moe_glu_config(int T, int n_used, int N, int K, int wtype, char* buf, size_t len) {
    return moe_config(run_moe_glu, T, n_used, 1, N, K, wtype, buf, len);
}

int qg_mul_mat_id_glu_from_view(const qg_tensor_view* as_gate, const qg_tensor_view* as_up, const qg_tensor_view* b,
                                const qg_tensor_view* ids, qg_tensor_view* out, int glu_op, qg_stream_t stream) {
    if (!as_up) return QG_ERR_INVALID_ARG;
    MoeCall c;
    const int rc = mul_mat_id_view(as_gate, b, ids, out, c);
    if (rc != QG_GO) return rc;
    if (c.a_rows != 1 || as_up->type != as_gate->type || memcmp(as_up->ne, as_gate->ne, sizeof as_up->ne) != 0 ||
        memcmp(as_up->nb, as_gate->nb, sizeof as_up->nb) != 0)
        return QG_ERR_UNSUPPORTED;
    c.ws = nullptr; c.ws_bytes = 0; c.st = (hipStream_t)stream;
    c.B_up = as_up->data; c.glu_op = glu_op;
    return run_moe_glu(c);
}

int qg_gemm_w4a8_moe_down(const void* A_q8_1, const void* B_experts, int n_expert, const int32_t* ids, int64_t ids_stride,
                          const float* weights, int64_t w_stride, float* C, int64_t ldc, int T, int n_used, int N, int K,
                          int wtype, qg_stream_t stream) {
    MoeCall c{A_q8_1, n_used, B_experts, n_expert, ids, ids_stride, C, ldc, T, n_used, N, K, wtype, nullptr, 0,
              (hipStream_t)stream};
    c.weights = weights; c.w_stride = w_stride;
    return run_moe_down(c);
}

int qg_moe_down_config(int T, int n_used, int N, int K, int wtype, char* buf, size_t len) {
    return moe_config(run_moe_down, T, n_used, 1, N, K, wtype, buf, len);
}

int qg_mul_mat_id_down_from_view(const qg_tensor_view* as, const qg_tensor_view* b, const qg_tensor_view* ids,
                                 const qg_tensor_view* weights, qg_tensor_view* out, qg_stream_t stream) {
    MoeCall c;
    const int rc = mul_mat_id_down_view(as, b, ids, weights, out, c);
    if (rc != QG_GO) return rc;
    c.st = (hipStream_t)stream;
    return run_moe_down(c);
}


int qg_gemm_w4a8_moe_glu_bias(const void* A_q8_1, const void* B_gate, const void* B_up, const float* bias_gate,
                              const float* bias_up, int64_t bias_stride, int n_expert, const int32_t* ids, int64_t ids_stride,
                              float* C, int64_t ldc, int T, int n_used, int N, int K, int wtype, int glu_op, float alpha,
                              float limit, qg_stream_t stream) {
    MoeCall c{A_q8_1, 1, B_gate, n_expert, ids, ids_stride, C, ldc, T, n_used, N, K, wtype, nullptr, 0, (hipStream_t)stream};
    c.B_up = B_up; c.glu_op = glu_op;
    c.bias_gate = bias_gate; c.bias_up = bias_up; c.bias_stride = bias_stride; c.alpha = alpha; c.limit = limit;
    return run_moe_glu_bias(c);
}

int qg_moe_glu_bias_config(int T, int n_used, int N, int K, int wtype, char* buf, size_t len) {
    return moe_config(run_moe_glu_bias, T, n_used, 1, N, K, wtype, buf, len);
}

int qg_mul_mat_id_glu_bias_from_view(const qg_tensor_view* as_gate, const qg_tensor_view* as_up, const qg_tensor_view* bias_gate,
                                     const qg_tensor_view* bias_up, const qg_tensor_view* b, const qg_tensor_view* ids,
                                     qg_tensor_view* out, int glu_op, float alpha, float limit, qg_stream_t stream) {
    if (!as_up) return QG_ERR_INVALID_ARG;
    MoeCall c;
    int rc = mul_mat_id_view(as_gate, b, ids, out, c);
    if (rc != QG_GO) return rc;
    if (c.a_rows != 1 || as_up->type != as_gate->type || memcmp(as_up->ne, as_gate->ne, sizeof as_up->ne) != 0 ||
        memcmp(as_up->nb, as_gate->nb, sizeof as_up->nb) != 0)
        return QG_ERR_UNSUPPORTED;
    if ((rc = bias_view(bias_gate, c, c.bias_gate, c.bias_stride)) != QG_GO) return rc;
    if ((rc = bias_view(bias_up, c, c.bias_up, c.bias_stride)) != QG_GO) return rc;
    c.ws = nullptr; c.ws_bytes = 0; c.st = (hipStream_t)stream;
    c.B_up = as_up->data; c.glu_op = glu_op; c.alpha = alpha; c.limit = limit;
    return run_moe_glu_bias(c);
}

int qg_gemm_w4a8_moe_down_bias(const void* A_q8_1, const void* B_experts, const float* bias, int64_t bias_stride, int n_expert,
                               const int32_t* ids, int64_t ids_stride, const float* weights, int64_t w_stride, float* C,
                               int64_t ldc, int T, int n_used, int N, int K, int wtype, qg_stream_t stream) {
    MoeCall c{A_q8_1, n_used, B_experts, n_expert, ids, ids_stride, C, ldc, T, n_used, N, K, wtype, nullptr, 0,
              (hipStream_t)stream};
    c.weights = weights; c.w_stride = w_stride;
    c.bias_gate = bias; c.bias_stride = bias_stride;
    return run_moe_down_bias(c);
}

int qg_moe_down_bias_config(int T, int n_used, int N, int K, int wtype, char* buf, size_t len) {
    return moe_config(run_moe_down_bias, T, n_used, 1, N, K, wtype, buf, len);
}

int qg_mul_mat_id_down_bias_from_view(const qg_tensor_view* as, const qg_tensor_view* bias, const qg_tensor_view* b,
                                      const qg_tensor_view* ids, const qg_tensor_view* weights, qg_tensor_view* out,
                                      qg_stream_t stream) {
    MoeCall c;
    int rc = mul_mat_id_down_view(as, b, ids, weights, out, c);
    if (rc != QG_GO) return rc;
    if ((rc = bias_view(bias, c, c.bias_gate, c.bias_stride)) != QG_GO) return rc;
    c.st = (hipStream_t)stream;
    return run_moe_down_bias(c);
}

int qg_gemm_w4a8_moe_prefill_bias(const void* A_q8_1, int a_rows, const void* B_experts, const float* bias, int64_t bias_stride,
                                  int n_expert, const int32_t* ids, int64_t ids_stride, float* C, int64_t ldc, int T, int n_used,
                                  int N, int K, int wtype, void* workspace, size_t workspace_bytes, qg_stream_t stream) {
    MoeCall c{A_q8_1, a_rows, B_experts, n_expert, ids, ids_stride, C, ldc, T, n_used, N, K, wtype, workspace,
              workspace_bytes, (hipStream_t)stream};
    c.bias_gate = bias; c.bias_stride = bias_stride;
    return run_moe_prefill_bias(c);
}

int qg_moe_prefill_bias_config(int T, int n_used, int n_expert, int N, int K, int wtype, char* buf, size_t len) {
    return moe_config(run_moe_prefill_bias, T, n_used, n_expert, N, K, wtype, buf, len);
}

int qg_gemm_w4a8_moe_batch_bias(const void* A_q8_1, int a_rows, const void* B_experts, const float* bias, int64_t bias_stride,
                                int n_expert, const int32_t* ids, int64_t ids_stride, float* C, int64_t ldc, int T, int n_used,
                                int N, int K, int wtype, void* workspace, size_t workspace_bytes, qg_stream_t stream) {
    MoeCall c{A_q8_1, a_rows, B_experts, n_expert, ids, ids_stride, C, ldc, T, n_used, N, K, wtype, workspace,
              workspace_bytes, (hipStream_t)stream};
    c.bias_gate = bias; c.bias_stride = bias_stride;
    return run_moe_batch_bias(c);
}

int qg_moe_batch_bias_config(int T, int n_used, int n_expert, int N, int K, int wtype, char* buf, size_t len) {
    return moe_config(run_moe_batch_bias, T, n_used, n_expert, N, K, wtype, buf, len);
}

// qg_mul_mat_id_bias_from_view_ws / _batch: the views of qg_mul_mat_id_from_view_ws, then the bias view, then the entry
static int mul_mat_id_bias_from_view(int (*run)(MoeCall&), const qg_tensor_view* as, const qg_tensor_view* bias,
                                     const qg_tensor_view* b, const qg_tensor_view* ids, const qg_tensor_view* out, void* ws,
                                     size_t ws_bytes, qg_stream_t stream) {
    MoeCall c;
    int rc = mul_mat_id_view(as, b, ids, out, c);
    if (rc != QG_GO) return rc;
    if ((rc = bias_view(bias, c, c.bias_gate, c.bias_stride)) != QG_GO) return rc;
    c.ws = ws; c.ws_bytes = ws_bytes; c.st = (hipStream_t)stream;
    return run(c);
}

int qg_mul_mat_id_bias_from_view_ws(const qg_tensor_view* as, const qg_tensor_view* bias, const qg_tensor_view* b,
                                    const qg_tensor_view* ids, qg_tensor_view* out, void* workspace, size_t workspace_bytes,
                                    qg_stream_t stream) {
    return mul_mat_id_bias_from_view(run_moe_prefill_bias, as, bias, b, ids, out, workspace, workspace_bytes, stream);
}

int qg_mul_mat_id_bias_from_view_batch(const qg_tensor_view* as, const qg_tensor_view* bias, const qg_tensor_view* b,
                                       const qg_tensor_view* ids, qg_tensor_view* out, void* workspace, size_t workspace_bytes,
                                       qg_stream_t stream) {
    return mul_mat_id_bias_from_view(run_moe_batch_bias, as, bias, b, ids, out, workspace, workspace_bytes, stream);
}

void qg_release_workspaces(void) { release_workspaces(); }

size_t qg_gemm_w4a8_f32_workspace_size(int M, int K) { return fused_workspace_bytes(M, K); }

int qg_gemm_w4a16(const float* A, const void* B_q4_0, float* C, int M, int N, int K, qg_stream_t stream) {
    return run_w16(QG_TYPE_Q4_0, A, B_q4_0, C, M, N, K, (hipStream_t)stream);
}

int qg_gemm_w8a16(const float* A, const void* B_q8_0, float* C, int M, int N, int K, qg_stream_t stream) {
    return run_w16(QG_TYPE_Q8_0, A, B_q8_0, C, M, N, K, (hipStream_t)stream);
}

size_t qg_gemm_w16_workspace_size(int M, int N, int K) { return M > 0 && N > 0 ? w16_workspace_bytes(M, N, K) : 0; }

int qg_gemm_w4a16_ws(const float* A, const void* B_q4_0, float* C, int M, int N, int K, void* workspace,
                     size_t workspace_bytes, qg_stream_t stream) {
    return run_w16(QG_TYPE_Q4_0, A, B_q4_0, C, M, N, K, (hipStream_t)stream, workspace, workspace_bytes);
}

int qg_gemm_w8a16_ws(const float* A, const void* B_q8_0, float* C, int M, int N, int K, void* workspace,
                     size_t workspace_bytes, qg_stream_t stream) {
    return run_w16(QG_TYPE_Q8_0, A, B_q8_0, C, M, N, K, (hipStream_t)stream, workspace, workspace_bytes);
}

// The operands are stand-ins nothing dereferences: the offsets reach the alignment rules of the dispatch
int qg_w16_config(int M, int N, int K, int wtype, int a_off, int b_off, size_t ws_bytes, char* buf, size_t len) {
    if (!buf || len == 0) return QG_ERR_INVALID_ARG;
    buf[0] = 0;
    return run_w16(wtype, (const float*)(uintptr_t)(256 + (intptr_t)a_off), (const void*)(uintptr_t)(256 + (intptr_t)b_off),
                   (float*)256, M, N, K, nullptr, ws_bytes ? (void*)256 : nullptr, ws_bytes, buf, len);
}

int qg_gemm_q4_0_fp32(const void* weight_q4_0, const float* activation, float* out, int M, int N, int K,
                      qg_stream_t stream) {
    return run_w16(QG_TYPE_Q4_0, activation, weight_q4_0, out, M, N, K, (hipStream_t)stream);
}

int qg_gemm_w4a8_f32(const float* X, const void* B, float* C, int M, int N, int K, int wtype, void* workspace,
                     size_t workspace_bytes, qg_stream_t stream) {
    GemmArgs g = product_args(X, B, C, M, N, K, wtype);
    g.ain = AIN_F32;
    return run_fused(g, workspace, workspace_bytes, (hipStream_t)stream);
}

int qg_gemm_q4_0_fp16_fused_ws(const void* W, const void* act_f16, float* out, int M, int N, int K, void* workspace,
                               size_t workspace_bytes, qg_stream_t stream) {
    GemmArgs g = weight_major_args(QG_TYPE_Q4_0, W, act_f16, out, M, N, K);
    g.ain = AIN_F16_FUSED;
    return run_fused(g, workspace, workspace_bytes, (hipStream_t)stream);
}

int qg_gemm_q4_0_fp16_fused(const void* W, const void* act_f16, float* out, int M, int N, int K, qg_stream_t stream) {
    return qg_gemm_q4_0_fp16_fused_ws(W, act_f16, out, M, N, K, nullptr, 0, stream);
}

int qg_quantize_q8_1_f16_fused(const void* x, void* y, int64_t k, qg_stream_t stream) {
    const int rc = precheck_count(k, 32, true, {{x, 1}, {y, 3}});
    if (rc != QG_GO) return rc;
    return hip_status(launch_quantize_f16_fused(x, y, k / 32, (hipStream_t)stream));
}

int qg_gemm_w4a8_ex(const void* A, const void* B, float* C, int M, int N, int K, int wtype, int algo,
                    qg_stream_t stream) {
    GemmArgs g = product_args(A, B, C, M, N, K, wtype);
    return run_product(g, algo, (hipStream_t)stream);
}

int qg_gemm_w4a8_strided_batched(const void* A, int64_t strideA, const void* B, int64_t strideB, float* C,
                                 int64_t strideC, int batch, int M, int N, int K, int wtype, qg_stream_t stream) {
    GemmArgs g = product_args(A, B, C, M, N, K, wtype);
    g.batch = batch; g.sA = strideA; g.sB = strideB; g.sC = strideC;
    return run_product(g, QG_ALGO_AUTO, (hipStream_t)stream, false);
}

size_t qg_gemm_w4a8_workspace_size(int M, int N, int K, int wtype) {
    if (M <= 0 || N <= 0 || K <= 0 || K % 32 != 0 || !is_weight_type(wtype)) return 0;
    const GemmArgs g = query_args(M, N, K, wtype);
    return repack_eligible(g) ? repack_workspace_bytes(g) : 0;
}

int qg_gemm_w4a8_ws(const void* A, const void* B, float* C, int M, int N, int K, int wtype, void* workspace,
                    size_t workspace_bytes, qg_stream_t stream) {
    GemmArgs g = product_args(A, B, C, M, N, K, wtype);
    g.ws = workspace; g.ws_bytes = workspace_bytes;
    return run_product(g, QG_ALGO_AUTO, (hipStream_t)stream, false);
}

size_t qg_repack_weights_bytes(int N, int K, int wtype) {
    if (N < 0 || K <= 0 || K % 32 != 0 || !is_weight_type(wtype)) return 0;
    return (size_t)N * (size_t)padded_blocks(K) * (size_t)block_bytes(wtype);
}

int qg_repack_weights(const void* B, void* B_packed, int N, int K, int wtype, qg_stream_t stream) {
    const int rc = precheck({N}, K, 32, is_weight_type(wtype), {{B, 1}, {B_packed, 15}});
    if (rc != QG_GO) return rc;
    const int bb = block_bytes(wtype);
    return hip_status(launch_pad_rows(B, B_packed, N, (K / 32) * bb, padded_blocks(K) * bb, (hipStream_t)stream));
}

int qg_quantize_q8_1_padded(const float* x, void* y, int M, int K, qg_stream_t stream) {
    const int rc = precheck({M}, K, 32, true, {{x, 3}, {y, 3}});
    if (rc != QG_GO) return rc;
    return hip_status(launch_quantize_q8_1_padded(x, y, M, K / 32, padded_blocks(K), (hipStream_t)stream));
}

int qg_gemm_w4a8_padded(const void* A_padded, const void* B_packed, float* C, int M, int N, int K, int wtype,
                        qg_stream_t stream) {
    // by hand: the logical K is checked before anything (M = -1, K = 33 is BAD_K here), the product sees K'
    if (K <= 0 || K % 32 != 0) return QG_ERR_BAD_K;
    GemmArgs g = product_args(A_padded, B_packed, C, M, N, padded_blocks(K) * 32, wtype);
    return run_product(g, QG_ALGO_AUTO, (hipStream_t)stream, false);
}

size_t qg_gemm_w4a8_prepacked_workspace_size(int M, int K) {
    if (M <= 0 || K <= 0 || K % 32 != 0 || padded_blocks(K) == K / 32) return 0;
    return (size_t)M * (size_t)padded_blocks(K) * 36;
}

int qg_gemm_w4a8_prepacked(const void* A, const void* B_packed, float* C, int M, int N, int K, int wtype,
                           void* workspace, size_t workspace_bytes, qg_stream_t stream) {
    // (alignment is left to the route taken below: the MFMA kernel's eligibility, the pad copy, run_product)
    const int rc = precheck({M, N}, K, 32, is_weight_type(wtype), {{A, 0}, {B_packed, 0}, {C, 0}});
    if (rc != QG_GO) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const int nbp = padded_blocks(K);
    GemmArgs g = product_args(A, B_packed, C, M, N, nbp * 32, wtype);
    if (nbp != K / 32) {
        // round 5: where the MFMA kernel runs (M >= 5), it reads the plain activation rows itself
        // (activation windows against the padded weight rows, qg_mmq_kernel.hpp AW): one launch, no
        // workspace touched
        GemmArgs w = g;
        w.K = K;
        w.nbw = nbp;
        if (M > 4 && mfma_eligible(w)) return hip_status(launch_mfma(w, st));
        // otherwise the activations are padded into the caller's workspace, same zero blocks
        if (!workspace || workspace_bytes < qg_gemm_w4a8_prepacked_workspace_size(M, K)) return QG_ERR_INVALID_ARG;
        if (((uintptr_t)A & 1) != 0 || ((uintptr_t)workspace & 15) != 0) return QG_ERR_ALIGN;
        const hipError_t e = launch_pad_rows(A, workspace, M, (K / 32) * 36, nbp * 36, st);
        if (e != hipSuccess) return hip_status(e);
        g.A = workspace;
    }
    return run_product(g, QG_ALGO_AUTO, st, false);
}

size_t qg_tile_weights_bytes(int N, int K, int wtype) {
    if (N < 0 || K <= 0 || K % 32 != 0 || !is_weight_type(wtype)) return 0;
    return tiled_weight_bytes(N, K, wtype);
}

int qg_tile_weights(const void* B, void* B_tiled, int N, int K, int wtype, qg_stream_t stream) {
    const int rc = precheck({N}, K, 32, is_weight_type(wtype), {{B, 1}, {B_tiled, 15}});
    if (rc != QG_GO) return rc;
    return hip_status(launch_tile_weights(B, B_tiled, N, K, wtype, (hipStream_t)stream));
}

int qg_gemm_w4a8_tiled_ldc(const void* A, const void* B_tiled, float* C, int M, int N, int K, int64_t ldc, int wtype,
                           qg_stream_t stream) {
    return tiled_product(LAY_TILED, A, B_tiled, C, M, N, K, ldc, wtype, stream);
}

int qg_gemm_w4a8_tiled(const void* A, const void* B_tiled, float* C, int M, int N, int K, int wtype, qg_stream_t stream) {
    return qg_gemm_w4a8_tiled_ldc(A, B_tiled, C, M, N, K, N, wtype, stream);
}

int qg_debug_sumi_tiled(const void* A, const void* B_tiled, int32_t* sumi, int M, int N, int K, int wtype,
                        qg_stream_t stream) {
    return tiled_sumi(LAY_TILED, A, B_tiled, sumi, M, N, K, wtype, stream);
}

int qg_debug_config_tiled(int M, int N, int K, int wtype, int sumi, char* buf, size_t len) {
    return describe_product(LAY_TILED, M, N, K, wtype, QG_ALGO_AUTO, sumi, buf, len);
}

// ---- round 5: tiled activations (LAY_TILED_ACT) -------------------------------------------------------
size_t qg_activations_tiled_bytes(int M, int K) {
    if (M < 0 || K <= 0 || K % 32 != 0) return 0;
    return tiled_act_bytes(M, K);
}

int qg_quantize_q8_1_tiled(const float* x, void* A_tiled, int M, int K, qg_stream_t stream) {
    const int rc = precheck({M}, K, 32, true, {{x, 15}, {A_tiled, 15}});
    if (rc != QG_GO) return rc;
    return hip_status(launch_quantize_q8_1_tiled(x, A_tiled, M, K, (hipStream_t)stream));
}

int qg_tile_activations(const void* A_q8_1, void* A_tiled, int M, int K, qg_stream_t stream) {
    const int rc = precheck({M}, K, 32, true, {{A_q8_1, 3}, {A_tiled, 15}});
    if (rc != QG_GO) return rc;
    return hip_status(launch_tile_activations(A_q8_1, A_tiled, M, K, (hipStream_t)stream));
}

int qg_gemm_w4a8_tiled_act_ldc(const void* A_tiled, const void* B_tiled, float* C, int M, int N, int K, int64_t ldc, int wtype,
                               qg_stream_t stream) {
    return tiled_product(LAY_TILED_ACT, A_tiled, B_tiled, C, M, N, K, ldc, wtype, stream);
}

int qg_gemm_w4a8_tiled_act(const void* A_tiled, const void* B_tiled, float* C, int M, int N, int K, int wtype,
                           qg_stream_t stream) {
    return qg_gemm_w4a8_tiled_act_ldc(A_tiled, B_tiled, C, M, N, K, N, wtype, stream);
}

int qg_debug_sumi_tiled_act(const void* A_tiled, const void* B_tiled, int32_t* sumi, int M, int N, int K, int wtype,
                            qg_stream_t stream) {
    return tiled_sumi(LAY_TILED_ACT, A_tiled, B_tiled, sumi, M, N, K, wtype, stream);
}

int qg_debug_config_tiled_act(int M, int N, int K, int wtype, int sumi, char* buf, size_t len) {
    return describe_product(LAY_TILED_ACT, M, N, K, wtype, QG_ALGO_AUTO, sumi, buf, len);
}

// qg_gemm_w4a8_grouped and qg_group_config: the items are validated alike, then launched or described
// (describe != nullptr: the route of the first launch is written there and nothing is enqueued).
static int run_grouped(const qg_gemv_item* items, int count, int M, int K, int wtype, hipStream_t st, char* describe,
                       size_t describe_len) {
    // by hand: the items pointer is checked with the sizes, and M == 0 is a no-op only after every item's sizes
    // and pointers have been checked (below)
    if (count < 0 || M < 0 || (count > 0 && !items)) return QG_ERR_INVALID_ARG;
    if (K <= 0 || K % 32 != 0) return QG_ERR_BAD_K;
    if (!is_weight_type(wtype)) return QG_ERR_UNSUPPORTED;
    auto item_args = [&](const qg_gemv_item& it) {
        GemmArgs g = product_args(it.A_q8_1, it.B, it.C, M, it.N, K, wtype);
        if (it.ldc) g.ldc_m = it.ldc;
        return g;
    };
    // validate every item before anything is enqueued; one launch only if AUTO picks the GEMV for all
    bool one_launch = M > 0 && M <= 4;  // the grouped GEMV is instantiated for MT <= 4 (qg_gemv_kernel.hpp)
    for (int i = 0; i < count; ++i) {
        const qg_gemv_item& it = items[i];
        if (it.N < 0 || it.ldc < 0 || (it.ldc != 0 && it.ldc < it.N)) return QG_ERR_INVALID_ARG;
        if (it.N == 0 || M == 0) continue;
        if (!it.A_q8_1 || !it.B || !it.C) return QG_ERR_INVALID_ARG;
        if (((uintptr_t)it.B & 1) != 0) return QG_ERR_ALIGN;
        const GemmArgs g = item_args(it);
        one_launch = one_launch && select_algo(g) == QG_ALGO_GEMV && gemv_eligible(g);
    }
    if (M == 0) {
        describe_line(describe, describe_len, "%s", "none");
        return QG_OK;
    }
    if (!one_launch) {
        if (describe) {
            describe_line(describe, describe_len, "%s", "items: one qg_gemm_w4a8 launch per item");
            return QG_OK;
        }
        for (int i = 0; i < count; ++i) {
            if (items[i].N == 0) continue;
            GemmArgs g = item_args(items[i]);
            const int rc = run_product(g, QG_ALGO_AUTO, st, false);
            if (rc != QG_OK) return rc;
        }
        return QG_OK;
    }
    describe_line(describe, describe_len, "%s", "none");
    for (int i0 = 0; i0 < count;) {
        GemvGroup grp = {};
        grp.M = M; grp.K = K;
        for (; i0 < count && grp.count < GEMV_GROUP_MAX; ++i0) {
            const qg_gemv_item& it = items[i0];
            if (it.N == 0) continue;
            grp.it[grp.count++] = GemvItemDesc{it.A_q8_1, it.B, it.C, it.N, it.ldc ? it.ldc : it.N};
        }
        if (grp.count == 0) break;
        GemmArgs q = group_args(grp, wtype);
        q.describe = describe;
        q.describe_len = describe_len;
        const int rc = hip_status(launch_gemv(q, st));
        if (rc != QG_OK || describe) return rc;
    }
    return QG_OK;
}

int qg_gemm_w4a8_grouped(const qg_gemv_item* items, int count, int M, int K, int wtype, qg_stream_t stream) {
    return run_grouped(items, count, M, K, wtype, (hipStream_t)stream, nullptr, 0);
}

int qg_group_config(const qg_gemv_item* items, int count, int M, int K, int wtype, char* buf, size_t len) {
    if (!buf || len == 0) return QG_ERR_INVALID_ARG;
    buf[0] = 0;
    return run_grouped(items, count, M, K, wtype, nullptr, buf, len);
}

void qg_set_group_affine(int mode) { set_group_affine(mode); }

int qg_gemm_w4a8(const void* A, const void* B, float* C, int M, int N, int K, int wtype, qg_stream_t stream) {
    return qg_gemm_w4a8_ex(A, B, C, M, N, K, wtype, QG_ALGO_AUTO, stream);
}

int qg_gemm_q4_0_q8_1_w4a8(const void* A_q8_1, const void* B_q4_0, float* C, int M, int N, int K,
                           qg_stream_t stream) {
    return qg_gemm_w4a8_ex(A_q8_1, B_q4_0, C, M, N, K, QG_TYPE_Q4_0, QG_ALGO_AUTO, stream);
}

int qg_gemm_q4_0_q8_1(const void* W, const void* A, float* out, int M, int N, int K, qg_stream_t s) {
    return weight_major(QG_TYPE_Q4_0, W, A, out, M, N, K, s);
}
int qg_gemm_q4_1_q8_1(const void* W, const void* A, float* out, int M, int N, int K, qg_stream_t s) {
    return weight_major(QG_TYPE_Q4_1, W, A, out, M, N, K, s);
}
int qg_gemm_q5_0_q8_1(const void* W, const void* A, float* out, int M, int N, int K, qg_stream_t s) {
    return weight_major(QG_TYPE_Q5_0, W, A, out, M, N, K, s);
}
int qg_gemm_q5_1_q8_1(const void* W, const void* A, float* out, int M, int N, int K, qg_stream_t s) {
    return weight_major(QG_TYPE_Q5_1, W, A, out, M, N, K, s);
}
int qg_gemm_q8_0_q8_1(const void* W, const void* A, float* out, int M, int N, int K, qg_stream_t s) {
    return weight_major(QG_TYPE_Q8_0, W, A, out, M, N, K, s);
}

int qg_gemm_w8a8(const void* A, const void* B, float* C, int M, int N, int K, qg_stream_t stream) {
    return qg_gemm_w4a8_ex(A, B, C, M, N, K, QG_TYPE_Q8_0, QG_ALGO_AUTO, stream);
}

int qg_quantize(int type, int variant, const float* x, void* y, int64_t k, qg_stream_t stream) {
    const bool type_ok = block_bytes(type) != 0 && !is_routed_type(type);  // (no Q4_K / Q6_K / MXFP4 quantizer)
    const bool variant_ok = variant == 0 || (variant == 1 && type == QG_TYPE_Q8_1) ||
                            (variant == 2 && (type == QG_TYPE_Q8_1 || type == QG_TYPE_Q4_0));
    const int rc = precheck_count(k, 32, type_ok && variant_ok, {{x, 3}, {y, type == QG_TYPE_Q8_1 ? 3u : 1u}});
    if (rc != QG_GO) return rc;
    return hip_status(launch_quantize(type, variant, x, y, k / 32, (hipStream_t)stream));
}

int qg_quantize_q8_1(const float* x, void* y, int64_t k, qg_stream_t s) { return qg_quantize(QG_TYPE_Q8_1, 0, x, y, k, s); }
int qg_quantize_q4_0(const float* x, void* y, int64_t k, qg_stream_t s) { return qg_quantize(QG_TYPE_Q4_0, 0, x, y, k, s); }
int qg_quantize_q8_1_definition(const float* x, void* y, int64_t num_elements, qg_stream_t s) {
    return qg_quantize(QG_TYPE_Q8_1, QG_QVAR_DEFINITION, x, y, num_elements, s);
}
int qg_quantize_q4_0_definition(const float* x, void* y, int64_t num_elements, qg_stream_t s) {
    return qg_quantize(QG_TYPE_Q4_0, QG_QVAR_DEFINITION, x, y, num_elements, s);
}

int qg_dequantize(int type, const void* x, float* y, int64_t k, qg_stream_t stream) {
    const int be = is_sb_type(type) ? 256 : 32;  // (an unknown type: the 32-element granule, then refused)
    const int rc = precheck_count(k, be, block_bytes(type) != 0, {{x, is_mxfp4_type(type) ? 0u : 1u}, {y, 3}});
    if (rc != QG_GO) return rc;
    if (is_mxfp4_type(type)) return hip_status(launch_dequantize_mxfp4(x, y, k / 32, (hipStream_t)stream));
    if (is_q6k_type(type)) return hip_status(launch_dequantize_q6k(x, y, k / 256, (hipStream_t)stream));
    if (is_q4k_type(type)) return hip_status(launch_dequantize_q4k(x, y, k / 256, (hipStream_t)stream));
    return hip_status(launch_dequantize(type, x, y, k / 32, (hipStream_t)stream));
}

int qg_dequantize_q4_0(const void* x, float* y, int64_t k, qg_stream_t s) { return qg_dequantize(QG_TYPE_Q4_0, x, y, k, s); }

int qg_debug_sumi(const void* A, const void* B, int32_t* sumi, int M, int N, int K, int wtype, int algo,
                  qg_stream_t stream) {
    GemmArgs g = product_args(A, B, nullptr, M, N, K, wtype);
    g.sumi = sumi;
    return run_product(g, algo, (hipStream_t)stream);
}

int qg_debug_config(int M, int N, int K, int wtype, int algo, int sumi, char* buf, size_t len) {
    return describe_product(LAY_ROWS, M, N, K, wtype, algo, sumi, buf, len);
}

int qg_gemm_w4a8_ldc(const void* A, const void* B, float* C, int M, int N, int K, int64_t ldc, int wtype, int algo,
                     qg_stream_t stream) {
    if (ldc < N || (M > 1 && ldc <= 0)) return QG_ERR_INVALID_ARG;
    GemmArgs g = product_args(A, B, C, M, N, K, wtype);
    g.ldc_m = (long)ldc;
    return run_product(g, algo, (hipStream_t)stream);
}

int qg_gemm_w4a8_from_view(const qg_tensor_view* act, const qg_tensor_view* w, qg_tensor_view* out,
                           const char* kernel_type, qg_stream_t stream) {
    if (!act || !w || !out) return QG_ERR_INVALID_ARG;
    int algo = QG_ALGO_AUTO;
    if (kernel_type) {
        static const char* autos[] = {"naive", "tiled", "dp4a", "tiled_dp4a", "vectorized_dp4a", "auto"};
        bool known = false;
        for (const char* a : autos) known = known || strcmp(kernel_type, a) == 0;
        if (known) algo = QG_ALGO_AUTO;
        else if (strcmp(kernel_type, "gemv") == 0) algo = QG_ALGO_GEMV;
        else if (strcmp(kernel_type, "mfma") == 0) algo = QG_ALGO_MFMA;
        else if (strcmp(kernel_type, "generic") == 0) algo = QG_ALGO_GENERIC;
        else if (strcmp(kernel_type, "ragged") == 0) algo = QG_ALGO_RAGGED;
        else return QG_ERR_INVALID_ARG;
    }
    if (act->type != QG_TYPE_Q8_1 || out->type != QG_TYPE_F32 || !(is_weight_type(w->type) || is_routed_type(w->type)))
        return QG_ERR_UNSUPPORTED;
    int64_t M, N, K;
    const int rc = view_dims(act, w, out, M, N, K, block_elems(w->type));  // super-block types: K % 256
    if (rc != QG_OK) return rc;
    return qg_gemm_w4a8_ex(act->data, w->data, (float*)out->data, (int)M, (int)N, (int)K, w->type, algo, stream);
}

int qg_gemm_w4a16_from_view(const qg_tensor_view* act, const qg_tensor_view* w, qg_tensor_view* out,
                            const char* kernel_type, qg_stream_t stream) {
    if (!act || !w || !out) return QG_ERR_INVALID_ARG;
    if (!baseline_kernel_type(kernel_type)) return QG_ERR_INVALID_ARG;
    if (act->type != QG_TYPE_F32 || out->type != QG_TYPE_F32 || (w->type != QG_TYPE_Q4_0 && w->type != QG_TYPE_Q8_0))
        return QG_ERR_UNSUPPORTED;
    int64_t M, N, K;
    const int rc = view_dims(act, w, out, M, N, K);
    if (rc != QG_OK) return rc;
    return run_w16(w->type, (const float*)act->data, w->data, (float*)out->data, (int)M, (int)N, (int)K,
                   (hipStream_t)stream);
}

int qg_gemm_fp32_from_view(const qg_tensor_view* act, const qg_tensor_view* w, qg_tensor_view* out,
                           const char* kernel_type, qg_stream_t stream) {
    if (!act || !w || !out) return QG_ERR_INVALID_ARG;
    if (!baseline_kernel_type(kernel_type)) return QG_ERR_INVALID_ARG;
    if (act->type != QG_TYPE_F32 || out->type != QG_TYPE_F32 || w->type != QG_TYPE_F32) return QG_ERR_UNSUPPORTED;
    int64_t M, N, K;
    const int rc = view_dims(act, w, out, M, N, K, 1);
    if (rc != QG_OK) return rc;
    return qg_gemm_fp32((const float*)act->data, (const float*)w->data, (float*)out->data, (int)M, (int)N, (int)K,
                        stream);
}

int qg_validate_view_types(const qg_tensor_view* act, const qg_tensor_view* w, const qg_tensor_view* out,
                           int expected_activation_type, int expected_weight_type, int expected_output_type) {
    return act && w && out && act->type == expected_activation_type && w->type == expected_weight_type &&
           out->type == expected_output_type;
}

int qg_gemm_fp32(const float* A, const float* B, float* C, int M, int N, int K, qg_stream_t stream) {
    // no K granule, and K = 0 is a product (of nothing), not an empty call: K is checked here, the rest as everywhere
    if (K < 0) return QG_ERR_INVALID_ARG;
    const int rc = precheck({M, N}, 1, 1, true, {{A, 3}, {B, 3}, {C, 3}});
    if (rc != QG_GO) return rc;
    GemmArgs g = product_args(A, B, C, M, N, K, 0);
    return hip_status(launch_fp32(g, (hipStream_t)stream));
}

const char* qg_status_string(int s) {
    switch (s) {
        case QG_OK: return "ok";
        case QG_ERR_INVALID_ARG: return "invalid argument";
        case QG_ERR_BAD_K: return "K must be a positive multiple of 32";
        case QG_ERR_UNSUPPORTED: return "unsupported type or algorithm for this shape";
        case QG_ERR_ALIGN: return "pointer misaligned for the block format";
        case QG_ERR_HIP: return "HIP launch error";
    }
    return "unknown status";
}

int qg_last_hip_error(void) { return g_last_hip; }

void qg_set_capture_fusion(int on) { set_capture_fusion(on); }

void qg_capture_fusion_stats(uint64_t* merged, uint64_t* nodes) { capture_fusion_stats(merged, nodes); }

int qg_select_algo(int M, int N, int K, int wtype) {
    return select_product_algo(query_args(M, N, K, wtype));
}

int qg_block_bytes(int type) { return block_bytes(type); }

int qg_block_elems(int type) { return block_elems(type); }

const char* qg_version(void) { return "qg-mi355x 0.1.0 (gfx950)"; }

}  // extern "C"
