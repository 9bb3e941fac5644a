// qg_capture_fuse.hip — the capture-time merge of back-to-back GEMVs (hazard test: qg_capture_fuse.hpp).
// The C-ABI (qg_api.hip) sees launch_or_merge_gemv, set_capture_fusion and capture_fusion_stats (qg_kernels.hpp).
#include <stdlib.h>

#include <algorithm>
#include <atomic>

#include "../../include/qg/qg.h"
#include "qg_capture_fuse.hpp"
#include "qg_kernels.hpp"

namespace qg {
namespace {
// ---- capture-time merge of back-to-back GEMVs (qg.h at qg_gemm_w4a8; hazard test: qg_capture_fuse.hpp) ----
// A GEMV enqueued on a capturing stream whose ONLY capture dependency is a GEMV node this thread created in
// the same capture, and which is independent of that node's items, adds no node: the node is rewritten
// (hipGraphKernelNodeSetParams) into one grouped launch over all of them — the gemvg_kernel, grid and LDS
// qg_gemm_w4a8_grouped would launch for the same items, so every output keeps its bits. The merged node keeps
// the first node's predecessors and the new GEMV's only predecessor was that node, so the only ordering
// removed is between items of the group (independent by the hazard test); successors captured earlier
// (forked streams) merely wait for one more item. Any error on the way is swallowed and the call takes the
// plain launch: a call that succeeds unmerged never fails merged.
static_assert(fuse::MAX_ITEMS == GEMV_GROUP_MAX, "qg_capture_fuse.hpp and qg_kernels.hpp disagree on the group size");
std::atomic<int> g_fuse_mode{-1};  // 0 off, 1 on (the measured classes), 2 every class (A/B runs); -1: not read yet
std::atomic<uint64_t> g_fuse_merged{0}, g_fuse_nodes{0};

int fuse_mode() {
    int m = g_fuse_mode.load(std::memory_order_relaxed);
    if (m >= 0) return m;
    const char* e = getenv("QG_CAPTURE_FUSE");  // read once: the default until qg_set_capture_fusion
    m = e && e[0] == '0' && !e[1] ? 0 : e && e[0] == '2' && !e[1] ? 2 : 1;
    int unset = -1;
    g_fuse_mode.compare_exchange_strong(unset, m, std::memory_order_relaxed);
    return g_fuse_mode.load(std::memory_order_relaxed);
}

// The node the calling thread's last captured GEMV created or merged into. Capture ids are unique, so a
// stale record never matches a later capture.
struct FuseRecord {
    bool valid = false;
    unsigned long long id = 0;
    hipGraphNode_t node = nullptr;
    int wtype = 0;
    GemvGroup grp = {};
    fuse::Group spans;
    bool no_affine = false;  // the node refused the strided batch's kernel once: grouped from then on
};
thread_local FuseRecord t_fuse;


// exactly the calls gemv_launch has a grouped form for (qg_gemv_kernel.hpp)
bool fuse_candidate(const GemmArgs& g) {
    return g.batch == 1 && g.ldc_n == 1 && !g.sumi && !g.describe && !g.group && g.ain == AIN_Q8_1 && g.nbw == 0 &&
           g.lay == LAY_ROWS && g.M <= 4 && g.ldc_m >= 0 && g.ldc_m <= INT32_MAX;
}

// Shape classes the merge is enabled for, by measurement: tools/ab_capture_fuse.py (64 GEMVs per step on
// distinct weight copies, merge off vs on in one process, interleaved rounds; us per GEMV, unfused -> fused),
// profiles/capture_fuse/ab_capture_fuse.txt. Enabled where fused beats unfused by more than the unfused
// arm's run-to-run spread (0.1 .. 5.4 % of its median):
//  * the loop-free one-unit form (nf.one; K <= 4096 and the short rows), any M <= 4, any row count. N = K =
//    4096: Q4_0 M = 1 3.354 -> 1.513, M = 2 3.823 -> 1.661, M = 4 4.517 -> 2.545, Q4_1 3.585 -> 1.682, Q5_0
//    3.878 -> 1.833, Q5_1 3.958 -> 2.006, Q8_0 4.611 -> 2.757; K = 2048 2.559 -> 0.771. More than one
//    dispatch round: Q4_0 N = 11008 6.598 -> 4.032, N = 14336 7.627 -> 5.228 (M = 2 8.189 -> 6.055), N = 32000
//    M = 1 12.491 -> 11.405, M = 2 15.000 -> 13.000, M = 4 24.757 -> 20.039, Q8_0 N = 32000 22.433 -> 21.238.
//  * the unit loop (K > 4096, K = 3072) at M = 1 (the grouped kernel loops where the Q4_0 single launch is
//    multi-unit): Q4_0 K = 3072 3.102 -> 1.156, K = 8192 4.891 -> 2.925, K = 11008 6.213 -> 3.953, K = 14336
//    7.709 -> 5.147; K = 14336 Q4_1 8.122 -> 5.700, Q5_1 10.893 -> 6.979, Q8_0 12.470 -> 9.597.
// Not merged: the unit loop at M >= 2. N = 4096, K = 14336: M = 2 8.720 -> 8.839, M = 3 10.111 -> 14.542,
// M = 4 10.819 -> 28.244 (the grouped unit loop at M tiles of 4 spills); M = 2 wins at K = 8192 (5.823 ->
// 3.815), K = 11008 (7.086 -> 6.021) and N = 8192, K = 14336 (15.654 -> 12.437), but the class is not a win
// throughout, so it stays off. M = 3 is not measured in the one-unit form (it runs the M = 4 instantiation).
bool fuse_class_enabled(const GemvNodeFill& nf, int M, int mode) {
    if (mode == 2) return true;
    return nf.one || M == 1;
}

hipError_t capture_gemv(const GemmArgs& g, hipStream_t st) {
    FuseRecord& r = t_fuse;
    unsigned long long id = 0;
    const hipGraphNode_t* deps = nullptr;
    size_t nd = 0;
    auto capturing = [&]() {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        hipGraph_t graph = nullptr;
        if (hipStreamGetCaptureInfo_v2(st, &cs, &id, &graph, &deps, &nd) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        return cs == hipStreamCaptureStatusActive;
    };
    if (!capturing()) {
        r.valid = false;
        return launch_gemv(g, st);
    }
    const int mode = fuse_mode();
    const fuse::ItemSpans sp = fuse::item_spans(g.A, g.B, g.C, g.M, g.N, g.K, g.ldc_m, block_bytes(g.wtype));
    if (mode && r.valid && r.id == id && nd == 1 && deps[0] == r.node && r.grp.M == g.M && r.grp.K == g.K &&
        r.wtype == g.wtype && r.grp.count < GEMV_GROUP_MAX && fuse::can_join(r.spans, sp)) {
        GemvGroup grp = r.grp;
        grp.it[grp.count++] = GemvItemDesc{g.A, g.B, g.C, g.N, (int)g.ldc_m};
        GemvNodeFill nf;
        GemmArgs q = group_args(grp, g.wtype);
        q.node_fill = &nf;
        if (r.no_affine) q.affine = -1;
        nf.p = hipKernelNodeParams{};
        hipError_t e = launch_gemv(q, st);  // launches nothing: the grouped launch's kernel, grid, block, LDS
        if (e == hipSuccess && !(nf.p.func && fuse_class_enabled(nf, g.M, mode))) e = hipErrorNotSupported;
        if (e == hipSuccess) {
            e = hipGraphKernelNodeSetParams(r.node, &nf.p);
            // The runtime refuses some changes of a node's kernel (seen: hipErrorLaunchFailure for the strided
            // batch's 512-thread kernel on a node that held a 256-thread gemvg_kernel, Q5_0 / Q5_1 at N = 4096).
            // The node is unchanged then: it takes the grouped kernel, for this call and the node's later ones.
            if (e != hipSuccess && nf.affine) {
                (void)hipGetLastError();
                r.no_affine = true;
                q.affine = -1;
                e = launch_gemv(q, st);
                if (e == hipSuccess && !nf.p.func) e = hipErrorNotSupported;
                if (e == hipSuccess) e = hipGraphKernelNodeSetParams(r.node, &nf.p);
            }
        }
        if (e == hipSuccess) {
            r.grp = grp;
            fuse::join(r.spans, sp);
            g_fuse_merged.fetch_add(1, std::memory_order_relaxed);
            return hipSuccess;
        }
        (void)hipGetLastError();
    }
    r.valid = false;
    const hipError_t e = launch_gemv(g, st);
    if (e != hipSuccess) return e;
    g_fuse_nodes.fetch_add(1, std::memory_order_relaxed);
    // exactly one dependency now: the node just created
    if (capturing() && nd == 1) {
        r.valid = true;
        r.id = id;
        r.node = deps[0];
        r.wtype = g.wtype;
        r.no_affine = false;
        r.grp = GemvGroup{};
        r.grp.count = 1; r.grp.M = g.M; r.grp.K = g.K;
        r.grp.it[0] = GemvItemDesc{g.A, g.B, g.C, g.N, (int)g.ldc_m};
        r.spans.count = 0;
        fuse::join(r.spans, sp);
    }
    return hipSuccess;
}
}  // namespace

hipError_t launch_or_merge_gemv(const GemmArgs& g, hipStream_t st) {
    return fuse_candidate(g) ? capture_gemv(g, st) : launch_gemv(g, st);
}

void set_capture_fusion(int on) { g_fuse_mode.store(on == 2 ? 2 : on ? 1 : 0, std::memory_order_relaxed); }

void capture_fusion_stats(uint64_t* merged, uint64_t* nodes) {
    if (merged) *merged = g_fuse_merged.load(std::memory_order_relaxed);
    if (nodes) *nodes = g_fuse_nodes.load(std::memory_order_relaxed);
}

}  // namespace qg
