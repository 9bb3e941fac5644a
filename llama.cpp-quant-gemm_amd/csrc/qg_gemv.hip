// qg_gemv.hip — product instantiations and dispatch of the GEMV kernels (qg_gemv_kernel.hpp).
//
// Configuration from the tuning sweeps (profiles/tools_archive/gemv_probe.hip, profiles/r01_tuning/): M <= 4 with
// K >= 4096: 2-block units, 64 lanes (one wave) per row, 1024-thread workgroups (512 for M = 1 and
// N >= 16384); otherwise 4-block units (72 B for Q4_0), 32 lanes per row, 512-thread workgroups;
// short rows (K/32/4 < 32) 4 lanes per row; K/32 not a multiple of 4: 2-block units.
// The fused-quantization variants (AIN_F32 / AIN_F16_FUSED) share the configuration.
#include <stdlib.h>

#include <algorithm>

#include "qg_gemv_impl.hpp"

namespace qg {

// The affine route of grouped launches (gemv_pick): 0 off, 1 the measured classes
// (group_affine_class_enabled), 2 every class; -1: not read yet.
static std::atomic<int> g_affine_mode{-1};

int group_affine_mode() {
    int m = g_affine_mode.load(std::memory_order_relaxed);
    if (m >= 0) return m;
    const char* e = getenv("QG_GROUP_AFFINE");  // read once: the default until qg_set_group_affine
    m = e && e[0] == '0' && !e[1] ? 0 : e && e[0] == '2' && !e[1] ? 2 : 1;
    int unset = -1;
    g_affine_mode.compare_exchange_strong(unset, m, std::memory_order_relaxed);
    return g_affine_mode.load(std::memory_order_relaxed);
}

void set_group_affine(int mode) { g_affine_mode.store(mode == 2 ? 2 : mode ? 1 : 0, std::memory_order_relaxed); }

bool gemv_eligible(const GemmArgs& g) {
    switch (g.wtype) {
        case FMT_Q4_0: return ok_f<FMT_Q4_0>(g);
        case FMT_Q4_1: return ok_f<FMT_Q4_1>(g);
        case FMT_Q5_0: return ok_f<FMT_Q5_0>(g);
        case FMT_Q5_1: return ok_f<FMT_Q5_1>(g);
        case FMT_Q8_0: return ok_f<FMT_Q8_0>(g);
    }
    return false;
}

// ---- what is done with a pick (gemv_pick, qg_gemv_kernel.hpp): named, written into a graph node, or launched ----
namespace {
// qg_debug_config / qg_group_config: one line per family word. SUMI is not in it (describe_kernel, qg_kernels.hpp).
hipError_t describe_pick(const GemvPick& p) {
    static const char* const sig[] = {"m1", "short", "full"};
    if (p.sig == GEMV_SIG_GROUP)
        describe_kernel(p.a, "%s F=%d MT=%d BPL=%d LPR=%d WGS=%d PRE=%d ONEU=%d TPW=%d full=%d grid=%ux%u", p.family, p.F, p.MT,
                        p.BPL, p.LPR, p.WGS, p.PRE, p.ONEU, p.TPW, p.full, p.grid.x, p.grid.y);
    else if (p.affine)
        describe_kernel(p.a, "%s F=%d MT=%d BPL=%d LPR=%d WGS=%d PRE=%d ONEU=%d TPW=%d grid=%ux%u", p.family, p.F, p.MT, p.BPL,
                        p.LPR, p.WGS, p.PRE, p.ONEU, p.TPW, p.grid.x, p.grid.y);
    else
        describe_kernel(p.a, "%s F=%d MT=%d BPL=%d LPR=%d WGS=%d AIN=%d NT=%d PRE=%d ONEU=%d SIG=%s grid=%ux%u", p.family, p.F,
                        p.MT, p.BPL, p.LPR, p.WGS, p.AIN, p.NT, p.PRE, p.ONEU, sig[p.sig], p.grid.x, p.grid.y);
    return hipSuccess;
}

// The launch as a graph node's parameters: the kernel's arguments copied into nf, one argv per signature.
void fill_pick(const GemvPick& p, GemvNodeFill* nf) {
    const GemmArgs& g = p.a;
    auto argv = [&](std::initializer_list<void*> a) { std::copy(a.begin(), a.end(), nf->argv); };
    auto& r = nf->r;
    nf->p = hipKernelNodeParams{};  // func == nullptr: nothing to launch
    if (p.sig == GEMV_SIG_GROUP) {
        if (p.grid.x == 0 || p.grid.y == 0) return;
        nf->grp = *static_cast<const GemvGroup*>(g.group);
        nf->grp.full = p.full;
        nf->flags = p.flags;
        nf->tiles = (int)p.grid.x;
        argv({&nf->grp.M, &nf->grp.K, &nf->flags, &nf->tiles, nf->grp.it});
    } else {
        r = {(const uint32_t*)g.A, (const uint8_t*)g.B, g.sA, g.sB, g.M, g.N, g.K, g.C, g.sC, g.ldc_m, g.ldc_n, g.sumi,
             g.sumi ? (void*)g.sumi : (void*)g.C, (int)g.ldc_m, (int)g.ldc_n};  // (out: the parity hook's buffer)
        if (p.sig == GEMV_SIG_M1) argv({&r.A, &r.B, &r.N, &r.K, &r.out});
        else if (p.sig == GEMV_SIG_SHORT) argv({&r.A, &r.B, &r.M, &r.N, &r.K, &r.out, &r.ldc_m32, &r.ldc_n32});
        else argv({&r.A, &r.B, &r.sA, &r.sB, &r.M, &r.N, &r.K, &r.C, &r.sC, &r.ldc_m, &r.ldc_n, &r.sumi});
    }
    nf->one = p.one;
    nf->affine = p.affine;
    nf->p.func = const_cast<void*>(p.fn);
    nf->p.gridDim = p.grid;
    nf->p.blockDim = dim3(p.WGS);
    nf->p.sharedMemBytes = (unsigned)p.lds;
    nf->p.kernelParams = nf->argv;
}
}  // namespace

hipError_t gemv_run(const GemvPick& p, hipStream_t st) {
    if (p.a.describe) return describe_pick(p);
    // the kernel derives its tile count from N (gemv_body): the grid must be exactly that
    assert(p.sig == GEMV_SIG_GROUP || (int)p.grid.x == gemv_tiles(p.a.N, p.rpw));
    const hipError_t e = lds_opt_in(p.fn, p.lds, *p.lds_done);  // (a merged node's kernel too)
    if (e != hipSuccess) return e;
    // the merge's node and the launch here come from the same parameters
    GemvNodeFill local;
    GemvNodeFill* nf = p.a.node_fill ? p.a.node_fill : &local;
    fill_pick(p, nf);
    if (p.a.node_fill || !nf->p.func) return hipSuccess;
    return hipLaunchKernel(nf->p.func, nf->p.gridDim, nf->p.blockDim, nf->argv, p.lds, st);
}

hipError_t launch_gemv(const GemmArgs& g, hipStream_t st) {
    switch (g.wtype) {
        case FMT_Q4_0: return gemv_launch_fmt<FMT_Q4_0>(g, st);
        case FMT_Q4_1: return gemv_launch_fmt<FMT_Q4_1>(g, st);
        case FMT_Q5_0: return gemv_launch_fmt<FMT_Q5_0>(g, st);
        case FMT_Q5_1: return gemv_launch_fmt<FMT_Q5_1>(g, st);
        case FMT_Q8_0: return gemv_launch_fmt<FMT_Q8_0>(g, st);
    }
    return hipErrorInvalidValue;
}

}  // namespace qg
