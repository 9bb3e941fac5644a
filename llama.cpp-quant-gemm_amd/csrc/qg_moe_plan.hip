// qg_moe_plan.hip — the plan kernel of the expert-grouped mul_mat_id entries (qg_moe_plan.hpp).
//
// moe_plan_kernel: one workgroup counting-sorts the T * n_used slots by expert id into the caller's workspace
// (MoePlanLayout): counts per bin (ids that name no expert: a bin of their own, the last), the slots and their
// activation rows in bin order, and one record {bin, first sorted position, rows} per tile of R = 1 << rsh rows with
// their number n_tiles. Its counters live in LDS and are zeroed by the kernel, so a replay starts clean. The order of
// the slots of one expert is whatever the LDS atomics give.
#include "qg_moe_plan.hpp"

namespace qg {
namespace {

constexpr int PLAN_WGS = 1024;
constexpr int PLAN_BINS = MOE_MAX_EXPERTS + 1;

// rsh: log2 of the tile's rows
__global__ __launch_bounds__(PLAN_WGS) void moe_plan_kernel(const MoePlanArgs a, int rsh) {
    __shared__ int cnt[PLAN_BINS];       // slots per bin; the scatter's cursors afterwards
    __shared__ int poff[PLAN_BINS + 1];  // first sorted position of a bin
    __shared__ int toff[PLAN_BINS + 1];  // first tile of a bin
    __shared__ int scan_p[PLAN_WGS], scan_t[PLAN_WGS];
    const int tid = threadIdx.x, E = a.n_expert, nbin = E + 1, R = 1 << rsh;
    const MoePlanLayout L = moe_plan_layout(a.slots, E);
    int32_t* __restrict__ ws = a.ws;

    for (int b = tid; b < nbin; b += PLAN_WGS) cnt[b] = 0;
    __syncthreads();
    for (int s = tid; s < a.slots; s += PLAN_WGS) {
        const int t = s / a.n_used, u = s - t * a.n_used;
        const int e = a.ids[(long)t * a.ids_stride + u];
        atomicAdd(&cnt[(unsigned)e < (unsigned)E ? e : E], 1);
    }
    __syncthreads();
    // exclusive prefix sums of the counts and of the tiles per bin: thread i owns bins [b0, b1)
    const int per = (nbin + PLAN_WGS - 1) / PLAN_WGS;
    const int b0 = min(tid * per, nbin), b1 = min(b0 + per, nbin);
    int sp = 0, stl = 0;
    for (int b = b0; b < b1; ++b) {
        sp += cnt[b];
        stl += (cnt[b] + R - 1) >> rsh;
    }
    scan_p[tid] = sp;
    scan_t[tid] = stl;
    __syncthreads();
    for (int d = 1; d < PLAN_WGS; d <<= 1) {
        const int vp = tid >= d ? scan_p[tid - d] : 0, vt = tid >= d ? scan_t[tid - d] : 0;
        __syncthreads();
        scan_p[tid] += vp;
        scan_t[tid] += vt;
        __syncthreads();
    }
    {
        int p = scan_p[tid] - sp, tl = scan_t[tid] - stl;
        for (int b = b0; b < b1; ++b) {
            poff[b] = p;
            toff[b] = tl;
            p += cnt[b];
            tl += (cnt[b] + R - 1) >> rsh;
        }
        if (tid == PLAN_WGS - 1) {
            poff[nbin] = scan_p[tid];
            toff[nbin] = scan_t[tid];
        }
    }
    __syncthreads();
    const int n_tiles = toff[nbin];
    if (tid == 0) *reinterpret_cast<int4*>(ws) = make_int4(n_tiles, poff[E], R, 0);
    for (int b = tid; b < nbin; b += PLAN_WGS) ws[L.counts + b] = cnt[b];
    // tile j belongs to the bin b with toff[b] <= j < toff[b + 1] (empty bins have no such j)
    for (int j = tid; j < n_tiles; j += PLAN_WGS) {
        int lo = 0, hi = nbin;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (toff[mid] <= j) lo = mid;
            else hi = mid;
        }
        const int i = j - toff[lo];
        reinterpret_cast<int4*>(ws + L.tiles)[j] = make_int4(lo, poff[lo] + (i << rsh), min(R, cnt[lo] - (i << rsh)), 0);
    }
    __syncthreads();
    for (int b = tid; b < nbin; b += PLAN_WGS) cnt[b] = poff[b];
    __syncthreads();
    for (int s = tid; s < a.slots; s += PLAN_WGS) {
        const int t = s / a.n_used, u = s - t * a.n_used;
        const int e = a.ids[(long)t * a.ids_stride + u];
        const int p = atomicAdd(&cnt[(unsigned)e < (unsigned)E ? e : E], 1);
        ws[L.sorted + p] = s;
        // a_rows is 1 (the token's one row) or n_used (a row per slot): u % a_rows
        ws[L.rows + p] = t * a.a_rows + (a.a_rows > 1 ? u : 0);
    }
}

}  // namespace

hipError_t launch_moe_plan_rows(const MoePlanArgs& a, int rsh, hipStream_t st) {
    hipLaunchKernelGGL(moe_plan_kernel, dim3(1), dim3(PLAN_WGS), 0, st, a, rsh);
    return hipGetLastError();
}

}  // namespace qg
