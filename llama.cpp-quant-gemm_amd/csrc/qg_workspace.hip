// qg_workspace.hip — what the kernels' launchers ask of the process: the per-(device, stream) workspaces,
// the device's compute-unit count and the qg_debug_config description hook (declared in qg_kernels.hpp).
//
// The library's only allocations are the workspaces of stream_workspace below — slot 0 the W4A16 / W8A16
// split-K partials, slot 1 the odd-K/32 prefill's padded copies — made outside capture, never handed to a
// captured call (captured calls take the non-workspace kernels, or the caller's buffer through the _ws entry
// points), and grown only: growing one synchronizes its stream once (the library's one host sync, qg.h),
// qg_release_workspaces frees them.
#include <stdarg.h>
#include <stdio.h>

#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <utility>

#include "qg_kernels.hpp"

namespace qg {
namespace {
std::mutex g_ws_mu;  // guards the map; each entry has its own lock for its buffer
struct WsEntry {
    void* p = nullptr;
    size_t n = 0;
    std::mutex mu;
};
// key: (device, stream, slot) — slot 0 the W4A16 split-K workspace (its counters must stay zero
// between calls), slot 1 the padded-repack buffers of the odd-K/32 prefill (qg_repack.hip)
std::map<std::tuple<int, hipStream_t, int>, std::unique_ptr<WsEntry>> g_ws;
}  // namespace

void* stream_workspace(hipStream_t st, size_t bytes, int slot, std::unique_lock<std::mutex>* hold) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    // Never hand the library's buffer to a stream capture: a graph would keep its raw pointer,
    // and a later eager call that grows the buffer (or qg_release_workspaces) would free it under
    // the graph. Captured calls run without it; graphs pass their own workspace
    // through the _ws entry points.
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
        (void)hipGetLastError();
        return nullptr;
    }
    WsEntry* e;
    {
        std::lock_guard<std::mutex> lk(g_ws_mu);
        auto& up = g_ws[std::make_tuple(dev, st, slot)];
        if (!up) up.reset(new WsEntry);
        e = up.get();
    }
    // The entry's lock is held while the buffer grows and, with `hold`, until the caller has
    // enqueued every kernel that uses it (two host threads on one stream must not
    // interleave a multi-kernel sequence on one buffer).
    std::unique_lock<std::mutex> lk(e->mu);
    if (!e->p || e->n < bytes) {
        const size_t sz = std::max(bytes, (size_t)4 << 20);
        void* p = nullptr;
        if (hipMalloc(&p, sz) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
        if (hipMemsetAsync(p, 0, sz, st) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(p);
            return nullptr;
        }
        if (e->p) {
            // launches still queued on st may use the old block: the one host sync of the library,
            // once per growth (documented in qg.h; the _ws entry points never reach it)
            (void)hipStreamSynchronize(st);
            (void)hipFree(e->p);
        }
        e->p = p;
        e->n = sz;
    }
    void* p = e->p;
    if (hold) *hold = std::move(lk);
    return p;
}

int device_cus() {
    static std::atomic<int> cached[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        (void)hipGetLastError();
        return 256;
    }
    int v = cached[dev].load(std::memory_order_relaxed);
    if (v > 0) return v;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
        (void)hipGetLastError();
        cus = 256;
    }
    cached[dev].store(cus, std::memory_order_relaxed);
    return cus;
}

void describe_kernel(const GemmArgs& g, const char* fmt, ...) {
    if (!g.describe || g.describe_len == 0) return;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g.describe, g.describe_len, fmt, ap);
    va_end(ap);
}

void release_workspaces() {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    bool synced = false;
    for (auto& kv : g_ws) {
        std::lock_guard<std::mutex> le(kv.second->mu);
        if (kv.second->p) {
            if (!synced) (void)hipDeviceSynchronize();
            synced = true;
            (void)hipFree(kv.second->p);
        }
    }
    g_ws.clear();
}
}  // namespace qg
