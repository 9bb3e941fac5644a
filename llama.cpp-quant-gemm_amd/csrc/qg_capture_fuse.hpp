// qg_capture_fuse.hpp — the hazard test of the capture-time GEMV merge (qg_capture_fuse.hip, capture_gemv).
//
// Under stream capture, a GEMV whose only capture dependency is a GEMV node this library created is
// merged into that node (one grouped launch, gemvg_kernel) when it is independent of the node's items.
// This header decides "independent" from the operands' byte spans alone. Pure host code, no HIP
// includes: tests/capture_fuse_host_test.cpp builds it with a plain C++ compiler under sanitizers.
//
// Spans of one item (M activation rows, N weight rows, K elements per row, bb bytes per weight block):
//   A: M * (K/32) * 36 bytes (Q8_1 blocks), read
//   B: N * (K/32) * bb bytes, read
//   C: ((M-1) * ldc + N) * 4 bytes, written — ONE conservative span for rows strided by ldc floats
// A new item may join a group iff its C span is disjoint from every earlier item's A, B and C spans
// (write-after-read, write-after-write) and its A and B spans are disjoint from every earlier item's
// C span (read-after-write). Shared A or B among items is fine: both are only read. Arithmetic in
// uintptr_t; a span whose size or end overflows counts as overlapping everything.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace qg {
namespace fuse {

constexpr int MAX_ITEMS = 64;  // == GEMV_GROUP_MAX (qg_kernels.hpp; static_assert in qg_capture_fuse.hip)

struct Span {
    uintptr_t lo, hi;  // [lo, hi)
    bool bad;          // size or end overflowed: overlaps everything
};

inline bool mul_ovf(uintptr_t a, uintptr_t b, uintptr_t* r) {
    if (a != 0 && b > UINTPTR_MAX / a) return true;
    *r = a * b;
    return false;
}

inline Span make_span(const void* p, uintptr_t bytes, bool size_ovf) {
    Span s;
    s.lo = (uintptr_t)p;
    s.hi = s.lo + bytes;
    s.bad = size_ovf || s.hi < s.lo;
    return s;
}

// touching spans ([a, b) and [b, c)) are disjoint; an empty span overlaps nothing
inline bool overlap(const Span& x, const Span& y) {
    if (x.bad || y.bad) return true;
    if (x.lo == x.hi || y.lo == y.hi) return false;
    return x.lo < y.hi && y.lo < x.hi;
}

struct ItemSpans {
    Span a, b, c;
};

// M, N >= 1, K a positive multiple of 32, ldc >= 0 floats (the caller has validated them)
inline ItemSpans item_spans(const void* A, const void* B, const void* C, int M, int N, int K, int64_t ldc,
                            int block_bytes) {
    const uintptr_t nb = (uintptr_t)(K / 32);
    uintptr_t t = 0, bytes = 0;
    ItemSpans s;
    bool o = mul_ovf((uintptr_t)M, nb, &t) || mul_ovf(t, 36, &bytes);
    s.a = make_span(A, bytes, o);
    o = mul_ovf((uintptr_t)N, nb, &t) || mul_ovf(t, (uintptr_t)block_bytes, &bytes);
    s.b = make_span(B, bytes, o);
    o = ldc < 0 || mul_ovf((uintptr_t)(M - 1), (uintptr_t)ldc, &t);
    if (!o) {
        o = t + (uintptr_t)N < t;
        t += (uintptr_t)N;
    }
    o = o || mul_ovf(t, 4, &bytes);
    s.c = make_span(C, bytes, o);
    return s;
}

// may `x` run concurrently with (in one launch as) the earlier item `e`?
inline bool independent(const ItemSpans& e, const ItemSpans& x) {
    if (overlap(x.c, e.a) || overlap(x.c, e.b) || overlap(x.c, e.c)) return false;
    if (overlap(x.a, e.c) || overlap(x.b, e.c)) return false;
    return true;
}

// The spans of a group under construction: what the merge keeps beside the kernel's descriptor.
struct Group {
    int count = 0;
    ItemSpans it[MAX_ITEMS];
};

inline bool can_join(const Group& g, const ItemSpans& x) {
    if (g.count >= MAX_ITEMS) return false;
    for (int i = 0; i < g.count; ++i)
        if (!independent(g.it[i], x)) return false;
    return true;
}

inline bool join(Group& g, const ItemSpans& x) {
    if (!can_join(g, x)) return false;
    g.it[g.count++] = x;
    return true;
}

}  // namespace fuse
}  // namespace qg
