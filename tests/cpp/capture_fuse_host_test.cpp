// Host test of the capture-time merge's hazard logic (csrc/qg_capture_fuse.hpp): pure host code,
// built with -fsanitize=address,undefined by tests/test_capture_fuse_host.py. Exit status 0 = all passed.
#include <stdio.h>

#include "qg_capture_fuse.hpp"

using namespace qg::fuse;

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            ++failures;                                                 \
        }                                                               \
    } while (0)

static const void* at(uintptr_t a) { return (const void*)a; }

// Q4_0 (18-B blocks) item at explicit addresses; M = 1, N = 64, K = 4096 unless said otherwise:
// A span 128 * 36 = 4608 B, B span 64 * 128 * 18 = 147456 B, C span 64 * 4 = 256 B
static ItemSpans item(uintptr_t a, uintptr_t b, uintptr_t c, int M = 1, int N = 64, int K = 4096, int64_t ldc = 64) {
    return item_spans(at(a), at(b), at(c), M, N, K, ldc, 18);
}

int main() {
    const uintptr_t A = 0x100000, B = 0x200000, C = 0x300000;
    const uintptr_t ASZ = 4608, BSZ = 147456, CSZ = 256;

    {  // span sizes
        const ItemSpans s = item(A, B, C);
        CHECK(!s.a.bad && s.a.hi - s.a.lo == ASZ);
        CHECK(!s.b.bad && s.b.hi - s.b.lo == BSZ);
        CHECK(!s.c.bad && s.c.hi - s.c.lo == CSZ);
        const ItemSpans q8 = item_spans(at(A), at(B), at(C), 4, 40, 256, 40, 34);
        CHECK(q8.a.hi - q8.a.lo == 4 * 8 * 36 && q8.b.hi - q8.b.lo == 40 * 8 * 34 && q8.c.hi - q8.c.lo == 4 * 40 * 4);
    }
    {  // disjoint spans; shared A and shared B are fine (read-only)
        const ItemSpans e = item(A, B, C);
        CHECK(independent(e, item(A + 0x10000, B + 0x40000, C + 0x1000)));
        CHECK(independent(e, item(A, B + 0x40000, C + 0x1000)));  // shared activations
        CHECK(independent(e, item(A + 0x10000, B, C + 0x1000)));  // shared weights
        CHECK(independent(e, item(A, B, C + 0x1000)));            // both shared, own output
    }
    {  // the five overlap kinds, each alone
        const ItemSpans e = item(A, B, C);
        const uintptr_t A2 = 0x500000, B2 = 0x600000, C2 = 0x700000;
        CHECK(independent(e, item(A2, B2, C2)));
        CHECK(!independent(e, item(A2, B2, A + ASZ - 4)));  // new C over earlier A (write-after-read)
        CHECK(!independent(e, item(A2, B2, B + 100)));      // new C over earlier B (write-after-read)
        CHECK(!independent(e, item(A2, B2, C)));            // new C over earlier C (write-after-write)
        CHECK(!independent(e, item(A2, B2, C + CSZ - 4)));  //   ... by one float
        CHECK(!independent(e, item(C, B2, C2)));            // new A over earlier C (read-after-write)
        CHECK(!independent(e, item(C - ASZ + 4, B2, C2)));  //   ... by its last dword
        CHECK(!independent(e, item(A2, C - BSZ + 2, C2)));  // new B over earlier C (read-after-write)
    }
    {  // touching but disjoint: [lo, hi) spans
        const ItemSpans e = item(A, B, C);
        CHECK(independent(e, item(0x500000, 0x600000, C + CSZ)));        // new C starts where earlier C ends
        CHECK(independent(e, item(0x500000, 0x600000, C - CSZ)));        // new C ends where earlier C starts
        CHECK(independent(e, item(0x500000, 0x600000, A + ASZ)));        // new C right after earlier A
        CHECK(independent(e, item(C + CSZ, 0x600000, 0x700000)));        // new A right after earlier C
        CHECK(independent(e, item(0x500000, C - BSZ, 0x700000)));        // new B ends where earlier C starts
        CHECK(!independent(e, item(0x500000, C - BSZ + 1, 0x700000)));   // one byte further: overlap
    }
    {  // overflow is overlap: span end past the address space, size products past uintptr_t
        const ItemSpans e = item(A, B, C);
        const ItemSpans hi = item(0x500000, 0x600000, UINTPTR_MAX - 100);  // C end wraps
        CHECK(hi.c.bad && !independent(e, hi));
        CHECK(!independent(hi, item(0x500000, 0x600000, 0x700000)));       // a bad earlier span blocks too
        const ItemSpans hb = item(0x500000, UINTPTR_MAX - 1000, 0x700000);
        CHECK(hb.b.bad && !independent(e, hb));
        const ItemSpans big = item_spans(at(0x500000), at(0x600000), at(0x700000), 4, 64, 4096, INT64_MAX, 18);
        CHECK(big.c.bad && !independent(e, big));                          // (M-1) * ldc overflows
        const ItemSpans neg = item_spans(at(0x500000), at(0x600000), at(0x700000), 2, 64, 4096, -1, 18);
        CHECK(neg.c.bad);
        // the largest sizes the entry points accept do not overflow
        const ItemSpans mx = item_spans(at(0x1000), at(0x2000), at(0x3000), 4, INT32_MAX, 4096, INT32_MAX, 34);
        CHECK(!mx.a.bad && !mx.b.bad && !mx.c.bad);
    }
    {  // strided C (ldc > N): ONE conservative span ((M-1) * ldc + N) * 4 that covers the gaps
        const ItemSpans e = item(A, B, C, 4, 64, 4096, 1000);
        CHECK(e.c.hi - e.c.lo == (3 * 1000 + 64) * 4);
        CHECK(!independent(e, item(0x500000, 0x600000, C + 64 * 4)));          // in the gap after row 0: conservative
        CHECK(!independent(e, item(0x500000, 0x600000, C + (3 * 1000 + 63) * 4)));  // the last element
        CHECK(independent(e, item(0x500000, 0x600000, C + (3 * 1000 + 64) * 4)));   // right after it
        CHECK(!independent(e, item(C + 2000 * 4, 0x600000, 0x700000)));        // reads inside the strided rows
        // M = 1: ldc does not matter
        CHECK(item(A, B, C, 1, 64, 4096, 1 << 20).c.hi - C == CSZ);
    }
    {  // groups: every earlier item is tested; the 64-item limit
        const uintptr_t B = 0x10000000;  // 64 weight matrices of 0x40000 B clear of the outputs at C
        Group g;
        for (int i = 0; i < MAX_ITEMS; ++i) {
            CHECK(g.count == i);
            CHECK(join(g, item(A, B + (uintptr_t)i * 0x40000, C + (uintptr_t)i * 0x1000)));
        }
        CHECK(g.count == MAX_ITEMS);
        const ItemSpans next = item(A, B + 64 * (uintptr_t)0x40000, C + 64 * (uintptr_t)0x1000);
        CHECK(independent(g.it[0], next));
        CHECK(!can_join(g, next) && !join(g, next) && g.count == MAX_ITEMS);  // full
        Group h;
        CHECK(join(h, item(A, B, C)) && join(h, item(A, B + 0x40000, C + 0x1000)) && join(h, item(A, B, C + 0x2000)));
        CHECK(!join(h, item(A, B, C + 0x1000)) && h.count == 3);        // collides with the SECOND item only
        CHECK(!join(h, item(C + 0x2000, B, C + 0x3000)) && h.count == 3);  // reads the THIRD item's output
        CHECK(join(h, item(A, B, C + 0x3000)) && h.count == 4);
    }
    if (failures) {
        printf("%d check(s) failed\n", failures);
        return 1;
    }
    printf("capture_fuse_host_test: ok\n");
    return 0;
}
