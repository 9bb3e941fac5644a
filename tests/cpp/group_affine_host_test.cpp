// Host test of csrc/qg_group_affine.hpp (built by tests/test_group_affine_host.py under ASan + UBSan): which
// grouped launches are strided batches, and with which strides. The pointers are plain integers here; the
// header never dereferences them.
#include <stdint.h>
#include <stdio.h>

#include <initializer_list>

#include "qg_group_affine.hpp"

using namespace qg::affine;

struct Item {  // the fields of GemvItemDesc (qg_kernels.hpp)
    const void* A;
    const void* B;
    float* C;
    int N, ldc;
};

static int g_fail = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            ++g_fail;                                             \
        }                                                         \
    } while (0)

static const void* P(uintptr_t v) { return reinterpret_cast<const void*>(v); }
static float* PF(uintptr_t v) { return reinterpret_cast<float*>(v); }

// count items from the bases with the byte strides (two's-complement pointer arithmetic)
static void fill(Item* it, int count, uintptr_t a, uintptr_t b, uintptr_t c, intptr_t sa, intptr_t sb, intptr_t sc,
                 int N = 4096, int ldc = 4096) {
    for (int i = 0; i < count; ++i)
        it[i] = Item{P(a + (uintptr_t)i * (uintptr_t)sa), P(b + (uintptr_t)i * (uintptr_t)sb),
                     PF(c + (uintptr_t)i * (uintptr_t)sc), N, ldc};
}

static bool aff(const Item* it, int count, Strides* s) { return group_affine(it, count, 3, 15, s); }

int main() {
    static Item it[64];
    const uintptr_t A0 = 0x7f0000001000u, B0 = 0x7f1000000000u, C0 = 0x7f2000000000u;
    const int counts[] = {1, 2, 3, 64};

    // ascending, descending and zero strides, shared A, for every count
    for (int n : counts) {
        Strides s = {-1, -1, -1};
        fill(it, n, A0, B0, C0, 4608, 9437184, 16384);
        CHECK(aff(it, n, &s));
        if (n > 1) CHECK(s.a == 4608 && s.b == 9437184 && s.c == 16384);
        else CHECK(s.a == 0 && s.b == 0 && s.c == 0);

        fill(it, n, A0 + 64 * 4608, B0 + 64 * (uintptr_t)9437184, C0 + 64 * 16384, -4608, -9437184, -16384);
        CHECK(aff(it, n, &s));
        if (n > 1) CHECK(s.a == -4608 && s.b == -9437184 && s.c == -16384);

        fill(it, n, A0, B0, C0, 0, 0, 0);  // every item the same product (degenerate, still affine)
        CHECK(aff(it, n, &s));
        CHECK(s.a == 0 && s.b == 0 && s.c == 0);

        fill(it, n, A0, B0, C0, 0, 9437184, 16384);  // shared A
        CHECK(aff(it, n, &s));
        if (n > 1) CHECK(s.a == 0 && s.b == 9437184 && s.c == 16384);

        fill(it, n, A0, B0, C0, 4608, 0, -16384);  // one weight matrix, per-item activations, C from the top down
        CHECK(aff(it, n, &s));
        if (n > 1) CHECK(s.a == 4608 && s.b == 0 && s.c == -16384);
    }

    // one item off by 4 bytes in A, in B, in C (first, middle and last position): not affine, s untouched
    for (int n : {3, 64}) {
        for (int pos : {1, n / 2, n - 1}) {
            for (int f = 0; f < 3; ++f) {
                Strides s = {7, 7, 7};
                fill(it, n, A0, B0, C0, 4608, 9437184, 16384);
                if (f == 0) it[pos].A = P((uintptr_t)it[pos].A + 4);
                if (f == 1) it[pos].B = P((uintptr_t)it[pos].B + 4);
                if (f == 2) it[pos].C = PF((uintptr_t)it[pos].C + 4);
                CHECK(!aff(it, n, &s));
                CHECK(s.a == 7 && s.b == 7 && s.c == 7);
            }
        }
    }
    // two items are always a progression; with a 4-byte offset the stride is what fails (B: not 16-aligned)
    {
        Strides s;
        fill(it, 2, A0, B0, C0, 4608, 9437184, 16384);
        it[1].B = P((uintptr_t)it[1].B + 4);
        CHECK(!aff(it, 2, &s));
        fill(it, 2, A0, B0, C0, 4608, 9437184, 16384);
        it[1].A = P((uintptr_t)it[1].A + 4);
        CHECK(aff(it, 2, &s) && s.a == 4612);
    }

    // unequal N or ldc
    for (int n : {2, 3, 64}) {
        Strides s;
        fill(it, n, A0, B0, C0, 0, 9437184, 16384);
        it[n - 1].N = 4095;
        CHECK(!aff(it, n, &s));
        fill(it, n, A0, B0, C0, 0, 9437184, 16384);
        it[n - 1].ldc = 8192;
        CHECK(!aff(it, n, &s));
    }

    // misaligned strides: A by 2, B by 8 (a multiple of 4 but not of 16), C by 2; the same going down
    {
        Strides s;
        fill(it, 3, A0, B0, C0, 4610, 9437184, 16384);
        CHECK(!aff(it, 3, &s));
        fill(it, 3, A0, B0, C0, 4608, 9437192, 16384);
        CHECK(!aff(it, 3, &s));
        fill(it, 3, A0, B0, C0, 4608, 9437184, 16386);
        CHECK(!aff(it, 3, &s));
        fill(it, 3, A0 + 0x100000, B0 + 0x10000000, C0 + 0x100000, -4608, -9437192, -16384);
        CHECK(!aff(it, 3, &s));
        // the masks are the caller's: with the kernel's own 4-byte rule the 8-byte B stride passes
        fill(it, 3, A0, B0, C0, 4608, 9437192, 16384);
        CHECK(group_affine(it, 3, 3, 3, &s) && s.b == 9437192);
    }

    // differences that do not fit intptr_t: between neighbours, and from the first to the last item
    {
        Strides s;
        it[0] = Item{P(0x10), P(B0), PF(C0), 64, 64};
        it[1] = Item{P(UINTPTR_MAX - 0xF), P(B0 + 16), PF(C0 + 256), 64, 64};  // A: +(2^64 - 0x20)
        CHECK(!aff(it, 2, &s));
        it[0].A = P(UINTPTR_MAX - 0xF);
        it[1].A = P(0x10);  // A: -(2^64 - 0x20)
        CHECK(!aff(it, 2, &s));
        it[0].A = P(0);
        it[1].A = P((uintptr_t)1 << 63);  // exactly 2^63: one past INTPTR_MAX
        CHECK(!aff(it, 2, &s));
        it[0].A = P((uintptr_t)1 << 63);
        it[1].A = P(0);  // exactly -2^63: INTPTR_MIN is refused as well
        CHECK(!aff(it, 2, &s));
        it[0].A = P(0);
        it[1].A = P(((uintptr_t)1 << 63) - 4);  // the largest aligned stride that fits
        CHECK(aff(it, 2, &s) && s.a == INTPTR_MAX - 3);
        // neighbours fit, first-to-last does not: stride 2^62 over 3 items spans 2^63
        const uintptr_t big = (uintptr_t)1 << 62;
        for (int i = 0; i < 3; ++i) it[i] = Item{P(A0), P(16 + (uintptr_t)i * big), PF(C0 + 256u * (uintptr_t)i), 64, 64};
        CHECK(!aff(it, 3, &s));
        for (int i = 0; i < 2; ++i) it[i] = Item{P(A0), P(16 + (uintptr_t)i * big), PF(C0 + 256u * (uintptr_t)i), 64, 64};
        CHECK(aff(it, 2, &s) && s.b == (intptr_t)big);
    }

    // no items
    {
        Strides s;
        CHECK(!aff(it, 0, &s));
        CHECK(!aff(nullptr, 2, &s));
    }

    if (g_fail) {
        printf("group_affine_host_test: %d failure(s)\n", g_fail);
        return 1;
    }
    printf("group_affine_host_test: ok\n");
    return 0;
}
