// qg_group_affine.hpp — is a grouped GEMV launch a strided batch? (gemv_pick, qg_gemv_kernel.hpp)
//
// A group (GemvGroup, qg_kernels.hpp) is AFFINE when its items share N and ldc and their A, B and C pointers
// each advance by one constant byte stride from item to item: item i = item 0 + i * stride. Such a group is
// exactly what qg_gemm_w4a8_strided_batched describes, so it runs the strided-batch kernel (all arguments in
// SGPRs, no descriptor load in front of the weight stream) instead of gemvg_kernel. Strides may be zero
// (shared activations, or one weight matrix for every item) or negative (items listed from the top down).
// The strides must keep the batch form's alignment: a_mask / b_mask are the low bits that must be zero in
// the A and B strides (gemv_shape_ok and the batch entry: 3 and 15); the C stride is whole floats.
//
// Pure host code, no HIP includes: tests/cpp/group_affine_host_test.cpp builds it with a plain C++ compiler
// under sanitizers. Arithmetic on the pointers' integer values, differences formed without wrap-around: a
// difference (between neighbours, or from the first to the last item) that does not fit intptr_t means "not
// affine".
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace qg {
namespace affine {

struct Strides {
    intptr_t a, b, c;  // bytes from item i to item i + 1
};

// q - p as a signed value; false: it does not fit (INTPTR_MIN is refused too, so -d is always safe)
inline bool ptr_diff(const void* q, const void* p, intptr_t* d) {
    const uintptr_t uq = (uintptr_t)q, up = (uintptr_t)p;
    if (uq >= up) {
        if (uq - up > (uintptr_t)INTPTR_MAX) return false;
        *d = (intptr_t)(uq - up);
    } else {
        if (up - uq > (uintptr_t)INTPTR_MAX) return false;
        *d = -(intptr_t)(up - uq);
    }
    return true;
}

// Item: any struct with A, B, C (pointers), N and ldc (GemvItemDesc). count >= 1; a single item is affine
// with zero strides. *s is written only when the answer is true.
template <class Item>
inline bool group_affine(const Item* it, int count, uintptr_t a_mask, uintptr_t b_mask, Strides* s) {
    if (!it || count < 1) return false;
    Strides st = {0, 0, 0};
    if (count > 1 && !(ptr_diff(it[1].A, it[0].A, &st.a) && ptr_diff(it[1].B, it[0].B, &st.b) &&
                       ptr_diff(it[1].C, it[0].C, &st.c)))
        return false;
    // the sign bit takes part: the low bits of a negative stride are those of its two's complement, which is
    // what the kernel's address arithmetic adds
    if (((uintptr_t)st.a & a_mask) != 0 || ((uintptr_t)st.b & b_mask) != 0 || ((uintptr_t)st.c & 3) != 0) return false;
    for (int i = 1; i < count; ++i) {
        if (it[i].N != it[0].N || it[i].ldc != it[0].ldc) return false;
        intptr_t da, db, dc;
        if (!(ptr_diff(it[i].A, it[i - 1].A, &da) && ptr_diff(it[i].B, it[i - 1].B, &db) &&
              ptr_diff(it[i].C, it[i - 1].C, &dc)))
            return false;
        if (da != st.a || db != st.b || dc != st.c) return false;
    }
    // (count - 1) * stride, which the kernel forms, is last - first: it must fit as well
    intptr_t t;
    if (!(ptr_diff(it[count - 1].A, it[0].A, &t) && ptr_diff(it[count - 1].B, it[0].B, &t) &&
          ptr_diff(it[count - 1].C, it[0].C, &t)))
        return false;
    *s = st;
    return true;
}

}  // namespace affine
}  // namespace qg
