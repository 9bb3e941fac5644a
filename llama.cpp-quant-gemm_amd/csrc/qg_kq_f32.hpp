// qg_kq_f32.hpp — what the C-ABI (qg_api.hip) and the kernel (qg_kq_f32.hip) of the K-quant decode GEMV on FP32 rows
// (qg_gemm_w4a8_f32_kq) share: one launch that quantizes the M rows to Q8_1 in its prologue and multiplies.
#pragma once
#include "qg_kernels.hpp"
#include "qg_types.hpp"

namespace qg {

struct KqF32Args {
    const float* X;  // [M][K], rows dense, 16-B aligned
    const void* B;   // Q4_K or Q6_K blocks [N][K/256]
    float* C;        // [M][N]
    int M, N, K, wtype;
};

// The dynamic LDS of a launch: the single call's records of the M rows.
constexpr size_t kq_f32_lds_bytes(int M, int K, int wtype) { return (size_t)M * kq_row_lds_bytes(wtype, K); }

// wtype Q4_K or Q6_K, 1 <= M <= 8, N >= 1, K a positive multiple of 256, kq_f32_lds_bytes <= MAX_LDS_BYTES.
// describe: name the kernel there (qg_f32_kq_config) and launch nothing.
hipError_t launch_kq_f32(const KqF32Args& a, hipStream_t st, char* describe = nullptr, size_t describe_len = 0);

}  // namespace qg
