// qg_moe_down.hpp — what the C-ABI (qg_api.hip) and the kernels (qg_moe_down.hip) of the down mul_mat_id with the
// weighted expert sum (qg_gemm_w4a8_moe_down, qg_gemm_w4a8_moe_down_bias) share.
#pragma once
#include "qg_common.hpp"
#include "qg_kernels.hpp"

namespace qg {

// Token t = blockIdx.y reads its n_used expert ids e_u = ids[t * ids_stride + u] on the device, computes d_u, the M = 1
// product of activation row t * n_used + u with expert e_u's matrix, and stores
// sum_u weights[t * w_stride + u] * d_u (ascending u, ids outside [0, n_expert) left out) into C + t * ldc.
// Passed by value as the kernel argument.
struct MoeDownArgs {
    const void* A;         // block_q8_1 [T][n_used][K/32]
    const void* B;         // n_expert matrices [N][K/256], estride bytes apart
    const int32_t* ids;    // device memory
    const float* weights;  // device memory; null: every weight 1.0f
    float* C;              // [T][ldc]
    long ids_stride, w_stride, ldc, estride, arow;  // elements, floats, floats, bytes, bytes of one activation row
    int n_used, n_expert, N, K, T;
};

// The form of the launch for (n_used, K, wtype): the decode GEMV's LPR, WGS and ONE (kq_gemv_form; for MXFP4, which
// only the _bias entry takes, kq_gemv_form_units(K / 32) and a record of MXFP4_REC_DW dwords per block), SW of the
// workgroup's WGS / 64 waves side by side on the slots of one row group (the largest power of two <=
// min(n_used, WGS / 64)), RPB = (WGS / 64 / SW) * (64 / LPR) rows per workgroup, and the dynamic LDS: the n_used
// activation rows' records and the n_used x RPB products. lds is SIZE_MAX where it does not fit a size_t's worth of
// sense (n_used beyond any LDS).
struct MoeDownForm {
    int lpr, wgs, one, sw, rpb;
    size_t lds;
};
MoeDownForm moe_down_form(int n_used, int K, int wtype);

// describe: name the kernel there (qg_moe_down_config) and launch nothing. The caller has checked the type (Q4_K /
// Q6_K), that AUTO at M = 1 takes the decode GEMV of the type, T <= 65535 and moe_down_form(...).lds <= MAX_LDS_BYTES.
hipError_t launch_moe_down(const MoeDownArgs& a, int wtype, hipStream_t st, char* describe = nullptr, size_t describe_len = 0);

// qg_gemm_w4a8_moe_down_bias: the same token with d_u = d_u + bias[e_u * bias_stride + n] ahead of the fold. A kernel
// argument of its own, so that the entry above keeps its argument block.
struct MoeDownBiasArgs : MoeDownArgs {
    const float* bias;  // device memory [n_expert][bias_stride]; null: no add
    long bias_stride;   // floats
};
// wtype Q4_K / Q6_K / MXFP4 (B and estride then any number of bytes). The caller has checked what launch_moe_down's has.
hipError_t launch_moe_down_bias(const MoeDownBiasArgs& a, int wtype, hipStream_t st, char* describe = nullptr,
                                size_t describe_len = 0);

}  // namespace qg
