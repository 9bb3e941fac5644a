// qg_moe_glu.hpp — what the C-ABI (qg_api.hip) and the kernels (qg_moe_glu.hip) of the fused gate / up mul_mat_id
// (qg_gemm_w4a8_moe_glu, qg_gemm_w4a8_moe_glu_bias) share.
#pragma once
#include "qg_common.hpp"
#include "qg_kernels.hpp"

namespace qg {

// Slot s = t * n_used + u of the launch's grid.y reads its expert e = ids[t * ids_stride + u] on the device, computes
// g and u, the M = 1 products of activation row t with expert e of B_gate and of B_up, and stores glu(g) * u into
// C + s * ldc. Passed by value as the kernel argument.
struct MoeGluArgs {
    const void* A;       // block_q8_1 [T][K/32]
    const void* B_gate;  // n_expert matrices [N][K/256], estride bytes apart
    const void* B_up;    // the same shape and type; may be B_gate
    const int32_t* ids;  // device memory
    float* C;
    long ids_stride, ldc, estride, arow;  // elements, floats, bytes, bytes of one activation row
    int n_used, n_expert, N, K, slots, glu_op;
};
// describe: name the kernel there (qg_moe_glu_config) and launch nothing. The caller has checked the type (Q4_K /
// Q6_K), glu_op and that AUTO at M = 1 takes the decode GEMV of the type.
hipError_t launch_moe_glu(const MoeGluArgs& a, int wtype, hipStream_t st, char* describe = nullptr, size_t describe_len = 0);

// qg_gemm_w4a8_moe_glu_bias: the same slot with g = g + bias_gate[e * bias_stride + n], u likewise, ahead of the op,
// and QG_GLU_SWIGLU_OAI among the ops. A kernel argument of its own, so that the entry above keeps its argument block.
struct MoeGluBiasArgs : MoeGluArgs {
    const float* bias_gate;  // device memory [n_expert][bias_stride]; null: no add
    const float* bias_up;
    long bias_stride;        // floats
    float alpha, limit;      // QG_GLU_SWIGLU_OAI alone
};
// wtype Q4_K / Q6_K / MXFP4 (B_gate, B_up and estride then any number of bytes). The caller has checked what
// launch_moe_glu's has, glu_op among the three.
hipError_t launch_moe_glu_bias(const MoeGluBiasArgs& a, int wtype, hipStream_t st, char* describe = nullptr,
                               size_t describe_len = 0);

}  // namespace qg
