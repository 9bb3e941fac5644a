// qg_moe_glu_batch.hpp — what the C-ABI (qg_api.hip) and the kernels (qg_moe_glu_batch.hip) of the expert-grouped
// decode GEMV gate / up product with its GLU (qg_gemm_w4a8_moe_glu_batch) share. The plan, its workspace, its limits
// and the rows per tile are the batch entry's (qg_moe_plan.hpp, qg_moe_batch.hpp).
#pragma once
#include "qg_moe_batch.hpp"

namespace qg {

// The kernel argument: the plan's, which the plan launch and the tile lookup take as it is (B is B_gate, a_rows is 1),
// then the up experts, the two bias tables and the op. MoePlanArgs keeps its layout.
struct MoeGluBatchArgs : MoePlanArgs {
    const void* B_up;        // the shape and type of B; may be B
    const float* bias_gate;  // device memory [n_expert][bias_stride]; null: no add
    const float* bias_up;
    long bias_stride;        // floats
    int glu_op;              // QG_GLU_REGLU / QG_GLU_SWIGLU / QG_GLU_SWIGLU_OAI
    float alpha, limit;      // QG_GLU_SWIGLU_OAI alone
};

// The plan and the fused product (two launches); describe: name them there (qg_moe_glu_batch_config) and launch
// nothing. wtype Q4_K / Q6_K / MXFP4. The caller has checked the type, glu_op, the bounds of the plan,
// moe_batch_rows != 0 and the workspace.
hipError_t launch_moe_glu_batch(const MoeGluBatchArgs& a, int wtype, hipStream_t st, char* describe = nullptr,
                                size_t describe_len = 0);

}  // namespace qg
