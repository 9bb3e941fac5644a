// qg_moe_glu_prefill.hpp — what the C-ABI (qg_api.hip) and the kernels (qg_moe_glu_prefill.hip) of the expert-grouped
// MFMA gate / up product with its GLU (qg_gemm_w4a8_moe_glu_prefill) share. The plan, its workspace and its limits are
// the prefill entry's (qg_moe_plan.hpp, qg_moe_prefill.hpp).
#pragma once
#include "qg_moe_prefill.hpp"

namespace qg {

// The kernel argument: the plan's, which the plan launch and the tile lookup take as it is (B is B_gate, a_rows is 1),
// then the up experts and the op. MoePlanArgs keeps its layout.
struct MoeGluPrefillArgs : MoePlanArgs {
    const void* B_up;  // the shape and type of B; may be B
    int glu_op;        // QG_GLU_REGLU / QG_GLU_SWIGLU
};

// The plan and the fused product (two launches); describe: name them there (qg_moe_glu_prefill_config) and launch
// nothing. The caller has checked the type (Q4_K / Q6_K), glu_op, the bounds of the plan and the workspace.
hipError_t launch_moe_glu_prefill(const MoeGluPrefillArgs& a, int wtype, hipStream_t st, char* describe = nullptr,
                                  size_t describe_len = 0);

}  // namespace qg
