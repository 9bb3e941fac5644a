// qg_moe_prefill.hpp — what the C-ABI (qg_api.hip) and the kernels (qg_moe_prefill.hip) of the expert-grouped MFMA
// prefill (qg_gemm_w4a8_moe_prefill) share; the plan, its workspace and the kernel argument are qg_moe_plan.hpp's.
#pragma once
#include "qg_moe_plan.hpp"

namespace qg {

constexpr int MOE_PREFILL_MIN_R = 16;  // the smallest tile the entry plans: what its workspace is sized for

// The plan alone for tiles of 16 * tt rows (tt = 1, 2 or 4), one launch.
hipError_t launch_moe_plan(const MoePlanArgs& a, int tt, hipStream_t st);
// The plan and the product (two launches); describe: name them there (qg_moe_prefill_config) and launch nothing.
// The caller has checked the type (Q4_K / Q6_K), the bounds of the plan and the workspace.
hipError_t launch_moe_prefill(const MoePlanArgs& a, int wtype, hipStream_t st, char* describe = nullptr,
                              size_t describe_len = 0);
// qg_gemm_w4a8_moe_prefill_bias: the same two launches with the per-expert bias added to the finished product, for Q4_K /
// Q6_K / MXFP4 (family "moe:mxfp4_mmq"). Q4_K / Q6_K with a null bias: launch_moe_prefill's launch itself.
hipError_t launch_moe_prefill_bias(const MoeBiasArgs& a, int wtype, hipStream_t st, char* describe = nullptr,
                                   size_t describe_len = 0);
// tt of the form launch_moe_prefill picks for this shape (qg_debug_moe_prefill_plan runs the plan it would run)
int moe_prefill_tt(const MoePlanArgs& a, int wtype);

}  // namespace qg
