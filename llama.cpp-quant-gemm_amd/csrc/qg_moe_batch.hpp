// qg_moe_batch.hpp — what the C-ABI (qg_api.hip) and the kernels (qg_moe_batch.hip) of the expert-grouped decode GEMV
// (qg_gemm_w4a8_moe_batch, qg_gemm_w4a8_moe_batch_bias) share; the plan, its workspace and the kernel argument are qg_moe_plan.hpp's.
#pragma once
#include "qg_moe_plan.hpp"

namespace qg {

constexpr int MOE_BATCH_MIN_R = 2;  // the smallest tile the entry plans: what its workspace is sized for
constexpr size_t MOE_BATCH_LDS_MAX = 160 * 1024;

// Bytes of the LDS records of one gathered row of K elements (Q4_K, Q6_K: a record per super-block; MXFP4: per block).
size_t moe_batch_row_lds(int K, int wtype);
// Rows per tile, R = 2, 4 or 8, from (slots, n_expert, K, type) alone; 0: the records of two rows do not fit the LDS.
int moe_batch_rows(long slots, int n_expert, int K, int wtype);
// The plan and the GEMV (two launches); describe: name them there (qg_moe_batch_config) and launch nothing.
// The caller has checked the type (Q4_K / Q6_K), the bounds of the plan, moe_batch_rows != 0 and the workspace.
hipError_t launch_moe_batch(const MoePlanArgs& a, int wtype, hipStream_t st, char* describe = nullptr,
                            size_t describe_len = 0);
// qg_gemm_w4a8_moe_batch_bias: the same two launches with the per-expert bias added to the finished product, for Q4_K /
// Q6_K / MXFP4 (family "moeb:mxfp4_gemv"). Q4_K / Q6_K with a null bias: launch_moe_batch's launch itself.
hipError_t launch_moe_batch_bias(const MoeBiasArgs& a, int wtype, hipStream_t st, char* describe = nullptr,
                                 size_t describe_len = 0);

}  // namespace qg
