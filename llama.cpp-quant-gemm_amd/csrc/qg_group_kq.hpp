// qg_group_kq.hpp — what the C-ABI (qg_api.hip) and the kernel (qg_group_kq.hip) of the grouped K-quant decode GEMV
// (qg_gemm_w4a8_grouped_kq) share: one launch of up to GEMV_GROUP_MAX independent Q4_K / Q6_K products.
#pragma once
#include "qg_kernels.hpp"
#include "qg_types.hpp"

namespace qg {

// The dynamic LDS of a launch of M activation rows: the records of the largest record type present, Q4_K's 84 dwords
// per (token, super-block) where a Q4_K item is present (n_q4k > 0), else Q6_K's.
constexpr size_t group_kq_lds_bytes(int M, int K, int n_q4k) {
    return (size_t)M * kq_row_lds_bytes(n_q4k > 0 ? QG_TYPE_Q4_K : QG_TYPE_Q6_K, K);
}

// One launch over grp.it[0 .. grp.count): the first n_q4k items are Q4_K, the rest Q6_K (the caller has sorted the
// table), 1 <= grp.count <= GEMV_GROUP_MAX, 1 <= grp.M <= 8, every N >= 1, group_kq_lds_bytes <= MAX_LDS_BYTES.
// describe: name the kernel there (qg_group_kq_config) and launch nothing.
hipError_t launch_group_kq(const GemvGroup& grp, int n_q4k, hipStream_t st, char* describe = nullptr, size_t describe_len = 0);

}  // namespace qg
