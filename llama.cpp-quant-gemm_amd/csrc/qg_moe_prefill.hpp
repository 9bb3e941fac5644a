// qg_moe_prefill.hpp — what the C-ABI (qg_api.hip) and the kernels (qg_moe_prefill.hip) of the expert-grouped MFMA
// prefill (qg_gemm_w4a8_moe_prefill) share: the kernel argument and the layout of the caller's workspace.
// A header of its own: the translation units that shipped before it do not see it.
#pragma once
#include "qg_kernels.hpp"

namespace qg {

// Bound on n_expert: the plan keeps three int32 tables of n_expert + 2 entries in LDS (qg_moe_prefill.hip).
constexpr int MOE_PREFILL_MAX_EXPERTS = 4096;
constexpr int MOE_PREFILL_MAX_SLOTS = 65535;
constexpr size_t MOE_PREFILL_WS_ALIGN = 16;  // the tile records are read as one 16-B load

// An upper bound on the tiles of R rows that `slots` slots in n_expert + 1 bins (the last: ids that name no expert)
// can need: sum_b ceil(c_b / R) <= floor(slots / R) + (bins that are not empty). gridDim.y of the product launch.
__host__ __device__ inline long moe_prefill_max_tiles(long slots, long n_expert, int R) {
    return slots / R + (n_expert + 1 < slots ? n_expert + 1 : slots);
}

// The workspace, in int32 units from its base. Everything the product kernels read the plan kernel of the same
// call has written; nothing is read that was there before.
//   [0]                 n_tiles, [1] slots with a valid id, [2] R, [3] 0
//   counts              n_expert + 1 slot counts, the last the invalid bin
//   sorted              the slots in bin order (the invalid bin's last), `slots` entries
//   rows                the activation row t * a_rows + u % a_rows of each sorted slot
//   tiles               {bin, first sorted position, rows, 0} per tile, sized for the smallest tile of the entry: R = 16
//                       for the prefill, min_r = 2 for the expert-grouped decode GEMV (qg_moe_batch.hpp). The region
//                       is the last, so every offset is the same for both and the plan kernel needs no min_r.
struct MoePlanLayout {
    long counts, sorted, rows, tiles, total;
};
__host__ __device__ inline MoePlanLayout moe_plan_layout(long slots, long n_expert, int min_r = 16) {
    MoePlanLayout L;
    L.counts = 4;
    L.sorted = L.counts + ((n_expert + 1 + 3) & ~3L);
    L.rows = L.sorted + ((slots + 3) & ~3L);
    L.tiles = L.rows + ((slots + 3) & ~3L);
    L.total = L.tiles + 4 * moe_prefill_max_tiles(slots, n_expert, min_r);
    return L;
}

// Passed by value as the kernel argument of the plan and of the product.
struct MoePrefillArgs {
    const void* A;       // block_q8_1 [T][a_rows][K/32]
    const void* B;       // n_expert matrices [N][K/256], estride bytes apart
    const int32_t* ids;  // device memory
    float* C;
    int32_t* ws;         // MoePlanLayout
    long ids_stride, ldc, estride;  // elements, floats, bytes
    int a_rows, n_used, n_expert, N, K, slots;
};

// The plan alone for tiles of 16 * tt rows (tt = 1, 2 or 4), one launch.
hipError_t launch_moe_plan(const MoePrefillArgs& a, int tt, hipStream_t st);
// The plan alone for tiles of 1 << rsh rows (rsh = 1 .. 6); the workspace's tile region holds moe_prefill_max_tiles
// at that size.
hipError_t launch_moe_plan_rows(const MoePrefillArgs& a, int rsh, hipStream_t st);
// The plan and the product (two launches); describe: name them there (qg_moe_prefill_config) and launch nothing.
// The caller has checked the type (Q4_K / Q6_K), the bounds above and the workspace.
hipError_t launch_moe_prefill(const MoePrefillArgs& a, int wtype, hipStream_t st, char* describe = nullptr,
                              size_t describe_len = 0);
// tt of the form launch_moe_prefill picks for this shape (qg_debug_moe_prefill_plan runs the plan it would run)
int moe_prefill_tt(const MoePrefillArgs& a, int wtype);

}  // namespace qg
