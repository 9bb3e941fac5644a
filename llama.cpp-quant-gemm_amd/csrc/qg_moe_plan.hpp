// qg_moe_plan.hpp — the plan of the two expert-grouped mul_mat_id entries (qg_gemm_w4a8_moe_prefill: qg_moe_prefill.hip,
// qg_gemm_w4a8_moe_batch: qg_moe_batch.hip): its limits, the layout of the caller's workspace, the kernel argument, the
// plan launch (qg_moe_plan.hip) and the tile lookup of the product kernels. What the C-ABI (qg_api.hip) and those three
// files share. A header of its own: the translation units that shipped before it do not see it.
#pragma once
#include <stddef.h>

#include "qg_kernels.hpp"

namespace qg {

// Bound on n_expert: the plan keeps three int32 tables of n_expert + 2 entries in LDS (qg_moe_plan.hip).
constexpr int MOE_MAX_EXPERTS = 4096;
constexpr int MOE_MAX_SLOTS = 65535;
constexpr size_t MOE_WS_ALIGN = 16;  // the tile records are read as one 16-B load

// An upper bound on the tiles of R rows that `slots` slots in n_expert + 1 bins (the last: ids that name no expert)
// can need: sum_b ceil(c_b / R) <= floor(slots / R) + (bins that are not empty). gridDim.y of the product launch.
__host__ __device__ inline long moe_max_tiles(long slots, long n_expert, int R) {
    return slots / R + (n_expert + 1 < slots ? n_expert + 1 : slots);
}

// The workspace, in int32 units from its base. Everything the product kernels read the plan kernel of the same
// call has written; nothing is read that was there before.
//   [0]                 n_tiles, [1] slots with a valid id, [2] R, [3] 0
//   counts              n_expert + 1 slot counts, the last the invalid bin
//   sorted              the slots in bin order (the invalid bin's last), `slots` entries
//   rows                the activation row t * a_rows + u % a_rows of each sorted slot
//   tiles               {bin, first sorted position, rows, 0} per tile, sized for the smallest tile of the entry
//                       (min_r: MOE_PREFILL_MIN_R, MOE_BATCH_MIN_R). The region is the last, so every offset is the
//                       same for both and the kernels need no min_r.
struct MoePlanLayout {
    long counts, sorted, rows, tiles, total;
};
__host__ __device__ inline MoePlanLayout moe_plan_layout(long slots, long n_expert, int min_r = 16) {
    MoePlanLayout L;
    L.counts = 4;
    L.sorted = L.counts + ((n_expert + 1 + 3) & ~3L);
    L.rows = L.sorted + ((slots + 3) & ~3L);
    L.tiles = L.rows + ((slots + 3) & ~3L);
    L.total = L.tiles + 4 * moe_max_tiles(slots, n_expert, min_r);
    return L;
}

// Passed by value as the kernel argument of the plan and of the products: its layout is the kernarg layout.
struct MoePlanArgs {
    const void* A;       // block_q8_1 [T][a_rows][K/32]
    const void* B;       // n_expert matrices [N][K/256], estride bytes apart
    const int32_t* ids;  // device memory
    float* C;
    int32_t* ws;         // MoePlanLayout
    long ids_stride, ldc, estride;  // elements, floats, bytes
    int a_rows, n_used, n_expert, N, K, slots;
};
static_assert(sizeof(MoePlanArgs) == 88 && offsetof(MoePlanArgs, ws) == 32 && offsetof(MoePlanArgs, ids_stride) == 40 &&
                  offsetof(MoePlanArgs, estride) == 56 && offsetof(MoePlanArgs, a_rows) == 64 &&
                  offsetof(MoePlanArgs, slots) == 84,
              "the kernarg layout");

// The kernel argument of the two biased entries (qg_gemm_w4a8_moe_prefill_bias, _moe_batch_bias): the plan's, which
// the plan launch and the tile lookup take as it is, then the bias. The shipped kernels keep MoePlanArgs.
struct MoeBiasArgs : MoePlanArgs {
    const float* bias;  // [n_expert] rows of N floats, bias_stride floats apart; null: no addition (the BIAS = false kernels)
    long bias_stride;
};

// C[s][n] += bias[ids[s]][n] for every slot with a valid id, one launch (qg_moe_prefill.hip): the bias of the Q4_K / Q6_K
// products in the two biased entries, whose product kernels are the unbiased entries'.
hipError_t launch_moe_bias_add(const MoeBiasArgs& a, hipStream_t st);

// The plan alone for tiles of 1 << rsh rows (rsh = 1 .. 6), one launch; the workspace's tile region holds
// moe_max_tiles at that size.
hipError_t launch_moe_plan_rows(const MoePlanArgs& a, int rsh, hipStream_t st);

// The tile of a product workgroup, blockIdx.y. false: blockIdx.y is beyond n_tiles.
struct MoeTile {
    int e, first, rows;        // bin, first sorted position, rows
    const int32_t* sorted;     // + first: the tile's slots
    const int32_t* arows;      // + first: their activation rows
};
__device__ __forceinline__ bool moe_tile_lookup(const MoePlanArgs& a, MoeTile& t) {
    const int32_t* __restrict__ ws = a.ws;
    const MoePlanLayout L = moe_plan_layout(a.slots, a.n_expert);  // (the offsets do not depend on the tile size)
    // both loads at once (the record's place is inside the workspace for every blockIdx.y of the grid, whatever it
    // holds beyond n_tiles): one round trip to memory before the workgroup knows its work, not two
    const int n_tiles = ws[0];
    const int4 rec = reinterpret_cast<const int4*>(ws + L.tiles)[blockIdx.y];
    if ((int)blockIdx.y >= __builtin_amdgcn_readfirstlane(n_tiles)) return false;
    t.e = __builtin_amdgcn_readfirstlane(rec.x);
    t.first = __builtin_amdgcn_readfirstlane(rec.y);
    t.rows = __builtin_amdgcn_readfirstlane(rec.z);
    t.sorted = ws + L.sorted + t.first;
    t.arows = ws + L.rows + t.first;
    return true;
}

}  // namespace qg
