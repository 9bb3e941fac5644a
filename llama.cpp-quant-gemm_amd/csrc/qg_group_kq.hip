// qg_group_kq.hip — the grouped K-quant decode GEMV (qg_gemm_w4a8_grouped_kq), family "gemvg:kq".
//
// One launch computes up to GEMV_GROUP_MAX independent products C_i = A_i . B_i^T (M <= 8 activation rows, one K) whose
// weights are Q4_K or Q6_K item by item: the Q / K / V or gate / up projections of a dense Q4_K_M / Q4_K_S layer, where
// Q and K are Q4_K and V is Q6_K in half the layers. blockIdx.y is the item, blockIdx.x its row tile in the single
// call's XCD order; a workgroup past its item's rows leaves at once (grid.x is the largest item's tile count) unless
// every item fills the grid (GEMVG_FULL).
//
// Work split and data movement are the single call's (qg_q4k_gemv.hip, qg_q6k_gemv.hip): the workgroup stages the M
// activation rows into LDS records, LPR lanes share a weight row and stride over its K / 64 units, the next unit in
// flight while the current one computes, DPP reduction in a fixed order. The bodies are the same texts
// (qg_q4k_gemv_body.inc, qg_q6k_gemv_body.inc) at the single call's (MT, LPR, WGS, ONE) — kq_gemv_form and the M ladder
// of kq_gemv_launch_m — so every item's outputs are the bits of qg_gemm_w4a8 on that item.
//
// The front end is gemvg_kernel's (qg_gemv_kernel.hpp; profiles/group_front/README.md): M, K, the flags and n_first are
// leading scalars, preloaded into SGPRs by the dispatch; the item's 32-B record (GemvItemDesc, the table by value) is
// the kernel's first instruction, ONE 8-dword scalar load, and the only scalar-memory round trip ahead of the weight
// stream. The flags word carries the tile count of an XCD-ordered grid (flags >> GKQ_TILES_SHIFT), so the hidden
// gridDim.x is not fetched either.
//
// The type never costs a load: the host writes the table sorted by type, Q4_K items first (the caller's order within a
// type), and passes their number as n_first. An item's type is `blockIdx.y < n_first`, one scalar compare of two
// registers the workgroup is born with. A type field in the record would have sat behind the record's load and in
// front of the branch that picks the body's first address computation.
//
// Three type forms (TY), so that a homogeneous group pays nothing for the mix: q4k and q6k hold one body each and
// ignore n_first; mix holds both behind the uniform branch. Its registers are the larger body's plus what the front
// end keeps live (profiles/group_kq/resource_usage.txt), its LDS Q4_K's records, the larger ones.
#include "qg_group_kq.hpp"

#include "qg_gemv_kernel.hpp"
#include "qg_kq_launch.hpp"
#include "qg_q4k.hpp"
#include "qg_q6k.hpp"

namespace qg {

// The shipped Q4_K / Q6_K decode GEMV bodies with M a run-time value and the item's own N and output row stride: the row
// tile a parameter, no sumi hook, the very text q4k_gemv_kernel / q6k_gemv_kernel include.
#define QG_KQ_DECLARE_TILE  // tile is a parameter here
#define QG_KQ_ABLK(g) A + (long)g * 9
#define QG_KQ_OUT(m) C[m * ldc + row]
template <int MT, int LPR, int WGS, bool ONE>
__device__ __forceinline__ void q4k_group_body(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B, int M, int N,
                                               int K, void* __restrict__ out, const long ldc, const int tile) {
    constexpr bool SUMI = false;
#include "qg_q4k_gemv_body.inc"
}

template <int MT, int LPR, int WGS, bool ONE>
__device__ __forceinline__ void q6k_group_body(const uint32_t* __restrict__ A, const uint8_t* __restrict__ B, int M, int N,
                                               int K, void* __restrict__ out, const long ldc, const int tile) {
    constexpr bool SUMI = false;
#include "qg_q6k_gemv_body.inc"
}
#undef QG_KQ_OUT
#undef QG_KQ_ABLK
#undef QG_KQ_DECLARE_TILE

namespace {

enum : int { GKQ_Q4K = 0, GKQ_Q6K = 1, GKQ_MIX = 2 };  // TY
constexpr const char* GKQ_NAME[] = {"q4k", "q6k", "mix"};
// the flags word: GEMVG_FULL, GEMVG_XCD (qg_kernels.hpp) and, with GEMVG_XCD, grid.x (<= 512) above them
constexpr int GKQ_TILES_SHIFT = 8;

template <int TY, int MT, int LPR, int WGS, bool ONE>
__global__ __launch_bounds__(WGS) void kq_group_kernel(int M, int K, int flags, int n_first, const GemvItems items) {
    constexpr int RPB = (WGS / 64) * (64 / LPR);  // rows per workgroup
    static_assert(sizeof(GemvItemDesc) == 32 && offsetof(GemvItemDesc, N) == 24 && offsetof(GemvItemDesc, ldc) == 28, "");
    const u32x8_a16 r = *reinterpret_cast<const u32x8_a16*>(&items.it[blockIdx.y]);
    const uint32_t* A = global_ptr<const uint32_t>(r[0], r[1]);
    const uint8_t* B = global_ptr<const uint8_t>(r[2], r[3]);
    float* C = global_ptr<float>(r[4], r[5]);
    const int N = (int)r[6];
    const long ldc = (int)r[7];
    // the single call's XCD-aware tile order within the item
    const int tile = (flags & GEMVG_XCD) ? xcd_tile(blockIdx.x, flags >> GKQ_TILES_SHIFT) : (int)blockIdx.x;
    if (!(flags & GEMVG_FULL) && tile * RPB >= N) return;  // past this item's rows (uniform)
    if constexpr (TY == GKQ_Q4K) {
        q4k_group_body<MT, LPR, WGS, ONE>(A, B, M, N, K, C, ldc, tile);
    } else if constexpr (TY == GKQ_Q6K) {
        q6k_group_body<MT, LPR, WGS, ONE>(A, B, M, N, K, C, ldc, tile);
    } else {
        // the table is sorted: Q4_K items first (uniform over the workgroup, two preloaded SGPRs)
        if ((int)blockIdx.y < n_first) q4k_group_body<MT, LPR, WGS, ONE>(A, B, M, N, K, C, ldc, tile);
        else q6k_group_body<MT, LPR, WGS, ONE>(A, B, M, N, K, C, ldc, tile);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------
struct GroupKqLaunch {
    const GemvGroup& grp;
    int n_q4k;
    hipStream_t st;
    char* describe;
    size_t describe_len;
};

template <int TY, int MT> hipError_t group_kq_form(const GroupKqLaunch& L) {
    const GemvGroup& grp = L.grp;
    // (LPR, WGS, ONE) of the single call: both types have K / 64 units per row
    return kq_gemv_form(grp.K, [&](auto lpr, auto wgs, auto one) -> hipError_t {
        constexpr int LPR = lpr, WGS = wgs, RPB = (WGS / 64) * (64 / LPR);
        const size_t lds = group_kq_lds_bytes(grp.M, grp.K, L.n_q4k);
        int tiles = 0, full = 1;
        for (int i = 0; i < grp.count; ++i) tiles = std::max(tiles, (grp.it[i].N + RPB - 1) / RPB);
        for (int i = 0; i < grp.count; ++i) full = full && (grp.it[i].N + RPB - 1) / RPB == tiles;
        const int xcd = tiles <= 512;  // one dispatch round, as the single call
        const int flags = (full ? GEMVG_FULL : 0) | (xcd ? GEMVG_XCD | (tiles << GKQ_TILES_SHIFT) : 0);
        if (L.describe) {
            describe_line(L.describe, L.describe_len, "gemvg:kq T=%s MT=%d LPR=%d WGS=%d ONE=%d grid=%dx%d lds=%zu", GKQ_NAME[TY], MT,
                          LPR, WGS, (int)one, tiles, grp.count, lds);
            return hipSuccess;
        }
        auto k = kq_group_kernel<TY, MT, LPR, WGS, one>;
        static std::atomic<unsigned long long> done;
        const hipError_t e = lds_opt_in((const void*)k, lds, done);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k, dim3(tiles, grp.count), dim3(WGS), lds, L.st, grp.M, grp.K, flags, L.n_q4k,
                           *reinterpret_cast<const GemvItems*>(grp.it));
        return hipGetLastError();
    });
}

// MT from M, as kq_gemv_launch_m picks it
template <int TY> hipError_t group_kq_m(const GroupKqLaunch& L) {
    if (L.grp.M <= 1) return group_kq_form<TY, 1>(L);
    if (L.grp.M <= 2) return group_kq_form<TY, 2>(L);
    if (L.grp.M <= 4) return group_kq_form<TY, 4>(L);
    return group_kq_form<TY, 8>(L);
}

}  // namespace

hipError_t launch_group_kq(const GemvGroup& grp, int n_q4k, hipStream_t st, char* describe, size_t describe_len) {
    if (grp.count < 1 || grp.count > GEMV_GROUP_MAX || grp.M < 1 || grp.M > 8 || n_q4k < 0 || n_q4k > grp.count)
        return hipErrorInvalidValue;
    const GroupKqLaunch L{grp, n_q4k, st, describe, describe_len};
    if (n_q4k == grp.count) return group_kq_m<GKQ_Q4K>(L);
    if (n_q4k == 0) return group_kq_m<GKQ_Q6K>(L);
    return group_kq_m<GKQ_MIX>(L);
}

}  // namespace qg
