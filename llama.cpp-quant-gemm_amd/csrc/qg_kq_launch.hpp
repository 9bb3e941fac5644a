// qg_kq_launch.hpp — the host side the super-block (Q4_K, Q6_K) and the MXFP4 kernels share: instantiation choice,
// launch and eligibility of the decode GEMV (qg_q4k_gemv.hip, qg_q6k_gemv.hip, qg_mxfp4_gemv.hip) and of the MFMA
// prefill (qg_q4k_mmq.hip, qg_q6k_mmq.hip, qg_mxfp4_mmq.hip). The kernels themselves stay one per type (DESIGN.md,
// "Q4_K": what was tried to share them); within a type a kernel's body is one text, qg_<type>_{gemv,mmq}_body.inc,
// which the shipped kernel and its expert-indexed / expert-grouped twins (qg_moe.hip, qg_moe_batch.hip,
// qg_moe_prefill.hip; their plan: qg_moe_plan.hip) all include.
//
// A type's file passes a struct F of constants and static functions:
//   GEMV:  REC_ELEMS and REC_DW (elements and dwords of an LDS record: a token's super-block, or its block for MXFP4;
//          K is a multiple of REC_ELEMS), UNIT (elements of a lane's unit), WMASK (the low bits of the weights pointer
//          that must be 0), kernel<MT, LPR, WGS, SUMI, ONE>() and describe(g, MT, LPR, WGS, one, grid, lds), the
//          qg_debug_config line
//   MMQ:   NAME (the family, for the qg_debug_config line), WAVES, WMASK, KMULT (K is a multiple of it),
//          kernel<TT, RG, SUMI>()
// The expert entries have no F: kq_gemv_form picks their instantiation too, kq_gemv_rec_dw / kq_family name the type.
#pragma once
#include "../../include/qg/qg.h"
#include "qg_common.hpp"
#include "qg_kernels.hpp"
#include "qg_q4k.hpp"
#include "qg_mxfp4.hpp"
#include "qg_q6k.hpp"

namespace qg {

// A super-block type by its id: the decode GEMV's LDS record, the family ("q4k" + "_gemv" / "_mmq" in the config lines).
constexpr int kq_gemv_rec_dw(int wtype) { return wtype == QG_TYPE_Q4_K ? Q4K_REC_DW : Q6K_REC_DW; }
constexpr const char* kq_family(int wtype) { return wtype == QG_TYPE_Q4_K ? "q4k" : "q6k"; }

// ---- decode GEMV (M <= 8) ------------------------------------------------------------------------------------
template <class F> inline size_t kq_gemv_lds_bytes(int M, int K) { return (size_t)M * (K / F::REC_ELEMS) * F::REC_DW * 4; }

// The decode GEMV's instantiation for K, chosen here and nowhere else: fn(LPR, WGS, ONE) as std::integral_constant /
// bool_constant. The single call below and the expert entries (qg_moe{,_glu,_batch}.hip) launch what it hands them.
// Lanes per row: the largest of 4 / 16 / 64 that the row's K / 64 units fill. K >= 4096: a wave per row, 16
// rows per 1024-thread workgroup (256 workgroups at N = 4096, as the row GEMV); K >= 1024: 16 lanes, 32 rows per
// 512-thread workgroup; below: 4 lanes, 64 rows per 256-thread workgroup. ONE: no lane owns a second unit.
// kq_gemv_form_units: the same ladder for a row of U units of any size (MXFP4: U = K / 32, a block per unit).
template <class Fn> auto kq_gemv_form_units(int U, Fn&& fn) {
    auto form = [&](auto lpr, auto wgs) {
        return U <= lpr ? fn(lpr, wgs, std::true_type{}) : fn(lpr, wgs, std::false_type{});
    };
    if (U >= 64) return form(ic<64>{}, ic<1024>{});
    if (U >= 16) return form(ic<16>{}, ic<512>{});
    return form(ic<4>{}, ic<256>{});
}
template <class Fn> auto kq_gemv_form(int K, Fn&& fn) { return kq_gemv_form_units(K / 64, fn); }

template <class F, int MT, bool SUMI> hipError_t kq_gemv_launch_mt(const GemmArgs& g, hipStream_t st) {
    // (units per row, rounded up: only a unit of several MXFP4 blocks can be partial)
    return kq_gemv_form_units((g.K + F::UNIT - 1) / F::UNIT, [&](auto lpr, auto wgs, auto one) -> hipError_t {
        constexpr int LPR = lpr, WGS = wgs, RPB = (WGS / 64) * (64 / LPR);
        const size_t lds = kq_gemv_lds_bytes<F>(g.M, g.K);
        const int grid = (g.N + RPB - 1) / RPB;
        if (g.describe) {
            F::describe(g, MT, LPR, WGS, (int)one, grid, lds);
            return hipSuccess;
        }
        auto k = F::template kernel<MT, LPR, WGS, SUMI, one>();
        static std::atomic<unsigned long long> done;
        const hipError_t e = lds_opt_in((const void*)k, lds, done);
        if (e != hipSuccess) return e;
        void* out = SUMI ? (void*)g.sumi : (void*)g.C;
        hipLaunchKernelGGL(k, dim3(grid), dim3(WGS), lds, st, (const uint32_t*)g.A, (const uint8_t*)g.B, g.M, g.N, g.K, out,
                           g.ldc_m);
        return hipGetLastError();
    });
}

template <class F, bool SUMI> hipError_t kq_gemv_launch_m(const GemmArgs& g, hipStream_t st) {
    if (g.M <= 1) return kq_gemv_launch_mt<F, 1, SUMI>(g, st);
    if (g.M <= 2) return kq_gemv_launch_mt<F, 2, SUMI>(g, st);
    if (g.M <= 4) return kq_gemv_launch_mt<F, 4, SUMI>(g, st);
    return kq_gemv_launch_mt<F, 8, SUMI>(g, st);
}

template <class F> hipError_t kq_gemv_launch(const GemmArgs& g, hipStream_t st) {
    // the sumi hook runs the instantiation the product picks for this shape (same MT and LPR)
    return g.sumi ? kq_gemv_launch_m<F, true>(g, st) : kq_gemv_launch_m<F, false>(g, st);
}

template <class F> bool kq_gemv_eligible(const GemmArgs& g) {
    if (g.M < 1 || g.M > 8 || g.N < 1 || g.K <= 0 || g.K % F::REC_ELEMS != 0) return false;
    if (((uintptr_t)g.B & F::WMASK) != 0 || ((uintptr_t)g.A & 3) != 0) return false;
    if (g.ldc_n != 1 || g.batch != 1 || g.ain != AIN_Q8_1 || g.lay != LAY_ROWS) return false;
    return kq_gemv_lds_bytes<F>(g.M, g.K) <= MAX_LDS_BYTES;
}

// ---- MFMA prefill ----------------------------------------------------------------------------------------------
template <class F, int TT, int RG, bool SUMI> hipError_t kq_mmq_launch_cfg(const GemmArgs& g, hipStream_t st) {
    const int gx = (g.N + 16 * RG - 1) / (16 * RG), gy = (g.M + 16 * TT - 1) / (16 * TT);
    if (g.describe) {
        describe_kernel(g, "%s TT=%d RG=%d KS=%d grid=%dx%d", F::NAME, TT, RG, F::WAVES / RG, gx, gy);
        return hipSuccess;
    }
    void* out = SUMI ? (void*)g.sumi : (void*)g.C;
    hipLaunchKernelGGL((F::template kernel<TT, RG, SUMI>()), dim3(gx, gy), dim3(64 * F::WAVES), 0, st, (const uint32_t*)g.A,
                       (const uint8_t*)g.B, g.M, g.N, g.K, out, g.ldc_m);
    return hipGetLastError();
}

template <class F, bool SUMI> hipError_t kq_mmq_launch_t(const GemmArgs& g, hipStream_t st) {
    if (g.M <= 16) return kq_mmq_launch_cfg<F, 1, 1, SUMI>(g, st);
    if (g.M <= 32) return kq_mmq_launch_cfg<F, 2, 1, SUMI>(g, st);
    // 64 x 64 tiles once they fill the CUs (M = 256 at N = 4096 on a whole MI355X)
    if ((long)((g.N + 63) / 64) * ((g.M + 63) / 64) >= device_cus()) return kq_mmq_launch_cfg<F, 4, 4, SUMI>(g, st);
    return kq_mmq_launch_cfg<F, 4, 1, SUMI>(g, st);
}

template <class F> hipError_t kq_mmq_launch(const GemmArgs& g, hipStream_t st) {
    return g.sumi ? kq_mmq_launch_t<F, true>(g, st) : kq_mmq_launch_t<F, false>(g, st);
}

template <class F> bool kq_mmq_eligible(const GemmArgs& g) {
    if (g.M < 1 || g.N < 1 || g.K <= 0 || g.K % F::KMULT != 0) return false;
    if (((uintptr_t)g.B & F::WMASK) != 0 || ((uintptr_t)g.A & 3) != 0) return false;
    if (g.ldc_n != 1 || g.batch != 1 || g.ain != AIN_Q8_1 || g.lay != LAY_ROWS) return false;
    return (g.M + 63) / 64 <= 65535;
}

// ---- the expert entries (qg_moe.hip, qg_moe_glu.hip, qg_moe_batch.hip, qg_moe_prefill.hip) ------------------------
// What an entry's launcher carries down to the instantiation it picks; its product kernel's launch: grid.x the row
// tiles of rpb rows, grid.y the slots or the plan's tiles.
template <class Args> struct MoeLaunch {
    const Args& a;
    hipStream_t st;
    char* describe;  // qg_moe*_config: name the kernel here, launch nothing
    size_t describe_len;
};
template <class K, class Args>
hipError_t moe_enqueue(K k, const MoeLaunch<Args>& L, int rpb, int gy, int wgs, size_t lds, std::atomic<unsigned long long>& done) {
    const hipError_t e = lds_opt_in((const void*)k, lds, done);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k, dim3((L.a.N + rpb - 1) / rpb, gy), dim3(wgs), lds, L.st, L.a);
    return hipGetLastError();
}

}  // namespace qg
