// qg_host.cpp — libqg_host.so: host-only twins of the reference's CPU entry points
// (include/qg/qg_host.h). Plain C++17 on the host, no HIP; built with -ffp-contract=off so every
// float operation is the single IEEE rounding the reference's scalar loops perform.
//
// Layout: a weight format is a traits struct (block bytes, field offsets, per-block formula); the
// GEMM walks output rows (optionally over a persistent worker pool — each output's summation stays
// serial in block order, so the thread count never changes a bit). Half <-> float goes through the F16C
// conversion instructions (round-to-nearest-even, as cuda_fp16's __float2half).
#include <immintrin.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/qg/blocks.h"
#include "../../include/qg/qg.h"
#include "../../include/qg/qg_host.h"

namespace {

__attribute__((target("f16c"))) inline float half_to_float(const uint8_t* p) {
    uint16_t h;
    memcpy(&h, p, 2);
    return _cvtsh_ss(h);
}
__attribute__((target("f16c"))) inline uint16_t float_to_half(float f) {
    return _cvtss_sh(f, _MM_FROUND_TO_NEAREST_INT);
}

constexpr int QK = 32;

// Q8_1 activation block: ds = (d, s) halves at 0 / 2, qs at 4 (include/quant_types.h:116-121).
struct ActBlock {
    float d, s;
    const int8_t* qs;
    explicit ActBlock(const uint8_t* p)
        : d(half_to_float(p)), s(half_to_float(p + 2)), qs(reinterpret_cast<const int8_t*>(p + 4)) {}
};

// Weight formats. `value(p, e)` is element e's stored integer (no offset removed), `term` the
// per-block fp32 formula in the reference's operation order (see qg_common.hpp's header).
struct FmtQ4_0 {
    static constexpr int bytes = 18;
    static int value(const uint8_t* p, int e) { return e < 16 ? (p[2 + e] & 0x0F) : (p[2 + e - 16] >> 4); }
    static float term(const uint8_t* p, int32_t sumi, const ActBlock& a) {
        const float dw = half_to_float(p);
        return dw * (a.d * (float)sumi - 8.0f * a.s);  // include/gemm_reference.h:216
    }
};
struct FmtQ4_1 {
    static constexpr int bytes = 20;
    static int value(const uint8_t* p, int e) { return e < 16 ? (p[4 + e] & 0x0F) : (p[4 + e - 16] >> 4); }
    static float term(const uint8_t* p, int32_t sumi, const ActBlock& a) {
        const float dw = half_to_float(p), mw = half_to_float(p + 2);
        return dw * a.d * (float)sumi + mw * a.s;  // d * d8 * sumi + m * s8 (no /4)
    }
};
template <int QH, int QS> inline int q5_value(const uint8_t* p, int e) {
    uint32_t qh;
    memcpy(&qh, p + QH, 4);
    const int nib = e < 16 ? (p[QS + e] & 0x0F) : (p[QS + e - 16] >> 4);
    return nib | (int)(((qh >> e) & 1u) << 4);
}
struct FmtQ5_0 {
    static constexpr int bytes = 22;
    static int value(const uint8_t* p, int e) { return q5_value<2, 6>(p, e); }
    static float term(const uint8_t* p, int32_t sumi, const ActBlock& a) {
        const float dw = half_to_float(p);
        return dw * (a.d * (float)sumi - 16.0f * a.s);
    }
};
struct FmtQ5_1 {
    static constexpr int bytes = 24;
    static int value(const uint8_t* p, int e) { return q5_value<4, 8>(p, e); }
    static float term(const uint8_t* p, int32_t sumi, const ActBlock& a) {
        const float dw = half_to_float(p), mw = half_to_float(p + 2);
        return dw * a.d * (float)sumi + mw * a.s;
    }
};
struct FmtQ8_0 {
    static constexpr int bytes = 34;
    static int value(const uint8_t* p, int e) { return (int)(int8_t)p[2 + e]; }
    static float term(const uint8_t* p, int32_t sumi, const ActBlock& a) {
        const float dw = half_to_float(p);
        return (float)sumi * a.d * dw;  // include/gemm_reference.h:260
    }
};

template <class F> inline int32_t block_sumi(const uint8_t* w, const ActBlock& a) {
    // element pairs (k, k + 16) in the reference's loop order (integer sums are order-free anyway);
    // constant indices, so the per-format branches fold away
    int32_t sumi = 0;
    for (int k = 0; k < QK / 2; ++k)
        sumi += (int32_t)a.qs[k] * F::value(w, k) + (int32_t)a.qs[k + QK / 2] * F::value(w, k + QK / 2);
    return sumi;
}

template <class F> void gemm_rows(const uint8_t* A, const uint8_t* B, float* C, int M, int N, int K, int j0, int j1) {
    const int nb = K / QK;
    const size_t arow = (size_t)nb * 36, wrow = (size_t)nb * F::bytes;
    for (int i = 0; i < M; ++i)
        for (int j = j0; j < j1; ++j) {
            float sum = 0.0f;
            for (int b = 0; b < nb; ++b) {
                const ActBlock a(A + i * arow + (size_t)b * 36);
                const uint8_t* w = B + j * wrow + (size_t)b * F::bytes;
                sum += F::term(w, block_sumi<F>(w, a), a);
            }
            C[(size_t)i * N + j] = sum;
        }
}

// Q4_K (qg/blocks.h: 144-B super-blocks of 8 sub-blocks; sub-block j of super-block sb meets activation block
// 8 sb + j). The product contract of qg.h, in the decode GEMV's operation order: per super-block one fp32 dot
// accumulator and one min accumulator in sub-block order, d and dmin applied once, super-blocks summed in order.
struct FmtQ4_K {
    static constexpr int bytes = 144;
    static void scale_min(const uint8_t* q, int j, int& sc, int& m) {
        if (j < 4) {
            sc = q[j] & 63;
            m = q[j + 4] & 63;
        } else {
            sc = (q[j + 4] & 15) | ((q[j - 4] >> 6) << 4);
            m = (q[j + 4] >> 4) | ((q[j] >> 6) << 4);
        }
    }
};
template <>
void gemm_rows<FmtQ4_K>(const uint8_t* A, const uint8_t* B, float* C, int M, int N, int K, int j0, int j1) {
    const int nsb = K / 256;
    const size_t arow = (size_t)(K / QK) * 36, wrow = (size_t)nsb * FmtQ4_K::bytes;
    for (int i = 0; i < M; ++i)
        for (int n = j0; n < j1; ++n) {
            float sum = 0.0f;
            for (int sb = 0; sb < nsb; ++sb) {
                const uint8_t* w = B + n * wrow + (size_t)sb * FmtQ4_K::bytes;
                const float d = half_to_float(w), dmin = half_to_float(w + 2);
                float fd = 0.0f, fm = 0.0f;
                for (int j = 0; j < 8; ++j) {
                    const ActBlock a(A + i * arow + (size_t)(8 * sb + j) * 36);
                    const uint8_t* qs = w + 16 + 32 * (j / 2);
                    int32_t sumi = 0;
                    for (int l = 0; l < 32; ++l) sumi += (int32_t)a.qs[l] * ((j & 1) ? qs[l] >> 4 : qs[l] & 15);
                    int sc, m;
                    FmtQ4_K::scale_min(w + 4, j, sc, m);
                    fd += a.d * (float)(sc * sumi);
                    fm += (float)m * a.s;
                }
                sum += d * fd - dmin * fm;
            }
            C[(size_t)i * N + n] = sum;
        }
}

// Q6_K (qg/blocks.h: 210-B super-blocks; Q8_1 block b of super-block sb is activation block 8 sb + b and meets the
// scale groups 2b and 2b + 1). The product contract of qg.h: isum = scales[2b] * s0 + scales[2b + 1] * s1 in int32,
// one fp32 accumulator per super-block in block order, d applied once, super-blocks summed in order.
struct FmtQ6_K {
    static constexpr int bytes = 210;
    // the signed code of element 32b + l of a super-block (b = 4h + c)
    static int value(const uint8_t* w, int b, int l) {
        const int h = b >> 2, c = b & 3;
        const int lo = (w[64 * h + 32 * (c & 1) + l] >> (4 * (c >> 1))) & 15;
        const int hi = (w[128 + 32 * h + l] >> (2 * c)) & 3;
        return (lo | (hi << 4)) - 32;
    }
};
template <>
void gemm_rows<FmtQ6_K>(const uint8_t* A, const uint8_t* B, float* C, int M, int N, int K, int j0, int j1) {
    const int nsb = K / 256;
    const size_t arow = (size_t)(K / QK) * 36, wrow = (size_t)nsb * FmtQ6_K::bytes;
    for (int i = 0; i < M; ++i)
        for (int n = j0; n < j1; ++n) {
            float sum = 0.0f;
            for (int sb = 0; sb < nsb; ++sb) {
                const uint8_t* w = B + n * wrow + (size_t)sb * FmtQ6_K::bytes;
                const int8_t* sc = reinterpret_cast<const int8_t*>(w + 192);
                const float d = half_to_float(w + 208);
                float fd = 0.0f;
                for (int b = 0; b < 8; ++b) {
                    const ActBlock a(A + i * arow + (size_t)(8 * sb + b) * 36);
                    int32_t s0 = 0, s1 = 0;
                    for (int l = 0; l < 16; ++l) {
                        s0 += (int32_t)a.qs[l] * FmtQ6_K::value(w, b, l);
                        s1 += (int32_t)a.qs[l + 16] * FmtQ6_K::value(w, b, l + 16);
                    }
                    fd += a.d * (float)((int32_t)sc[2 * b] * s0 + (int32_t)sc[2 * b + 1] * s1);
                }
                sum += d * fd;
            }
            C[(size_t)i * N + n] = sum;
        }
}

// Process-wide persistent worker pool: threads are started once (grown on demand) and parked on
// a condition variable between jobs, so a multi-threaded call costs one wake-up per worker instead
// of a thread start and join (which dominated a 1-9 ms GEMV at 256 threads). One job at a time
// (callers are serialised by run_mu); the calling thread takes part 0.
class Pool {
  public:
    static Pool& get() {
        static Pool p;
        return p;
    }
    void run(int parts, const std::function<void(int)>& fn) {
        std::lock_guard<std::mutex> serial(run_mu_);
        grow(parts - 1);
        {
            std::lock_guard<std::mutex> lk(mu_);
            job_ = &fn;
            parts_ = parts;
            pending_ = parts - 1;
            ++gen_;
        }
        cv_.notify_all();
        fn(0);
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [&] { return pending_ == 0; });
        job_ = nullptr;
    }
    ~Pool() {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (auto& t : workers_) t.join();
    }

  private:
    void grow(int n) {
        while ((int)workers_.size() < n) {
            const int id = (int)workers_.size() + 1;  // part index this worker takes
            workers_.emplace_back([this, id] { loop(id); });
        }
    }
    void loop(int id) {
        unsigned long long seen = 0;
        for (;;) {
            const std::function<void(int)>* job;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || gen_ != seen; });
                if (stop_) return;
                seen = gen_;
                if (id >= parts_) continue;  // not needed for this job
                job = job_;
            }
            (*job)(id);
            std::lock_guard<std::mutex> lk(mu_);
            if (--pending_ == 0) done_.notify_one();
        }
    }
    std::mutex run_mu_, mu_;
    std::condition_variable cv_, done_;
    std::vector<std::thread> workers_;
    const std::function<void(int)>* job_ = nullptr;
    int parts_ = 0, pending_ = 0;
    unsigned long long gen_ = 0;
    bool stop_ = false;
};

// MXFP4 (qg/blocks.h: 17-B blocks, an E8M0 scale byte and 16 bytes of 4-bit codes into the doubled E2M1 table). The
// product contract of qg.h: sumi in int32, (d_a * scale(e)) * float(sumi) per block, one fp32 accumulator per output,
// blocks in order.
struct FmtMXFP4 {
    static constexpr int bytes = 17;
    static int value(const uint8_t* p, int e) {
        static const int8_t kv[16] = {0, 1, 2, 3, 4, 6, 8, 12, 0, -1, -2, -3, -4, -6, -8, -12};
        return kv[e < 16 ? (p[1 + e] & 0x0F) : (p[1 + e - 16] >> 4)];
    }
    // 2^(e - 128) from its fp32 bits (subnormal for e < 2; no NaN code)
    static float scale(uint8_t e) {
        const uint32_t bits = e < 2 ? 0x00200000u << e : (uint32_t)(e - 1) << 23;
        float f;
        memcpy(&f, &bits, 4);
        return f;
    }
};
template <>
void gemm_rows<FmtMXFP4>(const uint8_t* A, const uint8_t* B, float* C, int M, int N, int K, int j0, int j1) {
    const int nb = K / QK;
    const size_t arow = (size_t)nb * 36, wrow = (size_t)nb * FmtMXFP4::bytes;
    for (int i = 0; i < M; ++i)
        for (int n = j0; n < j1; ++n) {
            float sum = 0.0f;
            for (int b = 0; b < nb; ++b) {
                const uint8_t* w = B + n * wrow + (size_t)b * FmtMXFP4::bytes;
                const ActBlock a(A + i * arow + (size_t)b * 36);
                int32_t sumi = 0;
                for (int l = 0; l < QK; ++l) sumi += (int32_t)a.qs[l] * FmtMXFP4::value(w, l);
                sum += (a.d * FmtMXFP4::scale(w[0])) * (float)sumi;
            }
            C[(size_t)i * N + n] = sum;
        }
}
template <class F> void gemm_threads(const void* A, const void* B, float* C, int M, int N, int K, int threads) {
    auto run = [&](int j0, int j1) {
        gemm_rows<F>((const uint8_t*)A, (const uint8_t*)B, C, M, N, K, j0, j1);
    };
    threads = std::max(1, std::min(threads, N));
    if (threads == 1) return run(0, N);
    const int per = (N + threads - 1) / threads;
    const std::function<void(int)> part = [&](int t) {
        const int j0 = t * per, j1 = std::min(N, j0 + per);
        if (j0 < j1) run(j0, j1);
    };
    Pool::get().run(threads, part);
}

int check_gemm(const void* A, const void* B, const float* C, int M, int N, int K) {
    if (M < 0 || N < 0) return QG_ERR_INVALID_ARG;
    if (K <= 0 || K % QK != 0) return QG_ERR_BAD_K;
    if ((M > 0 && N > 0) && (!A || !B || !C)) return QG_ERR_INVALID_ARG;
    return QG_OK;
}

}  // namespace

extern "C" {

int qg_gemm_w4a8_cpu_mt(const void* A, const void* B, float* C, int M, int N, int K, int wtype, int threads) {
    const int rc = check_gemm(A, B, C, M, N, K);
    if (rc != QG_OK) return rc;
    if ((wtype == QG_TYPE_Q4_K || wtype == QG_TYPE_Q6_K) && K % 256 != 0) return QG_ERR_BAD_K;
    if (M == 0 || N == 0) return QG_OK;
    switch (wtype) {
        case QG_TYPE_Q4_K: gemm_threads<FmtQ4_K>(A, B, C, M, N, K, threads); return QG_OK;
        case QG_TYPE_Q6_K: gemm_threads<FmtQ6_K>(A, B, C, M, N, K, threads); return QG_OK;
        case QG_TYPE_MXFP4: gemm_threads<FmtMXFP4>(A, B, C, M, N, K, threads); return QG_OK;
        case QG_TYPE_Q4_0: gemm_threads<FmtQ4_0>(A, B, C, M, N, K, threads); return QG_OK;
        case QG_TYPE_Q4_1: gemm_threads<FmtQ4_1>(A, B, C, M, N, K, threads); return QG_OK;
        case QG_TYPE_Q5_0: gemm_threads<FmtQ5_0>(A, B, C, M, N, K, threads); return QG_OK;
        case QG_TYPE_Q5_1: gemm_threads<FmtQ5_1>(A, B, C, M, N, K, threads); return QG_OK;
        case QG_TYPE_Q8_0: gemm_threads<FmtQ8_0>(A, B, C, M, N, K, threads); return QG_OK;
    }
    return QG_ERR_UNSUPPORTED;
}

int qg_gemm_w4a8_moe_cpu(const void* A, int a_rows, const void* B, int n_expert, const int32_t* ids, int64_t ids_stride,
                         float* C, int64_t ldc, int T, int n_used, int N, int K, int wtype, int threads) {
    const bool ksb = wtype == QG_TYPE_Q4_K || wtype == QG_TYPE_Q6_K;
    int bb = 0;
    switch (wtype) {
        case QG_TYPE_Q4_0: bb = FmtQ4_0::bytes; break;
        case QG_TYPE_Q4_1: bb = FmtQ4_1::bytes; break;
        case QG_TYPE_Q5_0: bb = FmtQ5_0::bytes; break;
        case QG_TYPE_Q5_1: bb = FmtQ5_1::bytes; break;
        case QG_TYPE_Q8_0: bb = FmtQ8_0::bytes; break;
        case QG_TYPE_Q4_K: bb = FmtQ4_K::bytes; break;
        case QG_TYPE_Q6_K: bb = FmtQ6_K::bytes; break;
        case QG_TYPE_MXFP4: bb = FmtMXFP4::bytes; break;
    }
    // the order of qg_gemm_w4a8_moe
    if (T < 0 || n_used < 0 || N < 0) return QG_ERR_INVALID_ARG;
    if (K <= 0 || K % (ksb ? 256 : QK) != 0) return QG_ERR_BAD_K;
    if (!bb) return QG_ERR_UNSUPPORTED;
    if (T == 0 || n_used == 0 || N == 0) return QG_OK;
    if (!A || !B || !ids || !C) return QG_ERR_INVALID_ARG;
    if ((a_rows != 1 && a_rows != n_used) || ids_stride < n_used || n_expert < 1 || ldc < 0 || (ldc > 0 && ldc < N))
        return QG_ERR_INVALID_ARG;
    const size_t arow = (size_t)(K / QK) * 36, estride = (size_t)N * (size_t)(K / (ksb ? 256 : QK)) * (size_t)bb;
    if (ldc == 0) ldc = N;
    for (int t = 0; t < T; ++t)
        for (int u = 0; u < n_used; ++u) {
            const int e = ids[(int64_t)t * ids_stride + u];
            float* c = C + ((int64_t)t * n_used + u) * ldc;
            if (e < 0 || e >= n_expert) {
                for (int n = 0; n < N; ++n) c[n] = 0.0f;
                continue;
            }
            const uint8_t* a = (const uint8_t*)A + ((size_t)t * a_rows + (size_t)(u % a_rows)) * arow;
            const int rc = qg_gemm_w4a8_cpu_mt(a, (const uint8_t*)B + (size_t)e * estride, c, 1, N, K, wtype, threads);
            if (rc != QG_OK) return rc;
        }
    return QG_OK;
}

int qg_gemm_w4a8_moe_glu_cpu(const void* A, const void* B_gate, const void* B_up, int n_expert, const int32_t* ids,
                             int64_t ids_stride, float* C, int64_t ldc, int T, int n_used, int N, int K, int wtype, int glu_op,
                             int threads) {
    const bool ksb = wtype == QG_TYPE_Q4_K || wtype == QG_TYPE_Q6_K;
    // the order of qg_gemm_w4a8_moe_glu
    if (T < 0 || n_used < 0 || N < 0) return QG_ERR_INVALID_ARG;
    if (K <= 0 || K % (ksb ? 256 : QK) != 0) return QG_ERR_BAD_K;
    if (!ksb) return QG_ERR_UNSUPPORTED;
    if (T == 0 || n_used == 0 || N == 0) return QG_OK;
    if (!A || !B_gate || !B_up || !ids || !C) return QG_ERR_INVALID_ARG;
    if (ids_stride < n_used || n_expert < 1 || ldc < 0 || (ldc > 0 && ldc < N)) return QG_ERR_INVALID_ARG;
    if (glu_op != QG_GLU_REGLU && glu_op != QG_GLU_SWIGLU) return QG_ERR_UNSUPPORTED;
    const size_t arow = (size_t)(K / QK) * 36;
    const size_t estride = (size_t)N * (size_t)(K / 256) * (size_t)(wtype == QG_TYPE_Q4_K ? FmtQ4_K::bytes : FmtQ6_K::bytes);
    if (ldc == 0) ldc = N;
    std::vector<float> g((size_t)N), up((size_t)N);
    for (int t = 0; t < T; ++t)
        for (int u = 0; u < n_used; ++u) {
            const int e = ids[(int64_t)t * ids_stride + u];
            float* c = C + ((int64_t)t * n_used + u) * ldc;
            if (e < 0 || e >= n_expert) {
                for (int n = 0; n < N; ++n) c[n] = 0.0f;
                continue;
            }
            const uint8_t* a = (const uint8_t*)A + (size_t)t * arow;
            int rc = qg_gemm_w4a8_cpu_mt(a, (const uint8_t*)B_gate + (size_t)e * estride, g.data(), 1, N, K, wtype, threads);
            if (rc == QG_OK)
                rc = qg_gemm_w4a8_cpu_mt(a, (const uint8_t*)B_up + (size_t)e * estride, up.data(), 1, N, K, wtype, threads);
            if (rc != QG_OK) return rc;
            // each operation one rounded fp32 operation (-ffp-contract=off), as the GPU entry
            if (glu_op == QG_GLU_REGLU)
                for (int n = 0; n < N; ++n) c[n] = (g[n] > 0.0f ? g[n] : 0.0f) * up[n];
            else
                for (int n = 0; n < N; ++n) c[n] = (g[n] / (1.0f + expf(-g[n]))) * up[n];
        }
    return QG_OK;
}

int qg_gemm_w4a8_moe_down_cpu(const void* A, const void* B, int n_expert, const int32_t* ids, int64_t ids_stride,
                              const float* weights, int64_t w_stride, float* C, int64_t ldc, int T, int n_used, int N, int K,
                              int wtype, int threads) {
    const bool ksb = wtype == QG_TYPE_Q4_K || wtype == QG_TYPE_Q6_K;
    // the order of qg_gemm_w4a8_moe_down
    if (T < 0 || n_used < 0 || N < 0) return QG_ERR_INVALID_ARG;
    if (K <= 0 || K % (ksb ? 256 : QK) != 0) return QG_ERR_BAD_K;
    if (!ksb) return QG_ERR_UNSUPPORTED;
    if (T == 0 || n_used == 0 || N == 0) return QG_OK;
    if (!A || !B || !ids || !C) return QG_ERR_INVALID_ARG;
    if (ids_stride < n_used || n_expert < 1 || ldc < 0 || (ldc > 0 && ldc < N) || (weights && w_stride < n_used))
        return QG_ERR_INVALID_ARG;
    const size_t arow = (size_t)(K / QK) * 36;
    const size_t estride = (size_t)N * (size_t)(K / 256) * (size_t)(wtype == QG_TYPE_Q4_K ? FmtQ4_K::bytes : FmtQ6_K::bytes);
    if (ldc == 0) ldc = N;
    std::vector<float> d((size_t)N);
    for (int t = 0; t < T; ++t) {
        float* c = C + (int64_t)t * ldc;
        for (int n = 0; n < N; ++n) c[n] = 0.0f;
        for (int u = 0; u < n_used; ++u) {
            const int e = ids[(int64_t)t * ids_stride + u];
            if (e < 0 || e >= n_expert) continue;  // neither its weight nor a weight byte is read
            const uint8_t* a = (const uint8_t*)A + ((size_t)t * n_used + (size_t)u) * arow;
            const int rc = qg_gemm_w4a8_cpu_mt(a, (const uint8_t*)B + (size_t)e * estride, d.data(), 1, N, K, wtype, threads);
            if (rc != QG_OK) return rc;
            // each operation one rounded fp32 operation (-ffp-contract=off), as the GPU entry
            const float w = weights ? weights[(int64_t)t * w_stride + u] : 1.0f;
            for (int n = 0; n < N; ++n) c[n] = c[n] + w * d[n];
        }
    }
    return QG_OK;
}

namespace {
// the two _bias twins: Q4_K / Q6_K / MXFP4, the bytes of a block and the elements it holds (0: not a type of theirs)
int bias_block(int wtype, int& elems) {
    elems = wtype == QG_TYPE_MXFP4 ? QK : 256;
    switch (wtype) {
        case QG_TYPE_Q4_K: return FmtQ4_K::bytes;
        case QG_TYPE_Q6_K: return FmtQ6_K::bytes;
        case QG_TYPE_MXFP4: return FmtMXFP4::bytes;
    }
    elems = QK;
    return 0;
}
}  // namespace

int qg_gemm_w4a8_moe_glu_bias_cpu(const void* A, const void* B_gate, const void* B_up, const float* bias_gate,
                                  const float* bias_up, int64_t bias_stride, int n_expert, const int32_t* ids,
                                  int64_t ids_stride, float* C, int64_t ldc, int T, int n_used, int N, int K, int wtype,
                                  int glu_op, float alpha, float limit, int threads) {
    int be;
    const int bb = bias_block(wtype, be);
    // the order of qg_gemm_w4a8_moe_glu_bias
    if (T < 0 || n_used < 0 || N < 0) return QG_ERR_INVALID_ARG;
    if (K <= 0 || K % be != 0) return QG_ERR_BAD_K;
    if (!bb) return QG_ERR_UNSUPPORTED;
    if (T == 0 || n_used == 0 || N == 0) return QG_OK;
    if (!A || !B_gate || !B_up || !ids || !C) return QG_ERR_INVALID_ARG;
    if (ids_stride < n_used || n_expert < 1 || ldc < 0 || (ldc > 0 && ldc < N)) return QG_ERR_INVALID_ARG;
    if (bias_stride < 0 || (bias_stride > 0 && bias_stride < N)) return QG_ERR_INVALID_ARG;
    if (glu_op == QG_GLU_SWIGLU_OAI && !(std::isfinite(alpha) && std::isfinite(limit) && limit > 0.0f)) return QG_ERR_INVALID_ARG;
    if (glu_op != QG_GLU_REGLU && glu_op != QG_GLU_SWIGLU && glu_op != QG_GLU_SWIGLU_OAI) return QG_ERR_UNSUPPORTED;
    const size_t arow = (size_t)(K / QK) * 36, estride = (size_t)N * (size_t)(K / be) * (size_t)bb;
    if (ldc == 0) ldc = N;
    if (bias_stride == 0) bias_stride = N;
    std::vector<float> g((size_t)N), up((size_t)N);
    for (int t = 0; t < T; ++t)
        for (int u = 0; u < n_used; ++u) {
            const int e = ids[(int64_t)t * ids_stride + u];
            float* c = C + ((int64_t)t * n_used + u) * ldc;
            if (e < 0 || e >= n_expert) {  // no bias is read or applied
                for (int n = 0; n < N; ++n) c[n] = 0.0f;
                continue;
            }
            const uint8_t* a = (const uint8_t*)A + (size_t)t * arow;
            int rc = qg_gemm_w4a8_cpu_mt(a, (const uint8_t*)B_gate + (size_t)e * estride, g.data(), 1, N, K, wtype, threads);
            if (rc == QG_OK)
                rc = qg_gemm_w4a8_cpu_mt(a, (const uint8_t*)B_up + (size_t)e * estride, up.data(), 1, N, K, wtype, threads);
            if (rc != QG_OK) return rc;
            // each operation one rounded fp32 operation (-ffp-contract=off), as the GPU entry
            if (bias_gate)
                for (int n = 0; n < N; ++n) g[n] = g[n] + bias_gate[(int64_t)e * bias_stride + n];
            if (bias_up)
                for (int n = 0; n < N; ++n) up[n] = up[n] + bias_up[(int64_t)e * bias_stride + n];
            if (glu_op == QG_GLU_REGLU)
                for (int n = 0; n < N; ++n) c[n] = (g[n] > 0.0f ? g[n] : 0.0f) * up[n];
            else if (glu_op == QG_GLU_SWIGLU)
                for (int n = 0; n < N; ++n) c[n] = (g[n] / (1.0f + expf(-g[n]))) * up[n];
            else
                for (int n = 0; n < N; ++n) {
                    const float x = fminf(g[n], limit), y = fminf(fmaxf(up[n], -limit), limit);
                    c[n] = (x / (1.0f + expf(alpha * (-x)))) * (y + 1.0f);
                }
        }
    return QG_OK;
}

int qg_gemm_w4a8_moe_down_bias_cpu(const void* A, const void* B, const float* bias, int64_t bias_stride, int n_expert,
                                   const int32_t* ids, int64_t ids_stride, const float* weights, int64_t w_stride, float* C,
                                   int64_t ldc, int T, int n_used, int N, int K, int wtype, int threads) {
    int be;
    const int bb = bias_block(wtype, be);
    // the order of qg_gemm_w4a8_moe_down_bias
    if (T < 0 || n_used < 0 || N < 0) return QG_ERR_INVALID_ARG;
    if (K <= 0 || K % be != 0) return QG_ERR_BAD_K;
    if (!bb) return QG_ERR_UNSUPPORTED;
    if (T == 0 || n_used == 0 || N == 0) return QG_OK;
    if (!A || !B || !ids || !C) return QG_ERR_INVALID_ARG;
    if (ids_stride < n_used || n_expert < 1 || ldc < 0 || (ldc > 0 && ldc < N) || (weights && w_stride < n_used))
        return QG_ERR_INVALID_ARG;
    if (bias_stride < 0 || (bias_stride > 0 && bias_stride < N)) return QG_ERR_INVALID_ARG;
    const size_t arow = (size_t)(K / QK) * 36, estride = (size_t)N * (size_t)(K / be) * (size_t)bb;
    if (ldc == 0) ldc = N;
    if (bias_stride == 0) bias_stride = N;
    std::vector<float> d((size_t)N);
    for (int t = 0; t < T; ++t) {
        float* c = C + (int64_t)t * ldc;
        for (int n = 0; n < N; ++n) c[n] = 0.0f;
        for (int u = 0; u < n_used; ++u) {
            const int e = ids[(int64_t)t * ids_stride + u];
            if (e < 0 || e >= n_expert) continue;  // neither its bias, its weight nor a weight byte is read
            const uint8_t* a = (const uint8_t*)A + ((size_t)t * n_used + (size_t)u) * arow;
            const int rc = qg_gemm_w4a8_cpu_mt(a, (const uint8_t*)B + (size_t)e * estride, d.data(), 1, N, K, wtype, threads);
            if (rc != QG_OK) return rc;
            // each operation one rounded fp32 operation (-ffp-contract=off), as the GPU entry
            if (bias)
                for (int n = 0; n < N; ++n) d[n] = d[n] + bias[(int64_t)e * bias_stride + n];
            const float w = weights ? weights[(int64_t)t * w_stride + u] : 1.0f;
            for (int n = 0; n < N; ++n) c[n] = c[n] + w * d[n];
        }
    }
    return QG_OK;
}

int qg_gemm_w4a8_moe_bias_cpu(const void* A, int a_rows, const void* B, const float* bias, int64_t bias_stride, int n_expert,
                              const int32_t* ids, int64_t ids_stride, float* C, int64_t ldc, int T, int n_used, int N, int K,
                              int wtype, int threads) {
    int be;
    const int bb = bias_block(wtype, be);
    // the order of qg_gemm_w4a8_moe_prefill_bias / _moe_batch_bias (no workspace here)
    if (T < 0 || n_used < 0 || N < 0) return QG_ERR_INVALID_ARG;
    if (K <= 0 || K % be != 0) return QG_ERR_BAD_K;
    if (!bb) return QG_ERR_UNSUPPORTED;
    if (T == 0 || n_used == 0 || N == 0) return QG_OK;
    if (!A || !B || !ids || !C) return QG_ERR_INVALID_ARG;
    if (bias_stride < 0 || (bias_stride > 0 && bias_stride < N)) return QG_ERR_INVALID_ARG;
    // the product of qg_gemm_w4a8_moe_cpu (the remaining checks are its own), then one rounded fp32 addition (-ffp-contract=off)
    const int rc = qg_gemm_w4a8_moe_cpu(A, a_rows, B, n_expert, ids, ids_stride, C, ldc, T, n_used, N, K, wtype, threads);
    if (rc != QG_OK || !bias) return rc;
    if (ldc == 0) ldc = N;
    if (bias_stride == 0) bias_stride = N;
    for (int t = 0; t < T; ++t)
        for (int u = 0; u < n_used; ++u) {
            const int e = ids[(int64_t)t * ids_stride + u];
            if (e < 0 || e >= n_expert) continue;  // +0.0f stays: no bias is read
            float* c = C + ((int64_t)t * n_used + u) * ldc;
            for (int n = 0; n < N; ++n) c[n] = c[n] + bias[(int64_t)e * bias_stride + n];
        }
    return QG_OK;
}

int qg_dequantize_row_mxfp4_cpu(const void* x, float* y, int64_t k) {
    if (k < 0 || k % QK != 0) return QG_ERR_BAD_K;
    if (k == 0) return QG_OK;
    if (!x || !y) return QG_ERR_INVALID_ARG;
    for (int64_t i = 0; i < k; ++i) {
        const uint8_t* b = (const uint8_t*)x + (i / QK) * FmtMXFP4::bytes;
        y[i] = (float)FmtMXFP4::value(b, (int)(i % QK)) * FmtMXFP4::scale(b[0]);
    }
    return QG_OK;
}

int qg_gemm_w4a8_q4_0_cpu(const void* A, const void* B, float* C, int M, int N, int K) {
    return qg_gemm_w4a8_cpu_mt(A, B, C, M, N, K, QG_TYPE_Q4_0, 1);
}

int qg_gemm_w8a8_cpu(const void* A, const void* B, float* C, int M, int N, int K) {
    return qg_gemm_w4a8_cpu_mt(A, B, C, M, N, K, QG_TYPE_Q8_0, 1);
}

void qg_vec_dot_q4_0_q8_1_cpu(int n, float* s, const void* vx, const void* vy) {
    const uint8_t* x = (const uint8_t*)vx;
    const uint8_t* y = (const uint8_t*)vy;
    float sum = 0.0f;
    for (int b = 0; b < n / QK; ++b) {
        const ActBlock a(y + (size_t)b * 36);
        const uint8_t* w = x + (size_t)b * FmtQ4_0::bytes;
        sum += FmtQ4_0::term(w, block_sumi<FmtQ4_0>(w, a), a);
    }
    *s = sum;
}

void qg_vec_dot_q8_0_q8_1_cpu(int n, float* s, const void* vx, const void* vy) {
    const uint8_t* x = (const uint8_t*)vx;
    const uint8_t* y = (const uint8_t*)vy;
    float sum = 0.0f;
    for (int b = 0; b < n / QK; ++b) {
        const ActBlock a(y + (size_t)b * 36);
        const uint8_t* w = x + (size_t)b * FmtQ8_0::bytes;
        const float dw = half_to_float(w);
        sum += (float)block_sumi<FmtQ8_0>(w, a) * dw * a.d;  // sumi * d_w * d_a (gemm_reference.h:333)
    }
    *s = sum;
}

int qg_gemm_fp32_cpu(const float* A, const float* B, float* C, int M, int N, int K) {
    if (M < 0 || N < 0 || K < 0) return QG_ERR_INVALID_ARG;
    if (M == 0 || N == 0) return QG_OK;
    if (!A || !B || !C) return QG_ERR_INVALID_ARG;
    for (int i = 0; i < M; ++i)
        for (int j = 0; j < N; ++j) {
            float sum = 0.0f;
            for (int k = 0; k < K; ++k) sum += A[(size_t)i * K + k] * B[(size_t)j * K + k];
            C[(size_t)i * N + j] = sum;
        }
    return QG_OK;
}

int qg_quantize_row_q8_1_cpu(const float* x, void* yv, int64_t k) {
    if (k < 0 || k % QK != 0) return QG_ERR_BAD_K;
    if (k && (!x || !yv)) return QG_ERR_INVALID_ARG;
    uint8_t* y = (uint8_t*)yv;
    for (int64_t b = 0; b < k / QK; ++b) {
        const float* v = x + b * QK;
        uint8_t* o = y + b * 36;
        float amax = 0.0f, sum = 0.0f;
        for (int j = 0; j < QK; ++j) {
            amax = std::max(amax, std::fabs(v[j]));
            sum += v[j];
        }
        const float d = amax / 127.0f;
        const uint16_t hd = float_to_half(d), hs = float_to_half(sum);
        memcpy(o, &hd, 2);
        memcpy(o + 2, &hs, 2);
        const float id = d > 0 ? 1.0f / d : 0.0f;
        for (int j = 0; j < QK; ++j) {
            const int q = (int)std::round(v[j] * id);  // roundf: half away from zero
            o[4 + j] = (uint8_t)(int8_t)std::max(-128, std::min(127, q));
        }
    }
    return QG_OK;
}

int qg_quantize_row_q4_0_cpu(const float* x, void* yv, int64_t k) {
    if (k < 0 || k % QK != 0) return QG_ERR_BAD_K;
    if (k && (!x || !yv)) return QG_ERR_INVALID_ARG;
    uint8_t* y = (uint8_t*)yv;
    for (int64_t b = 0; b < k / QK; ++b) {
        const float* v = x + b * QK;
        uint8_t* o = y + b * 18;
        float amax = 0.0f;
        for (int j = 0; j < QK; ++j) amax = std::max(amax, std::fabs(v[j]));
        const float d = amax / 7.0f;
        const uint16_t hd = float_to_half(d);
        memcpy(o, &hd, 2);
        const float id = d > 0 ? 1.0f / d : 0.0f;
        auto q4 = [&](float f) { return std::max(0, std::min(15, (int)std::round(f * id) + 8)); };
        for (int j = 0; j < QK / 2; ++j) o[2 + j] = (uint8_t)(q4(v[j]) | (q4(v[j + QK / 2]) << 4));
    }
    return QG_OK;
}

int qg_fill_step4_cpu(unsigned seed, int M, int N, int K, int row0, int row1, float* a, float* b) {
    if (M < 0 || N < 0 || K < 0 || row0 < 0 || row1 < row0 || row1 > N) return QG_ERR_INVALID_ARG;
    auto draw = []() { return 2.0f * (float)rand() / RAND_MAX - 1.0f; };
    srand(seed);
    const int64_t na = (int64_t)M * K;
    for (int64_t i = 0; i < na; ++i) {
        const float v = draw();
        if (a) a[i] = v;
    }
    const int64_t skip = (int64_t)row0 * K, take = (int64_t)(row1 - row0) * K;
    for (int64_t i = 0; i < skip; ++i) (void)rand();
    for (int64_t i = 0; i < take; ++i) {
        const float v = draw();
        if (b) b[i] = v;
    }
    return QG_OK;
}

}  // extern "C"
