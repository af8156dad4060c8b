// Shared internals of libttsk (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <utility>
#include "plan_common.h"
#include "ttsk.h"
#include "wave.h"

namespace ttsk {

void set_error(const char *fmt, ...);
hipStream_t stream_of(int s);   // nullptr + error set if invalid / not initialised
int ensure_init();
int device_num_cu();            // compute units of the device of this init; 0 + error if not initialised
// grow-only per-stream arenas; nullptr + error on failure.  Slots keep nested users apart:
enum { SCRATCH_DRIVER = 0, SCRATCH_GEMM = 1, SCRATCH_MISC = 2, SCRATCH_ORTH = 3, SCRATCH_SLOTS = 4 };
void *scratch(int stream, int slot, size_t bytes);
// small allocations that live from first use to ttsk_shutdown (status words, verdict slots), one per key: a re-init on
// another device gets fresh ones.  nullptr on failure.
enum { PA_PINV_HOST = 0, PA_PINV_DEV, PA_DEFERRED, PA_PINV_BATCH_VD, PA_DEFERRED_PINNED, PA_SLOTS };
void *persistent_alloc(int key, size_t bytes, bool host, bool zero);
// chain_pack.hip: frees every packed DRM image and empties the registry (ttsk_shutdown: a re-init starts without any)
void drm_packed_clear();

#define TTSK_HIP(call)                                                          \
    do {                                                                        \
        hipError_t e_ = (call);                                                 \
        if (e_ != hipSuccess) {                                                 \
            ttsk::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                            __FILE__, __LINE__);                                \
            return TTSK_ERR_HIP;                                                \
        }                                                                       \
    } while (0)

#define TTSK_ARG(cond, ...)                                                     \
    do {                                                                        \
        if (!(cond)) {                                                          \
            ttsk::set_error(__VA_ARGS__);                                       \
            return TTSK_ERR_ARG;                                                \
        }                                                                       \
    } while (0)

#define TTSK_STREAM(var, s)                                                     \
    hipStream_t var = ttsk::stream_of(s);                                       \
    if (!var) return TTSK_ERR_ARG

// Where a kernel is launched from: converted from the stream argument of launch(), so that its errors name the call site.
struct LaunchAt {
    hipStream_t st;
    const char *file;
    int line;
    LaunchAt(hipStream_t s, const char *f = __builtin_FILE(), int l = __builtin_LINE()) : st(s), file(f), line(l) {}
};

// runtime.hip: raises kern's dynamic-LDS limit to the device's LDS per workgroup minus its static LDS, once per init;
// lock-free once raised.
int raise_lds_limit(const void *kern, const char *file, int line);

// Every kernel launch of the library goes through here: the dynamic-LDS limit (lds > 0), the launch, its check.
// TTSK_OK, or TTSK_ERR_HIP with an error naming the call site.
template <typename... P, typename... A>
int launch(void (*kern)(P...), dim3 grid, dim3 block, size_t lds, LaunchAt at, A &&...args)
{
    if (lds > 0 && raise_lds_limit((const void *)kern, at.file, at.line) != TTSK_OK) return TTSK_ERR_HIP;
    hipLaunchKernelGGL(kern, grid, block, lds, at.st, std::forward<A>(args)...);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return TTSK_OK;
    set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e), at.file, at.line);
    return TTSK_ERR_HIP;
}

// reduce.hip: out[j] (+)= sum_b part[b][j], b < nparts, j < W <= 4, by one workgroup in the stated order (wave.h); nparts = 0
// writes zeros, or with `accumulate` leaves out as it is
int sum_partials(const double *part, unsigned nparts, int W, double *out, int accumulate, LaunchAt at);

// svd_grid.hip: one-sided Jacobi SVD over all compute units (n beyond the one-workgroup kernel)
int svd_jacobi_grid(const double *A, int64_t m, int64_t n, double *US, double *S, double *Vt, int stream, hipStream_t st);

// The one place a ttsk_gemm_desc is filled: one problem (batch = 1), C[m, n] (strides c_m, c_n) (+)= alpha sum_{ko, ki}
// A[m, ko, ki] B[ko, ki, n] with the element strides given ...
inline ttsk_gemm_desc gemm_desc2(int64_t M, int64_t N, int64_t Ko, int64_t Ki, int64_t a_m, int64_t a_ko, int64_t a_ki, int64_t b_ko,
                                 int64_t b_ki, int64_t b_n, int64_t c_m, int64_t c_n, int accumulate, double alpha = 1.0)
{
    ttsk_gemm_desc d{};
    d.batch = 1; d.M = M; d.N = N; d.Ko = Ko; d.Ki = Ki;
    d.a_m = a_m; d.a_ko = a_ko; d.a_ki = a_ki;
    d.b_ko = b_ko; d.b_ki = b_ki; d.b_n = b_n;
    d.c_m = c_m; d.c_n = c_n;
    d.alpha = alpha; d.accumulate = accumulate; d.split_k = 0;
    return d;
}
// ... and the plain product: one contracted index of length K, C row-major with row stride c_m (0: N)
inline ttsk_gemm_desc gemm_desc(int64_t M, int64_t N, int64_t K, int64_t a_m, int64_t a_k, int64_t b_k, int64_t b_n, double alpha = 1.0,
                                int accumulate = 0, int64_t c_m = 0)
{
    return gemm_desc2(M, N, 1, K, a_m, 0, a_k, 0, b_k, b_n, c_m ? c_m : N, 1, accumulate, alpha);
}
// that plain product through ttsk_gemm
inline int gemm_plain(int64_t M, int64_t N, int64_t K, const double *A, int64_t a_m, int64_t a_k, const double *B, int64_t b_k,
                      int64_t b_n, double *C, int stream, double alpha = 1.0, int accumulate = 0, int64_t c_m = 0)
{
    const ttsk_gemm_desc d = gemm_desc(M, N, K, a_m, a_k, b_k, b_n, alpha, accumulate, c_m);
    return ttsk_gemm(&d, A, B, C, nullptr, stream);
}

}  // namespace ttsk
