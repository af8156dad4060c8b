// Khatri-Rao DRM (drm/khatri_rao_drm.py): column m of a level is the Kronecker product of the m-th columns of one small
// Gaussian matrix per mode, so every step is an elementwise product of rows.  ttsk_kr_rows builds the table of the rows of
// ALL prefixes of one level from the level before (the start tables of the sparse pass, kind 1 / kind 5 of ttsk_sg_factor);
// ttsk_kr_step is one step of the panels (sketch_sparse with an index row, sketch_cp without).
// What each launch gets -- the checks, the grid -- is decided in khatri_rao_plan.h.
#include "common.h"
#include "khatri_rao_plan.h"

namespace ttsk {

// one thread per element of out, row-major: row = i * P + p
__global__ __launch_bounds__(KR_THREADS) void kr_rows_kernel(const double *__restrict__ prev, int64_t P, const double *__restrict__ g,
                                                             int64_t w, int64_t total, double *__restrict__ out)
{
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = t / w, c = t - row * w;
        const int64_t i = row / P, p = row - i * P;
        out[t] = (prev ? prev[p * w + c] : 1.0) * g[i * w + c];
    }
}

// out may be v: a thread reads v[t] and writes out[t].  An index outside [0, n) is clamped: nothing is read beyond g.
__global__ __launch_bounds__(KR_THREADS) void kr_step_kernel(const double *v, const double *__restrict__ g, int64_t n, int64_t w,
                                                             const int64_t *__restrict__ idx, int64_t total, double *out)
{
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = t / w, c = t - e * w;
        int64_t i = idx ? idx[e] : e;
        i = i < 0 ? 0 : (i >= n ? n - 1 : i);
        out[t] = (v ? v[t] : 1.0) * g[i * w + c];
    }
}

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_kr_rows(const double *dev_prev, int64_t P, const double *dev_g, int64_t n, int64_t w, double *dev_out, int stream)
{
    TTSK_STREAM(st, stream);
    KrPlan p;
    if (const int rc = kr_rows_plan(dev_prev, P, dev_g, n, w, dev_out, &p)) { set_error("%s", p.msg); return rc; }
    if (!p.blocks) return TTSK_OK;
    return launch(kr_rows_kernel, dim3((unsigned)p.blocks), dim3(KR_THREADS), 0, st, dev_prev, P, dev_g, w, p.total, dev_out);
}

int ttsk_kr_step(const double *dev_v, const double *dev_g, int64_t n, int64_t w, const int64_t *dev_idx, size_t N, double *dev_out,
                 int stream)
{
    TTSK_STREAM(st, stream);
    KrPlan p;
    if (const int rc = kr_step_plan(dev_v, dev_g, n, w, dev_idx, N, dev_out, &p)) { set_error("%s", p.msg); return rc; }
    if (!p.blocks) return TTSK_OK;
    return launch(kr_step_kernel, dim3((unsigned)p.blocks), dim3(KR_THREADS), 0, st, dev_v, dev_g, n, w, dev_idx, p.total, dev_out);
}

}  // extern "C"
