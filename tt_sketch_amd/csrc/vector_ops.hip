// Strided copies, axpby, the sum of the slices of a batch, and the probe of the fp64 matrix rate: the entry points that
// move or add vectors without a contraction.
// What each launch gets -- the checks, the copy's CopyDesc, the route of the slice sum, the grids -- is decided in vector_plan.h.
#include "common.h"
#include "vector_plan.h"

namespace ttsk {

__global__ void copy_strided_kernel(double *dst, const double *src, CopyDesc c)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < c.total;
         i += (int64_t)gridDim.x * blockDim.x) {
        int64_t t = i, so = 0, dof = 0;
#pragma unroll
        for (int a = 4; a >= 0; --a) {
            int64_t q = t / c.shape[a], r = t - q * c.shape[a];
            so += r * c.ss[a];
            dof += r * c.ds[a];
            t = q;
        }
        dst[dof] = src[so];
    }
}

__global__ void axpby_kernel(double *y, const double *x, double a, double b, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x)
        y[i] = a * x[i] + (b == 0.0 ? 0.0 : b * y[i]);
}

// dst[i] (+)= sum_b src[b * stride + i]: the sketches of a batch summed into one (TensorSum)
// (the slices are requested eight at a time and added in order: one load after the other, each waiting for the sum,
// was 15 us for 32 slices of 6400 numbers -- a handful of workgroups, nothing to hide a round trip behind)
__global__ __launch_bounds__(256) void sum_slices_kernel(double2 *dst, const double2 *src, int nb, size_t stride2,
                                                         size_t n2, int accumulate)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2; i += (size_t)gridDim.x * blockDim.x) {
        double2 acc = accumulate ? dst[i] : make_double2(0.0, 0.0);
        const double2 *p = src + i;
        int b = 0;
        for (; b + 8 <= nb; b += 8, p += 8 * stride2) {
            double2 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(size_t)u * stride2];
#pragma unroll
            for (int u = 0; u < 8; ++u) { acc.x += v[u].x; acc.y += v[u].y; }
        }
        for (; b < nb; ++b, p += stride2) {
            const double2 v = *p;
            acc.x += v.x;
            acc.y += v.y;
        }
        dst[i] = acc;
    }
}

// the same for odd lengths / strides or bases that are not 16-byte aligned
__global__ __launch_bounds__(256) void sum_slices_scalar_kernel(double *dst, const double *src, int nb, size_t stride, size_t n,
                                                                int accumulate)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        double acc = accumulate ? dst[i] : 0.0;
        const double *p = src + i;
        int b = 0;
        for (; b + 8 <= nb; b += 8, p += 8 * stride) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(size_t)u * stride];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u];
        }
        for (; b < nb; ++b, p += stride) acc += *p;
        dst[i] = acc;
    }
}

// 512 threads = two waves per SIMD and at most 256 registers each: with __launch_bounds__(256) hipcc parks the
// accumulators in AGPRs and copies them in and out around every instruction (32 v_accvgpr moves + s_nop per
// 4 matrix instructions) -- round 1's "49 TF/s ceiling of the 16x16x4 form" was that code, not the pipe.
__global__ __launch_bounds__(512) void mfma_probe_kernel(double *sink, int iters, double seed)
{
    v4d a0 = {0, 0, 0, 0}, a1 = a0, a2 = a0, a3 = a0;
    double x = seed + threadIdx.x * 1e-3, y = seed - threadIdx.x * 1e-3;
    for (int i = 0; i < iters; ++i) {
        a0 = mfma16(x, y, a0);
        a1 = mfma16(y, x, a1);
        a2 = mfma16(x, x, a2);
        a3 = mfma16(y, y, a3);
    }
    v4d t = a0 + a1 + a2 + a3;
    if (t[0] + t[1] + t[2] + t[3] == 12345.678) sink[blockIdx.x] = t[0];
}

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_mfma_f64_peak_probe(double *tflops)
{
    TTSK_STREAM(st, 0);
    TTSK_ARG(tflops, "ttsk_mfma_f64_peak_probe: NULL");
    double *sink = (double *)scratch(0, SCRATCH_GEMM, 1 << 16);
    if (!sink) return TTSK_ERR_HIP;
    const int blocks = 256 * 4, iters = 2000;
    hipEvent_t a, b;
    TTSK_HIP(hipEventCreate(&a));
    TTSK_HIP(hipEventCreate(&b));
    double best = 0;
    for (int rep = 0; rep < 4; ++rep) {
        TTSK_HIP(hipEventRecord(a, st));
        if (int rc = launch(mfma_probe_kernel, dim3(blocks), dim3(512), 0, st, sink, iters, 1.0 + rep)) return rc;
        TTSK_HIP(hipEventRecord(b, st));
        TTSK_HIP(hipEventSynchronize(b));
        float ms = 0;
        TTSK_HIP(hipEventElapsedTime(&ms, a, b));
        double fl = (double)blocks * 8 /*waves*/ * iters * 4 /*mfma*/ * 2048.0;
        double tf = fl / (ms * 1e-3) * 1e-12;
        if (rep > 0 && tf > best) best = tf;
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    *tflops = best;
    return TTSK_OK;
}

int ttsk_copy_strided(double *dst, const double *src, int ndim, const int64_t *shape,
                      const int64_t *dst_strides, const int64_t *src_strides, int stream)
{
    TTSK_STREAM(st, stream);
    CopyPlan p;
    if (const int rc = copy_strided_plan(dst, src, ndim, shape, dst_strides, src_strides, &p)) { set_error("%s", p.msg); return rc; }
    if (!p.blocks) return TTSK_OK;
    return launch(copy_strided_kernel, dim3((unsigned)p.blocks), dim3(VEC_THREADS), 0, st, dst, src, p.c);
}

int ttsk_sum_slices(double *dst, const double *src, int nb, size_t stride, size_t n, int accumulate, int stream)
{
    TTSK_STREAM(st, stream);
    SumSlicesPlan p;
    if (const int rc = sum_slices_plan(dst, src, nb, stride, n, accumulate, &p)) { set_error("%s", p.msg); return rc; }
    if (!p.blocks) return TTSK_OK;
    if (!p.vector)
        return launch(sum_slices_scalar_kernel, dim3((unsigned)p.blocks), dim3(VEC_THREADS), 0, st, dst, src, nb, p.stride, p.n, accumulate);
    return launch(sum_slices_kernel, dim3((unsigned)p.blocks), dim3(VEC_THREADS), 0, st, (double2 *)dst, (const double2 *)src,
                  nb, p.stride, p.n, accumulate);
}

int ttsk_axpby(double *y, const double *x, double a, double b, size_t n, int stream)
{
    TTSK_STREAM(st, stream);
    AxpbyPlan p;
    if (const int rc = axpby_plan(y, x, a, b, n, &p)) { set_error("%s", p.msg); return rc; }
    if (!p.blocks) return TTSK_OK;
    return launch(axpby_kernel, dim3((unsigned)p.blocks), dim3(VEC_THREADS), 0, st, y, x, a, b, n);
}

}  // extern "C"
