// Products with a Gaussian DRM matrix that is never stored (DenseGaussianDRM(stored=False), drm/dense_gaussian_drm.py):
//   G[m, c] = ndtri(u),  u = mant_unit(force_exponent(mix64(m * cols + c + key))),  key = mix64(seed ^ 0x9E3779B97F4A7C15),
//   u == 0 -> 2^-53
// -- the rows of what ttsk_fill_normal writes for (rows, cols) and the same seed, from the same device code (sampler_dev.h), so
// the same bits.  ttsk_gauss_lazy_left and ttsk_gauss_lazy_right are ONE fp64 MFMA GEMM D[m, n] = sum_k G[lo + m, k] X[k, n]
// (gauss_lazy_plan.h) that differ in how X and D lie in memory.  What each launch gets is decided in gauss_lazy_plan.h.
//
// A workgroup: GL_NT columns n, one chunk of k, walked GL_KB at a time.  Per step
//   1. its 256 threads load the (GL_KB x GL_NT) tile of X into registers (in flight during 2),
//   2. sample the (w x GL_KB) tile of G into LDS: central samples finished in place, tail samples queued (tile_sample),
//   3. store the X tile to LDS, evaluate the queued tails in full waves (tile_drain),
//   4. every wave multiplies the sample tile into its 64 columns: MT x 4 accumulator tiles, four v_mfma_f64_16x16x4 each.
// A wave's own vector-ALU work is not hidden behind its own fp64 matrix instructions, so 2 and 4 take turns
// and what counts is the ratio: w * GL_KB samples per 2 * w * GL_KB * GL_NT flops, one sample per 512 flops whatever w is.
// Sums: k ascending inside a chunk (the matrix instruction's own order inside its four), chunks ascending in the closing
// launch.  No atomics on memory; the same bits on every call.
#include "common.h"
#include "gauss_lazy_plan.h"
#include "prof.h"
#include "sampler_dev.h"

namespace ttsk {

struct GlArgs {
    uint64_t key;                // mix64(seed ^ 0x9E37...): added to the flat index
    int64_t row_lo, cols;        // first row of G, its row length (= K)
    int w, K, N;
    int64_t chunk;               // k per workgroup (blockIdx.y)
    const double *x;
    int64_t xs_k, xs_n;          // element strides of X[k, n]
    double *d;                   // D[m, n] at d[m * ds_m + n * ds_n]: the product itself, or the workspace's first chunk
    int64_t ds_m, ds_n, ds_chunk;
};

template <int MT, bool KFAST>
__global__ __launch_bounds__(GL_THREADS) void gauss_lazy_kernel(GlArgs a)
{
    __shared__ double Gs[GL_KB * GL_GP];                                   // [k][m]; rows m >= w stay zero
    __shared__ double Xs[KFAST ? GL_NT * GL_XPK : GL_KB * GL_XP];          // KFAST: [n][k], else [k][n]
    __shared__ unsigned short tq[GL_KB * GL_GP];
    __shared__ int tq_n;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * GL_NT;
    const int64_t kb = (int64_t)blockIdx.y * a.chunk;
    const int64_t kend = kb + a.chunk < a.K ? kb + a.chunk : (int64_t)a.K;
    for (int i = tid; i < GL_KB * GL_GP; i += GL_THREADS) Gs[i] = 0.0;
    v4d acc[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = v4d{0.0, 0.0, 0.0, 0.0};

    for (int64_t k0 = kb; k0 < kend; k0 += GL_KB) {
        double xr[GL_KB];
#pragma unroll
        for (int s = 0; s < GL_KB; ++s) {
            const int e = tid + GL_THREADS * s;
            const int k = KFAST ? (e & (GL_KB - 1)) : s;
            const int n = KFAST ? (e >> 4) : tid;
            const int64_t kg = k0 + k, ng = n0 + n;
            xr[s] = (kg < kend && ng < a.N) ? a.x[kg * a.xs_k + ng * a.xs_n] : 0.0;
        }
        if (tid == 0) tq_n = 0;
        __syncthreads();                                                   // the step before has read its tiles
        for (int e = tid; e < a.w * GL_KB; e += GL_THREADS) {
            const int k = e & (GL_KB - 1), m = e >> 4;
            const int slot = k * GL_GP + m;
            const int64_t kg = k0 + k;
            if (kg < kend) {
                const uint64_t flat = (uint64_t)(a.row_lo + m) * (uint64_t)a.cols + (uint64_t)kg;
                double u = mant_unit(force_exponent(mix64(flat + a.key)));
                if (u == 0.0) u = 0x1p-53;
                tile_sample(u, slot, 1.0, Gs, tq, &tq_n);
            } else {
                Gs[slot] = 0.0;
            }
        }
#pragma unroll
        for (int s = 0; s < GL_KB; ++s) {
            const int e = tid + GL_THREADS * s;
            if (KFAST) Xs[(e >> 4) * GL_XPK + (e & (GL_KB - 1))] = xr[s];
            else Xs[s * GL_XP + tid] = xr[s];
        }
        tile_drain(1.0, Gs, tq, &tq_n);
#pragma unroll
        for (int kk = 0; kk < GL_KB / 4; ++kk) {
            const int kr = kk * 4 + (lane >> 4);
            double af[MT], bf[4];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) af[mt] = Gs[kr * GL_GP + mt * 16 + (lane & 15)];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int n = wv * 64 + nt * 16 + (lane & 15);
                bf[nt] = KFAST ? Xs[n * GL_XPK + kr] : Xs[kr * GL_XP + n];
            }
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = mfma16(af[mt], bf[nt], acc[mt][nt]);
        }
    }
    double *d = a.d + (int64_t)blockIdx.y * a.ds_chunk;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int m = mt * 16 + (lane >> 4) + 4 * j;
                const int64_t n = n0 + wv * 64 + nt * 16 + (lane & 15);
                if (m < a.w && n < a.N) d[m * a.ds_m + n * a.ds_n] = acc[mt][nt][j];
            }
}

// D[m, n] = sum_c ws[c, m, n], c ascending; one thread per element, n fastest
__global__ __launch_bounds__(GL_THREADS) void gauss_lazy_close_kernel(const double *__restrict__ ws, int64_t nchunks, int64_t w, int64_t N,
                                                                     double *__restrict__ d, int64_t ds_m, int64_t ds_n)
{
    const int64_t total = w * N;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        double s = ws[t];
        for (int64_t c = 1; c < nchunks; ++c) s += ws[c * total + t];
        const int64_t m = t / N, n = t - m * N;
        d[m * ds_m + n * ds_n] = s;
    }
}

template <bool KFAST>
static int launch_main(int mt, dim3 grid, hipStream_t st, const GlArgs &a)
{
    switch (mt) {
    case 1: return launch(gauss_lazy_kernel<1, KFAST>, grid, dim3(GL_THREADS), 0, st, a);
    case 2: return launch(gauss_lazy_kernel<2, KFAST>, grid, dim3(GL_THREADS), 0, st, a);
    case 3: return launch(gauss_lazy_kernel<3, KFAST>, grid, dim3(GL_THREADS), 0, st, a);
    default: return launch(gauss_lazy_kernel<4, KFAST>, grid, dim3(GL_THREADS), 0, st, a);
    }
}

static int gauss_lazy(int side, uint64_t seed, int64_t row_lo, int64_t row_hi, int64_t cols, const double *x, int64_t N, int64_t ldx, double *d,
                      int64_t ldd, int stream)
{
    TTSK_STREAM(st, stream);
    GlPlan p;
    if (const int rc = gauss_lazy_plan(side, row_lo, row_hi, cols, x, N, ldx, d, ldd, &p)) { set_error("%s", p.msg); return rc; }
    if (p.branch == GL_NOTHING) return TTSK_OK;
    ProfBracket prof(st, PROF_OTHER, p.flops, side == GL_LEFT ? "gauss_lazy_kernel (left)" : "gauss_lazy_kernel (right)");
    GlArgs a{};
    a.key = mix64(seed ^ 0x9E3779B97F4A7C15ULL);                             // as ttsk_fill_normal: the same samples
    a.row_lo = row_lo; a.cols = cols;
    a.w = p.w; a.K = (int)p.K; a.N = (int)p.N;
    a.chunk = p.chunk;
    a.x = x;
    a.xs_k = side == GL_LEFT ? ldx : 1;
    a.xs_n = side == GL_LEFT ? 1 : ldx;
    const int64_t ds_m = side == GL_LEFT ? ldd : 1, ds_n = side == GL_LEFT ? 1 : ldd;
    double *ws = nullptr;
    if (p.branch == GL_SPLIT) {
        ws = (double *)scratch(stream, SCRATCH_MISC, (size_t)p.ws_elems * 8);
        if (!ws) return TTSK_ERR_HIP;
        a.d = ws; a.ds_m = p.N; a.ds_n = 1; a.ds_chunk = (int64_t)p.w * p.N;
    } else {
        a.d = d; a.ds_m = ds_m; a.ds_n = ds_n; a.ds_chunk = 0;
    }
    const dim3 grid((unsigned)p.tiles, (unsigned)p.nchunks);
    if (const int rc = side == GL_LEFT ? launch_main<false>(p.mt, grid, st, a) : launch_main<true>(p.mt, grid, st, a)) return rc;
    if (p.branch == GL_SPLIT)
        return launch(gauss_lazy_close_kernel, dim3((unsigned)p.close_blocks), dim3(GL_THREADS), 0, st, ws, p.nchunks, (int64_t)p.w, p.N, d, ds_m,
                      ds_n);
    return TTSK_OK;
}

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_gauss_lazy_left(uint64_t seed, int64_t row_lo, int64_t row_hi, int64_t cols, const double *dev_xu, int64_t Q, int64_t ldx,
                         double *dev_z, int64_t ldz, int stream)
{
    return gauss_lazy(GL_LEFT, seed, row_lo, row_hi, cols, dev_xu, Q, ldx, dev_z, ldz, stream);
}

int ttsk_gauss_lazy_right(uint64_t seed, int64_t row_lo, int64_t row_hi, int64_t cols, const double *dev_s, int64_t rows, int64_t lds,
                          double *dev_out, int64_t ldo, int stream)
{
    return gauss_lazy(GL_RIGHT, seed, row_lo, row_hi, cols, dev_s, rows, lds, dev_out, ldo, stream);
}

}  // extern "C"
