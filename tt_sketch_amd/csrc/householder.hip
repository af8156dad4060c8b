// ttsk_qr_thin: Householder thin QR of the tall-skinny Psi unfolding (sketch_dispatch.py:172), row blocks spread over the
// whole chip, two launches per column, LAPACK dlarfg sign convention -- the robust path behind CholeskyQR2 (cholesky.hip).
#include "solver.h"

namespace ttsk {

// ---------------------------------------------------------------- Householder QR
struct Refl { double tau, scale, beta; };
__device__ __forceinline__ Refl make_refl(double alpha, double xnorm2)
{
    // LAPACK dlarfg: x = (alpha, tail), xnorm2 = |tail|^2
    Refl h;
    if (xnorm2 == 0.0) { h.tau = 0.0; h.scale = 0.0; h.beta = alpha; return h; }
    double nrm = sqrt(alpha * alpha + xnorm2);
    h.beta = alpha >= 0 ? -nrm : nrm;
    h.tau = (h.beta - alpha) / h.beta;
    h.scale = 1.0 / (alpha - h.beta);
    return h;
}

constexpr int QR_ROWS = 128;  // rows per workgroup

// All cross-workgroup reductions of the QR go through per-workgroup partial slots that the
// NEXT launch sums in a fixed order: no atomics, bit-reproducible results.
//   tpart[b]        partial of the tail norm^2 of the current pivot column (nb_t slots)
//   wpart[b*n + k]  partial of w[k] = sum_i v_i M[i][k]                     (nb_w slots)
__device__ __forceinline__ double sum_slots(const double *p, int nslots, int stride)
{
    double s = 0;
    for (int b = 0; b < nslots; ++b) s += p[(size_t)b * stride];
    return s;
}

// tpart[b] = sum_{i in block b, i>j} A[i][j]^2 ; block b covers rows j + 128 b ...
__global__ __launch_bounds__(256) void qr_tail_norm_kernel(const double *A, int64_t m, int64_t n, int64_t j,
                                                           double *tpart)
{
    const int64_t r0 = j + (int64_t)blockIdx.x * QR_ROWS;
    const int64_t r1 = r0 + QR_ROWS < m ? r0 + QR_ROWS : m;
    __shared__ double red[4];
    double acc = 0;
    for (int64_t i = r0 + threadIdx.x; i < r1; i += blockDim.x)
        if (i > j) { double x = A[i * n + j]; acc = fma(x, x, acc); }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    // left to right, unlike block_total; kept for bit-compatibility
    if (threadIdx.x == 0) tpart[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// wpart[b][k] = sum_{i in block b} v_i * M[i][k], k in [k0, n); v from column j of A.
__global__ __launch_bounds__(256) void qr_w_kernel(const double *A, const double *M, int64_t m, int64_t n,
                                                   int64_t j, int64_t k0, const double *tpart, int nb_t,
                                                   double *wpart)
{
    const Refl h = make_refl(A[j * n + j], sum_slots(tpart, nb_t, 1));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = j + (int64_t)blockIdx.x * QR_ROWS;
    const int64_t r1 = r0 + QR_ROWS < m ? r0 + QR_ROWS : m;
    __shared__ double red[4][64];
    for (int64_t kb = k0; kb < n; kb += 64) {
        const int64_t k = kb + lane;
        double acc = 0;
        if (k < n && h.tau != 0.0)
            for (int64_t i = r0 + wave; i < r1; i += 4) {
                double v = (i == j) ? 1.0 : A[i * n + j] * h.scale;
                acc = fma(v, M[i * n + k], acc);
            }
        red[wave][lane] = acc;
        __syncthreads();
        if (wave == 0 && k < n)
            wpart[(size_t)blockIdx.x * n + k] = red[0][lane] + red[1][lane] + red[2][lane] + red[3][lane];
        __syncthreads();
    }
}

// M[i][k] -= tau * v_i * w[k] for i>=j, k in [k0,n); optionally the tail norm partials of
// column j+1 of M (rows > j+1) for the next reflector go to next_tpart[b].
__global__ __launch_bounds__(256) void qr_update_kernel(const double *A, double *M, int64_t m, int64_t n,
                                                        int64_t j, int64_t k0, const double *tpart, int nb_t,
                                                        const double *wpart, int nb_w, double *next_tpart)
{
    const Refl h = make_refl(A[j * n + j], sum_slots(tpart, nb_t, 1));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = j + (int64_t)blockIdx.x * QR_ROWS;
    const int64_t r1 = r0 + QR_ROWS < m ? r0 + QR_ROWS : m;
    __shared__ double red[4];
    double nacc = 0;
    for (int64_t kb = k0; kb < n; kb += 64) {
        const int64_t k = kb + lane;
        if (k >= n) continue;
        const double tw = h.tau * sum_slots(wpart + k, nb_w, (int)n);
        for (int64_t i = r0 + wave; i < r1; i += 4) {
            double v = (i == j) ? 1.0 : A[i * n + j] * h.scale;
            double x = M[i * n + k];
            if (h.tau != 0.0) { x = fma(-tw, v, x); M[i * n + k] = x; }
            if (next_tpart && k == j + 1 && i > j + 1) nacc = fma(x, x, nacc);
        }
    }
    if (next_tpart) {
        nacc = wave_sum(nacc);
        if (lane == 0) red[wave] = nacc;
        __syncthreads();
        // left to right, unlike block_total; kept for bit-compatibility
        if (threadIdx.x == 0) next_tpart[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
    }
}

__global__ void eye_kernel(double *Q, int64_t m, int64_t n)
{
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m * n;
         t += (int64_t)gridDim.x * blockDim.x)
        Q[t] = (t / n == t % n) ? 1.0 : 0.0;
}

__global__ void triu_kernel(double *A, int64_t m, int64_t n)
{
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < m * n;
         t += (int64_t)gridDim.x * blockDim.x)
        if (t % n < t / n) A[t] = 0.0;
}

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_triu(double *A, int64_t m, int64_t n, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(A && m >= 1 && n >= 1, "ttsk_triu: bad argument");
    const int64_t blocks = cdiv(m * n, 256);
    return launch(triu_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(256), 0, st, A, m, n);
}

int ttsk_qr_thin(double *A, int64_t m, int64_t n, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(A, "ttsk_qr_thin: NULL argument");
    TTSK_ARG(m >= n && n >= 1, "ttsk_qr_thin: need m >= n >= 1, got (%lld, %lld)", (long long)m,
             (long long)n);
    const int fr = qr_cholesky(A, m, n, stream, st);
    if (fr < 0) return fr;
    if (fr == 1) return TTSK_OK;
    // scratch: tpart[n][nb] (tail-norm partials per pivot column), wpart[nb][n], Q[m*n]
    const int64_t nb = cdiv(m, QR_ROWS);
    const size_t small = (size_t)n * nb + (size_t)nb * n;
    double *ws = (double *)scratch(stream, SCRATCH_MISC, (small + (size_t)m * n) * 8);
    if (!ws) return TTSK_ERR_HIP;
    double *tpart = ws, *wpart = ws + (size_t)n * nb, *Q = ws + small;
    auto blocks_at = [&](int64_t j) { return (int)cdiv(m - j, QR_ROWS); };
    int rc;
    if ((rc = launch(qr_tail_norm_kernel, dim3(blocks_at(0)), dim3(256), 0, st, A, m, n, (int64_t)0, tpart))) return rc;
    // factorisation: reflector j from column j applied to columns j+1..n-1; the update of
    // column j also leaves the tail-norm partials of column j+1 in tpart[j+1][*]
    for (int64_t j = 0; j + 1 < n; ++j) {
        const int nbj = blocks_at(j);
        if ((rc = launch(qr_w_kernel, dim3(nbj), dim3(256), 0, st, A, A, m, n, j, j + 1, tpart + j * nb,
                         blocks_at(j > 0 ? j - 1 : 0), wpart))) return rc;
        if ((rc = launch(qr_update_kernel, dim3(nbj), dim3(256), 0, st, A, A, m, n, j, j + 1,
                         tpart + j * nb, blocks_at(j > 0 ? j - 1 : 0), wpart, nbj, tpart + (j + 1) * nb))) return rc;
    }
    // Q = H_0 H_1 ... H_{n-1} [I; 0]
    if ((rc = launch(eye_kernel, dim3(1024), dim3(256), 0, st, Q, m, n))) return rc;
    for (int64_t j = n - 1; j >= 0; --j) {
        const int nbj = blocks_at(j);
        const int nbt = blocks_at(j > 0 ? j - 1 : 0);
        if ((rc = launch(qr_w_kernel, dim3(nbj), dim3(256), 0, st, A, Q, m, n, j, j, tpart + j * nb, nbt, wpart))) return rc;
        if ((rc = launch(qr_update_kernel, dim3(nbj), dim3(256), 0, st, A, Q, m, n, j, j, tpart + j * nb, nbt,
                         wpart, nbj, (double *)nullptr))) return rc;
    }
    TTSK_HIP(hipMemcpyAsync(A, Q, (size_t)m * n * 8, hipMemcpyDeviceToDevice, st));
    return TTSK_OK;
}

}  // extern "C"
