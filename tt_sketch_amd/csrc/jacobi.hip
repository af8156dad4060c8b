// The one-workgroup Jacobi SVD of the sketch path.
//
//  ttsk_pinv's robust path: pinv(Omega) with gelsd's truncation rule (utils.py:98-109), one-sided Jacobi SVD of the tall
//  orientation of Omega inside ONE workgroup (Omega is l x r with l, r of order 10..300: a few tens of KB); queued behind
//  the normal-equations attempt of pinv.hip, predicated on its verdict.  ttsk_svd_small: the factors themselves.
#include <cfloat>
#include <cmath>
#include "jacobi_pair.h"

namespace ttsk {

// Householder QR of Wc (column-major mW x nW, mW >= nW) in place, R only: afterwards the leading nW x nW block
// holds R^T (lower triangular, i.e. column j = row j of R) and nothing else of Wc is meaningful.  One barrier pair
// per column; every 16-lane group recomputes the reflector of column j itself and applies it to its own columns.
__device__ void jac_qr_rt(double *Wc, const int mW, const int nW, const int tid, const int nthreads, double *s_beta)
{
    const int grp = tid >> 4, gl = tid & 15, ngrp = nthreads >> 4;
    for (int j = 0; j < nW; ++j) {
        const double *cj = Wc + (size_t)j * mW;
        double sig = 0.0;
        for (int i = j + 1 + gl; i < mW; i += 16) sig = fma(cj[i], cj[i], sig);
        sig = row_sum16(sig);
        const double alpha = cj[j];
        double beta = alpha, tau = 0.0, scale = 0.0;
        if (sig != 0.0) {                                              // LAPACK dlarfg
            const double nrm = sqrt(alpha * alpha + sig);
            beta = alpha >= 0 ? -nrm : nrm;
            tau = (beta - alpha) / beta;
            scale = 1.0 / (alpha - beta);
        }
        for (int k = j + 1 + grp; k < nW; k += ngrp) {
            double *ck = Wc + (size_t)k * mW;
            double w = gl == 0 ? ck[j] : 0.0;                          // v[0] = 1
            for (int i = j + 1 + gl; i < mW; i += 16) w = fma(cj[i] * scale, ck[i], w);
            w = row_sum16(w) * tau;
            if (gl == 0) ck[j] -= w;
            for (int i = j + 1 + gl; i < mW; i += 16) ck[i] = fma(-w, cj[i] * scale, ck[i]);
        }
        if (tid == 0) *s_beta = beta;
        __syncthreads();
        for (int i = j + tid; i < mW; i += nthreads) Wc[(size_t)j * mW + i] = i == j ? *s_beta : 0.0;
        __syncthreads();
    }
    // R (upper triangle of the leading block) -> R^T
    for (int t = tid; t < nW * nW; t += nthreads) {
        const int j = t / nW, i = t - j * nW;
        if (i < j) { Wc[(size_t)i * mW + j] = Wc[(size_t)j * mW + i]; Wc[(size_t)j * mW + i] = 0.0; }
    }
    __syncthreads();
}

// ---------------------------------------------------------------- Jacobi SVD pinv
// W: mW x nW (mW >= nW) column-major in Wc (column j at Wc + j*mW), V: nW x nW column-major.
// On exit P[i*ldp_i + k*ldp_k] = sum_{j kept} Wc_j[i] * V_j[k] / sigma_j^2.
// With svd_US != nullptr the kernel returns the factors instead of the pseudo-inverse (input taken
// untransposed, l >= r): US (l x r row-major) = U diag(S), S (r) descending, Vt (r x r row-major).
template <int LM>
__global__ __launch_bounds__(1024) void jacobi_pinv_kernel(const double *__restrict__ omega, int64_t l,
                                                           int64_t r, int transposed, double *Wc,
                                                           double *V, double rcond, double *P,
                                                           int *rank_out, double *svd_US,
                                                           double *svd_S, double *svd_Vt,
                                                           const int *run_if_nonzero = nullptr, int64_t om_stride = 0,
                                                           int64_t p_stride = 0)
{
    // a batch of equally spaced matrices: workgroup b takes matrix b (grid 1, strides 0: the plain call)
    omega += (int64_t)blockIdx.x * om_stride;
    P += (int64_t)blockIdx.x * p_stride;
    if (run_if_nonzero) run_if_nonzero += blockIdx.x;
    // queued behind the normal-equations attempt without the host having looked at its verdict (ttsk_pinv_end):
    // nothing to do if that attempt was accepted
    if (run_if_nonzero && *run_if_nonzero == 0) return;
    const int mW = (int)(transposed ? r : l), nW = (int)(transposed ? l : r);
    // LM = 1: W lives in LDS, 2: W and V (the global scratch is then unused).  A template parameter, not a
    // run-time switch: a pointer that may be LDS or global compiles to FLAT loads and stores (67 + 54 of them
    // in this kernel), several times slower than ds_read / ds_write for data that is in LDS.
    // All LDS is dynamic: [sigma^2 (nW doubles) | order (nW ints, padded) | W | V], so that a 100 x 100
    // factor (2 x 80 KB) still fits next to them in the 160 KB of a CU.
    extern __shared__ double jac_lds[];
    double *s_inv2 = jac_lds;
    int *s_ord = reinterpret_cast<int *>(jac_lds + nW);
    double *jac_mat = jac_lds + nW + (nW + 1) / 2;
    if constexpr (LM >= 1) Wc = jac_mat;
    if constexpr (LM >= 2) V = jac_mat + (size_t)mW * nW;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwave = blockDim.x >> 6;
    __shared__ int s_rot;
    __shared__ double s_smax;
    const int grp = tid >> 4, gl = tid & 15, ngrp = blockDim.x >> 4;
    // load: W = Omega^T (transposed) or Omega
    for (int t = tid; t < mW * nW; t += blockDim.x) {
        int j = t / mW, i = t - j * mW;
        Wc[t] = transposed ? omega[(int64_t)j * r + i] : omega[(int64_t)i * r + j];
    }
    for (int t = tid; t < nW * nW; t += blockDim.x) V[t] = (t / nW == t % nW) ? 1.0 : 0.0;
    __syncthreads();
    // Pseudo-inverse mode: QR first, then the sweeps run on R^T (nW x nW, lower triangular) without accumulating V
    // (dgejsv's preconditioning: Jacobi on the transposed triangular factor needs fewer sweeps -- 15 -> 10 for a
    // rank-15 100 x 50 sketch -- and the columns are nW instead of mW long).  The right singular vectors are then
    // the normalised columns of the converged matrix, and W V is recomputed from the input.  1.1 -> 0.54 ms for that
    // sketch; the factor mode (svd_US) keeps the plain iteration with its high relative accuracy.
    const bool precond = svd_US == nullptr;
    __shared__ double s_beta;
    if (precond) jac_qr_rt(Wc, mW, nW, tid, blockDim.x, &s_beta);
    const int rows = precond ? nW : mW;          // length of the columns the sweeps rotate (column stride stays mW)
    const int np = nW + (nW & 1);  // players (one dummy if odd)
    // LAPACK dgesvj stops at sqrt(m) eps: the computed inner product of two columns of length m carries that
    // much rounding noise, a tighter bound keeps rotating noise until the sweep limit
    const double tol = fmax(4.0, sqrt((double)mW)) * DBL_EPSILON, tol2 = tol * tol;
    const int nm1 = np - 1;
    const int itc = rows <= 64 ? 4 : (rows <= 128 ? 8 : 0);   // mW >= nW
    // Pseudo-inverse mode ends with ONE closing sweep that rotates every pair (tolerance 0).  The sweeps stop with cosines of up
    // to tol left between the columns, and the sigma^-2 weights below turn a cosine c between a large and a small singular
    // direction into a relative error c kappa of the result: 11 kappa eps at 150 x 128, 17 kappa eps at 200 x 64 (kappa = 3000;
    // 37 and 11 times gelsd's error, tests/test_gpu_solve_edges.py).  Jacobi converges quadratically, so one more sweep takes the
    // cosines from tol to rounding level: 5 and 3 kappa eps, for one sweep in about ten.
    bool closing = false;
    for (int sweep = 0; sweep < 60; ++sweep) {
        const double swtol2 = closing ? 0.0 : tol2;
        if (tid == 0) { s_rot = 0; s_smax = 0.0; }
        __syncthreads();
        // largest column norm^2 of this sweep (fixed reduction order: per-column sums, then one thread)
        for (int j = grp; j < nW; j += ngrp) {
            const double *wj = Wc + (size_t)j * mW;
            double a = 0;
            for (int i = gl; i < rows; i += 16) a = fma(wj[i], wj[i], a);
            a = row_sum16(a);
            if (gl == 0) s_inv2[j] = a;
        }
        __syncthreads();
        if (tid == 0) {
            double mx = 0;
            for (int j = 0; j < nW; ++j) mx = fmax(mx, s_inv2[j]);
            s_smax = mx;
        }
        __syncthreads();
        const double tiny = 4.0 * mW * DBL_EPSILON, tiny2 = tiny * tiny * s_smax;
        for (int round = 0; round < np - 1; ++round) {
            // one column pair per group of 16 lanes (a DPP row): 64 pairs of a round rotate at once and the
            // three inner products are reduced by four in-register row rotations.  (A whole wave per pair was
            // four sequential pair steps per round at n = 100, each paying six ds_bpermute stages.)
            for (int pi = grp; pi < np / 2; pi += ngrp) {
                int p, q;
                if (pi == 0) { p = nm1; q = round; }
                else {
                    p = round + pi; p -= p >= nm1 ? nm1 : 0;
                    q = round + nm1 - pi; q -= q >= nm1 ? nm1 : 0;
                }
                if (p >= nW || q >= nW) continue;
                if (p > q) { int t = p; p = q; q = t; }
                double *wp = Wc + (size_t)p * mW, *wq = Wc + (size_t)q * mW;
                double *vp = V + (size_t)p * nW, *vq = V + (size_t)q * nW;
                if (precond) {
                    if (itc == 4) jac_pair<4, false>(wp, wq, vp, vq, rows, nW, gl, swtol2, tiny2, &s_rot);
                    else if (itc == 8) jac_pair<8, false>(wp, wq, vp, vq, rows, nW, gl, swtol2, tiny2, &s_rot);
                    else jac_pair<0, false>(wp, wq, vp, vq, rows, nW, gl, swtol2, tiny2, &s_rot);
                } else if (itc == 4) jac_pair<4>(wp, wq, vp, vq, mW, nW, gl, tol2, tiny2, &s_rot);
                else if (itc == 8) jac_pair<8>(wp, wq, vp, vq, mW, nW, gl, tol2, tiny2, &s_rot);
                else jac_pair<0>(wp, wq, vp, vq, mW, nW, gl, tol2, tiny2, &s_rot);
            }
            __syncthreads();
        }
        const int rot = s_rot;
        __syncthreads();
        if (closing) break;
        if (!rot) {
            if (!precond) break;
            closing = true;
        }
    }
    if (precond) {
        // V_j = column j of the converged R^T V' over its norm (zero for a column that vanished), then W V from the input
        for (int j = grp; j < nW; j += ngrp) {
            const double *wj = Wc + (size_t)j * mW;
            double a = 0;
            for (int i = gl; i < rows; i += 16) a = fma(wj[i], wj[i], a);
            a = row_sum16(a);
            if (gl == 0) s_inv2[j] = a;
        }
        __syncthreads();
        for (int t = tid; t < nW * nW; t += blockDim.x) {
            const int j = t / nW, k = t - j * nW;
            V[t] = s_inv2[j] > 0.0 ? Wc[(size_t)j * mW + k] / sqrt(s_inv2[j]) : 0.0;
        }
        __syncthreads();
        for (int t = tid; t < mW * nW; t += blockDim.x) {
            const int j = t / mW, i = t - j * mW;
            const double *vj = V + (size_t)j * nW;
            double acc = 0.0;
            if (transposed) for (int k = 0; k < nW; ++k) acc = fma(omega[(int64_t)k * r + i], vj[k], acc);
            else for (int k = 0; k < nW; ++k) acc = fma(omega[(int64_t)i * r + k], vj[k], acc);
            Wc[t] = acc;
        }
        __syncthreads();
    }
    // singular values -> reuse the first nW entries of a shared array
    if (tid == 0) s_smax = 0.0;
    __syncthreads();
    for (int j = wave; j < nW; j += nwave) {
        double a = 0;
        const double *wj = Wc + (size_t)j * mW;
        for (int i = lane; i < mW; i += 64) a = fma(wj[i], wj[i], a);
        a = wave_sum(a);
        if (lane == 0) s_inv2[j] = a;  // sigma^2
    }
    __syncthreads();
    if (svd_US) {
        // order the columns by descending singular value (nW <= 1024, one thread)
        if (tid == 0) {
            for (int j = 0; j < nW; ++j) s_ord[j] = j;
            for (int a = 1; a < nW; ++a) {
                const int key = s_ord[a];
                const double kv = s_inv2[key];
                int b = a - 1;
                while (b >= 0 && s_inv2[s_ord[b]] < kv) { s_ord[b + 1] = s_ord[b]; --b; }
                s_ord[b + 1] = key;
            }
        }
        __syncthreads();
        for (int t = tid; t < mW * nW; t += blockDim.x) {
            const int i = t / nW, k = t - i * nW;
            svd_US[t] = Wc[(size_t)s_ord[k] * mW + i];
        }
        for (int t = tid; t < nW * nW; t += blockDim.x) {
            const int k = t / nW, i = t - k * nW;
            svd_Vt[t] = V[(size_t)s_ord[k] * nW + i];
        }
        for (int k = tid; k < nW; k += blockDim.x) svd_S[k] = sqrt(s_inv2[s_ord[k]]);
        return;
    }
    if (tid == 0) {
        double mx = 0;
        for (int j = 0; j < nW; ++j) mx = fmax(mx, s_inv2[j]);
        s_smax = sqrt(mx);
        int rk = 0;
        const double thr = rcond * s_smax;
        for (int j = 0; j < nW; ++j) {
            double sg = sqrt(s_inv2[j]);
            if (sg > thr && sg > 0.0) { s_inv2[j] = 1.0 / s_inv2[j]; ++rk; }
            else s_inv2[j] = 0.0;
        }
        if (rank_out) *rank_out = rk;
    }
    __syncthreads();
    // P (r x l row-major): transposed -> P[i][k] (i<mW=r, k<nW=l); else P[k][i] (k<nW=r, i<mW=l)
    for (int t = tid; t < mW * nW; t += blockDim.x) {
        int i = t / nW, k = t - i * nW;
        double acc = 0;
        for (int j = 0; j < nW; ++j) acc = fma(Wc[(size_t)j * mW + i] * s_inv2[j], V[(size_t)j * nW + k], acc);
        if (transposed) P[(int64_t)i * l + k] = acc;
        else P[(int64_t)k * l + i] = acc;
    }
}

// where the Jacobi working set lives: 2 = W and V in LDS, 1 = W only, 0 = global scratch
static int jacobi_lds_mode(int64_t mW, int64_t nW, size_t *bytes)
{
    const size_t cap = 160 * 1024 - 256;            // 160 KB per CU minus the kernel's few static bytes
    const size_t w = (size_t)mW * nW * 8, v = (size_t)nW * nW * 8;
    const size_t small = ((size_t)nW + (nW + 1) / 2) * 8;          // sigma^2 and the sort order
    if (small + w + v <= cap) { *bytes = small + w + v; return 2; }
    if (small + w <= cap) { *bytes = small + w; return 1; }
    *bytes = small;
    return 0;
}

bool jacobi_fits_lds(int64_t mW, int64_t nW)
{
    size_t bytes = 0;
    return jacobi_lds_mode(mW, nW, &bytes) == 2;
}

int launch_jacobi(int count, const double *omega, int64_t l, int64_t r, int transposed, double *Wc, double *V, double rcond,
                  double *P, int *rank_out, double *svd_US, double *svd_S, double *svd_Vt, const int *run_if_nonzero,
                  int64_t om_stride, int64_t p_stride, hipStream_t st)
{
    size_t jl = 0;
    const int jm = jacobi_lds_mode(transposed ? r : l, transposed ? l : r, &jl);
    auto kern = jm == 2 ? jacobi_pinv_kernel<2> : (jm == 1 ? jacobi_pinv_kernel<1> : jacobi_pinv_kernel<0>);
    return launch(kern, dim3((unsigned)count), dim3(1024), jl, st, omega, l, r, transposed, Wc, V, rcond, P, rank_out, svd_US, svd_S,
                  svd_Vt, run_if_nonzero, om_stride, p_stride);
}

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_svd_small(const double *dev_A, int64_t m, int64_t n, double *dev_US, double *dev_S, double *dev_Vt,
                   int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(dev_A && dev_US && dev_S && dev_Vt, "ttsk_svd_small: NULL argument");
    TTSK_ARG(m >= n && n >= 1 && n <= 8192 && m <= (1 << 20), "ttsk_svd_small: need m >= n, 1 <= n <= 8192, got (%lld, %lld)",
             (long long)m, (long long)n);
    // beyond one workgroup's reach: the whole-chip kernel of svd_grid.hip
    if (n > 1024) return svd_jacobi_grid(dev_A, m, n, dev_US, dev_S, dev_Vt, stream, st);
    double *ws = (double *)scratch(stream, SCRATCH_MISC, (size_t)(m * n + n * n) * 8);
    if (!ws) return TTSK_ERR_HIP;
    return launch_jacobi(1, dev_A, m, n, 0, ws, ws + m * n, 0.0, nullptr, nullptr, dev_US, dev_S, dev_Vt, nullptr, 0, 0, st);
}

}  // extern "C"
