// The Cholesky family of the sketch path's small dense solves.
//
//  chol_inv_kernel   G = R^T R and R^-1 (optionally G^-1) of a small symmetric matrix in one workgroup, with a verdict
//                    (rejected: not positive definite, or diag(R) spread beyond the caller's gate); chol_inv_any takes it
//                    to n = 256 by a 2 x 2 block factorisation.
//  qr_cholesky       thin QR by CholeskyQR2 (one launch for a small tall matrix: cholqr2_lds_kernel; small_qr_kernel, a
//                    one-workgroup Householder QR, for a small nearly square one) with LAPACK's Householder column signs
//                    reconstructed from a modified LU of the top block of Q (hh_signs_lds, qr_signs), and the same steps for
//                    up to QR_BATCH_MAX matrices of one shape per launch (qr_cholesky_batch, qr_signs_batch, apply_signs).
#include <cfloat>
#include <cmath>
#include "skinny.h"
#include "solver.h"

namespace ttsk {

constexpr int CHOL_SIGN_MAX = 72;             // second factorisation + sign reconstruction in one kernel: three n x (n + 1) images in LDS
constexpr size_t SMALL_QR_MAX = 19000;      // doubles of LDS the one-workgroup Householder QR may take (152 KB)

// Both solves of the path are overwhelmingly applied to well-conditioned matrices: Omega is an
// (l x r) sketch of full row or column rank, and the matrix orth_step factorises is Psi Omega^+.
// For those, pinv(Omega) = Omega^T (Omega Omega^T)^-1 and the thin QR by CholeskyQR2 are a handful
// of products on the chain kernels plus an n x n Cholesky in one workgroup (n <= 128) -- ~0.1 ms
// instead of 2 ms (one-workgroup Jacobi SVD) and 8 ms (4 n Householder launches) at C3.  The
// Cholesky kernel reports failure (not positive definite, or diag(R) spread beyond cond_tol) and the
// callers then run the robust kernels above on the untouched input, so rank-deficient sketches
// behave exactly as before.
// G (n x n symmetric, row-major) = R^T R; Rinv = R^-1 (upper triangular, dense n x n) and optionally
// Ginv = Rinv Rinv^T = G^-1.  status[0] = 0 ok, 1 rejected.
__device__ void hh_signs_lds(double *B, int n, int ld, int square, double *S, double *shadow, int tid, int nthr = 256);

// Qtop (optional, n <= CHOL_SIGN_MAX): the call is the SECOND factorisation of CholeskyQR2 -- the kernel goes on to form
// the top n x n block of Q = Qtop R^-1 in LDS, reconstructs LAPACK's Householder column signs from it (hh_signs_lds)
// and writes Rinv with its columns scaled by them: three launches of qr_cholesky in one.
// sticky (optional): set to 1 on rejection, never cleared here (deferred verdicts: ttsk_orth_step);
// pminmax (optional): smallest / largest pivot, for callers that combine several blocks (chol_inv_any).
// The factorisation and the inverse of chol_inv_kernel on a matrix that sits in LDS (A: n x n with row stride ld, both
// triangles; xd: n doubles): afterwards X = R^-1 is stored with its strict upper part transposed into A's lower
// triangle (X[i][c], i < c, at A[c][i]) and its diagonal in xd.  Every thread of the workgroup calls it (barriers
// inside); threads beyond the first 256 take part in the recurrence only.  bad / pmin / pmax: the verdict's inputs
// (every thread has them).
__device__ __forceinline__ void chol_lds(double *A, double *xd, const int n, const int ld, double *shadow, const int tid,
                                         const int nthr, int &bad, double &pmin, double &pmax)
{
    const bool core = tid < 256;
    const int ti = tid >> 4, tc = tid & 15, nrow = nthr >> 4;
    auto rcp2 = [](double x) { double r = __builtin_amdgcn_rcp(x); r = r * (2.0 - x * r); return r * (2.0 - x * r); };
    int j = 0;
    for (; j + 1 < n; j += 2) {
        const double *r0 = A + j * ld, *r1 = A + (j + 1) * ld;
        double p0 = r0[j];
        if (!(p0 > 0.0)) { bad = 1; p0 = 1.0; }
        const double pi0 = rcp2(p0);
        const double g = r0[j + 1] * pi0;                      // factor of row j + 1 against row j
        double p1 = fma(-g, r0[j + 1], r1[j + 1]);             // pivot of column j + 1 after step j
        if (!(p1 > 0.0)) { bad = 1; p1 = 1.0; }
        const double pi1 = rcp2(p1);
        pmin = fmin(pmin, fmin(p0, p1));
        pmax = fmax(pmax, fmax(p0, p1));
        for (int i = j + 2 + ti; i < n; i += nrow) {
            const double a0 = r0[i], a1 = fma(-g, a0, r1[i]);  // A[j][i] and A[j+1][i] after step j
            const double f0 = a0 * pi0, f1 = a1 * pi1;
            for (int c = i + tc; c < n; c += 16) {
                const double u1 = fma(-g, r0[c], r1[c]);       // row j + 1 after step j, at c
                A[i * ld + c] = fma(-f1, u1, fma(-f0, r0[c], A[i * ld + c]));
            }
        }
        double *sh = shadow + ((j >> 1) & 1) * 128;
        for (int c = j + 1 + tid; c < n; c += nthr) sh[c] = fma(-g, r0[c], r1[c]);
        __syncthreads();
        for (int c = j + 1 + tid; c < n; c += nthr) A[(j + 1) * ld + c] = sh[c];
    }
    __syncthreads();
    if (j < n) {                                               // odd n: the last pivot
        double piv = A[j * ld + j];
        if (!(piv > 0.0)) { bad = 1; piv = 1.0; }
        pmin = fmin(pmin, piv);
        pmax = fmax(pmax, piv);
    }
    // R[j][c] = row j / r_j; xd[j] = 1 / R[j][j] = 1 / r_j
    if (core && tid < n) xd[tid] = 1.0 / sqrt(A[tid * ld + tid] > 0.0 ? A[tid * ld + tid] : 1.0);
    __syncthreads();
    if (core)
        for (int jj = ti; jj < n; jj += 16) {
            const double sc = xd[jj];
            for (int c = jj + tc; c < n; c += 16) A[jj * ld + c] *= sc;
        }
    __syncthreads();
    // X = R^-1 stays in LDS: its strict upper part X[i][c] (i < c) goes to the unused strict lower triangle of A at
    // A[c][i], its diagonal to xd[].
    // X = R^-1 in 16 x 16 blocks.  (1) The diagonal blocks, all at once: a quad of lanes owns a column and walks the
    // (up to 15) rows of its own block -- one wavefront per 16 columns, in order, no workgroup barrier.  (2) Block rows
    // from the bottom: X_ij = -X_ii (sum_{i<k<=j} R_ik X_kj) on the matrix cores; the accumulator registers of the sum
    // are the B operand of the second product (register kb of a lane holds rows 4 kb + (lane >> 4): exactly k-block
    // kb); one barrier per block row.  (One column per quad over ALL rows was 42 k of the kernel's 118 k cycles at
    // n = 50 -- 900 cycles of dependent LDS reads per row -- and 152 k of 396 k at n = 100; now 20 k and 55 k.)
    const int q4 = tid & 3, col4 = tid >> 2;
    for (int c = core ? col4 : n; c < n; c += 64) {
        const double *xc = A + c * ld;                                  // X[k][c] at A[c][k], k < c
        const int top = c & ~15;
        for (int i = c - 1; i >= top; --i) {
            const double *ri = A + i * ld;
            double acc = 0.0;
            for (int k = i + 1 + q4; k < c; k += 4) acc = fma(ri[k], xc[k], acc);
            acc += jac_dpp<0xB1>(acc);              // quad_perm 1 0 3 2
            acc += jac_dpp<0x4E>(acc);              // quad_perm 2 3 0 1
            if (q4 == 0) A[c * ld + i] = -(acc + ri[c] * xd[c]) * xd[i];
        }
    }
    __syncthreads();
    {
        const int lane = tid & 63, wv = tid >> 6, x16 = lane & 15, kq = lane >> 4;
        const int nt = (n + 15) >> 4;
        // X(r, c), r <= c, from its storage: strict upper part transposed into the lower triangle, diagonal in xd
        auto Xat = [&](int r, int c) -> double {
            if (r >= n || c >= n || r > c) return 0.0;
            return r == c ? xd[c] : A[c * ld + r];
        };
        for (int bi = nt - 2; bi >= 0; --bi) {
            for (int bj = core ? bi + 1 + wv : nt; bj < nt; bj += 4) {
                v4d S = {0.0, 0.0, 0.0, 0.0};
                const int ra = 16 * bi + x16;
                for (int bk = bi + 1; bk <= bj; ++bk)
#pragma unroll
                    for (int kb = 0; kb < 4; ++kb) {
                        const int k = 16 * bk + 4 * kb + kq;
                        const double av = (ra < n && k < n) ? A[ra * ld + k] : 0.0;          // R[ra][k], k > ra
                        S = mfma16(av, Xat(k, 16 * bj + x16), S);
                    }
                v4d Xn = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int kb = 0; kb < 4; ++kb) Xn = mfma16(Xat(16 * bi + x16, 16 * bi + 4 * kb + kq), S[kb], Xn);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int r = 16 * bi + kq + 4 * jj, c = 16 * bj + x16;
                    if (r < n && c < n) A[c * ld + r] = -Xn[jj];
                }
            }
            __syncthreads();
        }
    }
}

// Launched with 256 threads, or with 1024 (n <= 128, chol_threads()): the extra twelve waves take part in the recurrence
// only -- one row per 16-lane group instead of four, twelve more waves to hide the LDS round trips behind -- and leave.
__global__ __launch_bounds__(1024) void chol_inv_kernel(const double *__restrict__ G, int n, double *__restrict__ Rinv,
                                                       double *__restrict__ Ginv, int *__restrict__ status,
                                                       double cond_tol, int *__restrict__ sticky, double *__restrict__ pminmax,
                                                       const double *__restrict__ Qtop = nullptr, int square = 0, int expand = 1)
{
    extern __shared__ double sm[];
    const int ld = n + 1, tid = threadIdx.x;
    // a batch of independent factorisations: workgroup b takes the matrices n * n * b further on (grid 1: the plain call)
    G += (size_t)blockIdx.x * n * n;
    Rinv += (size_t)blockIdx.x * n * n;
    if (Ginv) Ginv += (size_t)blockIdx.x * n * n;
    status += blockIdx.x;
    double *A = sm;
    double *xd = sm + n * ld;
    const int nthr = blockDim.x;
    const bool core = tid < 256;                       // the threads that run every phase
    for (int e = tid; e < n * n; e += nthr) A[(e / n) * ld + e % n] = G[e];
    __syncthreads();
    // Unscaled right-looking recurrence: row j keeps r_j R[j][:] (r_j^2 = pivot) until the end, the trailing update
    // divides by the pivot instead, every thread reads the pivots itself.  TWO columns per barrier: the pivot of
    // column j + 1 and its row after step j follow from rows j and j + 1 alone, so every thread forms them on the
    // fly and updates its elements with both columns at once; the updated row j + 1 goes through a shadow row (the
    // others still read the old one) and home after the barrier -- nobody reads it again before the scaling pass.
    // (History at n = 50: three barriers per column 75 us of 118; one per column 55 k cycles; two columns 42 k.)
    int bad = 0;
    double pmin = 1e300, pmax = 0.0;                 // pivots r_j^2: the square root is not needed in the loop
    const int ti = tid >> 4, tc = tid & 15, nrow = nthr >> 4;
    // hardware reciprocal + two Newton steps (a full division is ~4x the instructions, on the critical path)
    auto rcp2 = [](double x) { double r = __builtin_amdgcn_rcp(x); r = r * (2.0 - x * r); return r * (2.0 - x * r); };
    __shared__ double shadow[2 * 128];
    int j = 0;
    bool expanded = false;
    if ((Qtop && expand) || expand == 2) {                  // expand == 2: a second factorisation whose signs come later
        // The second factorisation of CholeskyQR2 sees G = I + E with |E| ~ n kappa(A)^2 eps.  For n max|E| <= 1e-8 the
        // factor's inverse is I - Phi(E) (Phi: strict upper triangle + half the diagonal) to within n |E|^2 < 1e-17:
        // no recurrence at all (n / 2 steps of ~1600 cycles otherwise).
        double em = 0.0;
        if (core) {
            for (int e = tid; e < n * n; e += 256) {
                const int i = e / n, c = e - i * n;
                em = nan_max(em, fabs(A[i * ld + c] - (i == c ? 1.0 : 0.0)));
            }
            em = nan_max(em, jac_dpp<0xB1>(em));
            em = nan_max(em, jac_dpp<0x4E>(em));
            if ((tid & 3) == 0) shadow[tid >> 2] = em;
        }
        __syncthreads();
        em = 0.0;
        for (int k = 0; k < 64; ++k) em = nan_max(em, shadow[k]);
        __syncthreads();
        // nan_max keeps a NaN (fmax would drop it and a Gram matrix full of NaN would pass as the identity): NaN compares
        // false here and the recurrence below rejects it
        if (em * n <= 1e-8) {
            if (core)
                for (int e = tid; e < n * n; e += 256) {
                    const int i = e / n, c = e - i * n;
                    if (i < c) A[c * ld + i] = -A[i * ld + c];      // X[i][c] lives at A[c][i]
                    else if (i == c) xd[c] = 1.0 - 0.5 * (A[i * ld + i] - 1.0);
                }
            if (tid == 0) status[0] = 0;
            __syncthreads();
            expanded = true;
        }
    }
    if (expanded && !core) return;
    if (!expanded) {
    chol_lds(A, xd, n, ld, shadow, tid, nthr, bad, pmin, pmax);
    if (!core) return;
    if (tid == 0) {
        const int rej = (bad || pmin < cond_tol * cond_tol * pmax) ? 1 : 0;
        status[0] = rej;
        if (rej && sticky) *sticky = 1;
        if (pminmax) { pminmax[0] = bad ? -1.0 : pmin; pminmax[1] = pmax; }
    }
    }   // !expanded
    // X(r, c) from that storage (zero below the diagonal): the results are written straight from it -- no pass that
    // makes X dense in LDS first
    auto Xe = [&](int r, int c) -> double {
        if (r >= n || c >= n || r > c) return 0.0;
        return r == c ? xd[c] : A[c * ld + r];
    };
    if (Qtop) {
        // top block of Q = Qtop X (X upper triangular), the signs of LAPACK's reflectors from its modified LU, Rinv = X S
        double *B = xd + n, *S = B + n * ld, *Qs = S + n;      // Qs: Qtop staged (one coalesced pass instead of n dependent loads per cell)
        for (int e = tid; e < n * n; e += 256) Qs[(e / n) * ld + e % n] = Qtop[e];
        __syncthreads();
        for (int e = tid; e < n * n; e += 256) {
            const int i = e / n, c = e - i * n;
            const double *qi = Qs + i * ld, *xc = A + c * ld;    // X[k][c], k < c, sits at A[c][k]; the diagonal in xd
            double acc = qi[c] * xd[c];
            for (int k = 0; k < c; ++k) acc = fma(qi[k], xc[k], acc);
            B[i * ld + c] = acc;
        }
        __syncthreads();
        hh_signs_lds(B, n, ld, square, S, shadow, tid);
        for (int i = ti; i < n; i += 16)
            for (int c = tc; c < n; c += 16) Rinv[i * n + c] = Xe(i, c) * S[c];
        return;
    }
    for (int i = ti; i < n; i += 16)
        for (int c = tc; c < n; c += 16) Rinv[i * n + c] = Xe(i, c);
    if (Ginv) {
        // G^-1 = X X^T on the matrix cores: tile (ta, tb), tb >= ta, one per wave and turn, mirrored on the way out;
        // X is upper triangular, so the sum over k starts at the column tile (22 k -> 11 k cycles at n = 50, 125 k ->
        // 30 k at n = 100 against one thread per element)
        const int lane = tid & 63, wv = tid >> 6, x16 = lane & 15, kq = lane >> 4;
        const int nt = (n + 15) >> 4, nkb = (n + 3) >> 2;
        int t = 0;
        for (int ta = 0; ta < nt; ++ta)
            for (int tb = ta; tb < nt; ++tb, ++t) {
                if ((t & 3) != wv) continue;
                v4d acc = {0.0, 0.0, 0.0, 0.0};
                const int ra = 16 * ta + x16, rb = 16 * tb + x16;
                for (int kb = 4 * tb; kb < nkb; ++kb) {
                    const int k = 4 * kb + kq;
                    acc = mfma16(Xe(ra, k), Xe(rb, k), acc);
                }
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int i = 16 * ta + kq + 4 * jj, c = 16 * tb + x16;
                    if (i < n && c < n) { Ginv[i * n + c] = acc[jj]; Ginv[c * n + i] = acc[jj]; }
                }
            }
    }
}

// Column signs that turn the Q of CholeskyQR (R with positive diagonal) into LAPACK's Householder Q:
// the modified LU of the top n x n block of Q (Ballard et al., "Reconstructing Householder vectors
// from TSQR"): S_j = -sgn(pivot_j); for a square matrix the last reflector is the identity.
// Scales the columns of Rinv (n x n) by S in place.
__device__ void hh_signs_lds(double *B, int n, int ld, int square, double *S, double *shadow, int tid, int nthr)
{
    // only the signs are needed: every thread derives the modified pivots itself and the trailing update uses the
    // unscaled columns; two columns per barrier as in chol_inv_kernel (row j + 1 after step j through a shadow row)
    const int ti = tid >> 4, tc = tid & 15, nrow = nthr >> 4;          // (every thread of the workgroup calls this: barriers inside)
    int j = 0;
    for (; j + 1 < n; j += 2) {
        const double *b0 = B + j * ld, *b1 = B + (j + 1) * ld;
        const double sgn0 = b0[j] >= 0.0 ? -1.0 : 1.0;
        const double pinv0 = 1.0 / (b0[j] - sgn0);
        const double g = b1[j] * pinv0;                                  // factor of row j + 1 against row j
        const double piv1 = fma(-g, b0[j + 1], b1[j + 1]);               // pivot of column j + 1 after step j
        double sgn1 = piv1 >= 0.0 ? -1.0 : 1.0;
        if (square && j + 1 == n - 1) sgn1 = -sgn1;
        const double pinv1 = 1.0 / (piv1 - sgn1);
        if (tid == 0) { S[j] = sgn0; S[j + 1] = sgn1; }
        for (int i = j + 2 + ti; i < n; i += nrow) {
            const double f0 = B[i * ld + j] * pinv0;
            const double f1 = fma(-f0, b0[j + 1], B[i * ld + j + 1]) * pinv1;
            for (int c = j + 2 + tc; c < n; c += 16) {
                const double u1 = fma(-g, b0[c], b1[c]);                 // row j + 1 after step j, at c
                B[i * ld + c] = fma(-f1, u1, fma(-f0, b0[c], B[i * ld + c]));
            }
        }
        double *sh = shadow + ((j >> 1) & 1) * 128;
        for (int c = j + 2 + tid; c < n; c += nthr) sh[c] = fma(-g, b0[c], b1[c]);
        __syncthreads();
        for (int c = j + 2 + tid; c < n; c += nthr) B[(j + 1) * ld + c] = sh[c];
    }
    __syncthreads();
    if (j < n) {                                                         // odd n: the last pivot
        double sgn = B[j * ld + j] >= 0.0 ? -1.0 : 1.0;
        if (square && j == n - 1) sgn = -sgn;
        if (tid == 0) S[j] = sgn;
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void hh_sign_scale_kernel(const double *__restrict__ Qtop, int n, int square,
                                                            double *__restrict__ Rinv)
{
    extern __shared__ double sm[];
    const int ld = n + 1, tid = threadIdx.x;
    double *B = sm, *S = sm + n * ld;
    __shared__ double shadow[2 * 128];
    for (int e = tid; e < n * n; e += 256) B[(e / n) * ld + e % n] = Qtop[e];
    __syncthreads();
    hh_signs_lds(B, n, ld, square, S, shadow, tid);
    for (int e = tid; e < n * n; e += 256) Rinv[e] *= S[e % n];
}

// Thin QR of a SMALL, nearly square matrix (m n doubles fit the LDS: the first mode of a sketch whose rank was trimmed to
// the mode size, m = n_0 rows) in one workgroup: Householder with LAPACK's dlarfg signs, Q formed in place as dorg2r does
// -- no condition gate (CholeskyQR2 gives up beyond kappa ~ 1e6, which a square unfolding Psi_0 Omega_0^+ reaches
// easily).  A (m, n) row-major in, Q (m, n) row-major out.  Column-major working copy; every 16-lane group applies a
// reflector to its own columns.
__global__ __launch_bounds__(1024) void small_qr_kernel(double *__restrict__ A, int m, int n)
{
    extern __shared__ double sq[];
    double *W = sq;                    // m x n column-major
    double *tau = sq + (size_t)m * n;  // n
    const int tid = threadIdx.x, grp = tid >> 4, gl = tid & 15, ngrp = 64;
    for (int e = tid; e < m * n; e += 1024) W[(size_t)(e % n) * m + e / n] = A[e];
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        double *cj = W + (size_t)j * m;
        double sig = 0.0;
        for (int i = j + 1 + gl; i < m; i += 16) sig = fma(cj[i], cj[i], sig);
        sig = row_sum16(sig);
        const double alpha = cj[j];
        double beta = alpha, t = 0.0, scale = 0.0;
        if (sig != 0.0) {                                              // LAPACK dlarfg
            const double nrm = sqrt(alpha * alpha + sig);
            beta = alpha >= 0 ? -nrm : nrm;
            t = (beta - alpha) / beta;
            scale = 1.0 / (alpha - beta);
        }
        for (int k = j + 1 + grp; k < n; k += ngrp) {
            double *ck = W + (size_t)k * m;
            double w = gl == 0 ? ck[j] : 0.0;                          // v[0] = 1
            for (int i = j + 1 + gl; i < m; i += 16) w = fma(cj[i] * scale, ck[i], w);
            w = row_sum16(w) * t;
            if (gl == 0) ck[j] -= w;
            for (int i = j + 1 + gl; i < m; i += 16) ck[i] = fma(-w, cj[i] * scale, ck[i]);
        }
        __syncthreads();
        for (int i = j + 1 + tid; i < m; i += 1024) cj[i] *= scale;    // v below the diagonal (v[0] = 1 implied); R is not kept
        if (tid == 0) tau[j] = t;
        __syncthreads();
    }
    // Q = H_0 ... H_{n-1} [I; 0] in place (dorg2r): from the last reflector to the first
    for (int j = n - 1; j >= 0; --j) {
        double *vj = W + (size_t)j * m;
        const double t = tau[j];
        for (int k = j + 1 + grp; k < n; k += ngrp) {                  // columns > j already hold columns of Q (zero above row j + 1)
            double *qk = W + (size_t)k * m;
            double w = 0.0;                                            // row j of column k is still zero
            for (int i = j + 1 + gl; i < m; i += 16) w = fma(vj[i], qk[i], w);
            w = row_sum16(w) * t;
            if (gl == 0) qk[j] = -w;
            for (int i = j + 1 + gl; i < m; i += 16) qk[i] = fma(-w, vj[i], qk[i]);
        }
        __syncthreads();
        for (int i = tid; i < m; i += 1024) vj[i] = i < j ? 0.0 : (i == j ? 1.0 - t : -t * vj[i]);
        __syncthreads();
    }
    for (int e = tid; e < m * n; e += 1024) A[e] = W[(size_t)(e % n) * m + e / n];
}

// The same signs for n beyond one workgroup's LDS (129..256): the working copy is B itself in global memory (L2), one
// column per step, 1024 threads.  Only the signs are needed, so the trailing update uses the unscaled columns.
__global__ __launch_bounds__(1024) void hh_sign_scale_global_kernel(double *__restrict__ B, int n, int square, double *__restrict__ Rinv)
{
    __shared__ double S[CHOL_MAX_N];
    const int tid = threadIdx.x;
    for (int j = 0; j < n; ++j) {
        const double piv = B[j * n + j];
        double sgn = piv >= 0.0 ? -1.0 : 1.0;
        if (square && j == n - 1) sgn = -sgn;
        if (tid == 0) S[j] = sgn;
        const double pinv = 1.0 / (piv - sgn);
        const int rem = n - j - 1;
        for (int e = tid; e < rem * rem; e += 1024) {
            const int i = j + 1 + e / rem, c = j + 1 + e % rem;
            B[i * n + c] = fma(-B[i * n + j] * pinv, B[j * n + c], B[i * n + c]);
        }
        __threadfence_block();
        __syncthreads();
    }
    for (int e = tid; e < n * n; e += 1024) Rinv[e] *= S[e % n];
}

static unsigned chol_threads(int n)
{
    return n <= CHOL_ONE_N ? 1024u : 256u;
}

int launch_chol(const double *G, int n, double *Rinv, double *Ginv, int *status, double cond_tol, hipStream_t st, int *sticky,
                double *pminmax, int count)
{
    return launch(chol_inv_kernel, dim3((unsigned)count), dim3(chol_threads(n)), (size_t)(n * (n + 1) + n) * 8, st, G, n, Rinv, Ginv, status,
                  cond_tol, sticky, pminmax, (const double *)nullptr, 0, 1);
}

// verdict of a two-block factorisation: both blocks accepted AND the pivots of the whole matrix within cond_tol
__global__ void chol_combine_kernel(const double *pm, const int *st2, double cond_tol, int *status, int *sticky)
{
    const double lo = fmin(pm[0], pm[2]), hi = fmax(pm[1], pm[3]);
    const int rej = (st2[0] || st2[1] || !(lo > 0.0) || lo < cond_tol * cond_tol * hi) ? 1 : 0;
    status[0] = rej;
    if (rej && sticky) *sticky = 1;
}

// The same contract as chol_inv_kernel for n up to 256: beyond 128 (the one-workgroup kernel's LDS) a 2 x 2 block
// factorisation -- R11 = chol(G11), R12 = R11^-T G12, R22 = chol(G22 - R12^T R12), R^-1 = [X11, -X11 R12 X22; 0, X22] --
// i.e. two one-workgroup factorisations and a handful of small products (rank 145 / 290 of scripts/plot_timings.py).
// ws: chol_ws_elems(n) doubles from the caller's arena (nested scratch() calls would move it).
size_t chol_ws_elems(int n) { return n <= CHOL_ONE_N ? 0 : (size_t)6 * CHOL_ONE_N * CHOL_ONE_N + 16; }

int chol_inv_any(const double *G, int n, double *Rinv, double *Ginv, int *status, double cond_tol, int stream, hipStream_t st,
                 double *ws, int *sticky)
{
    if (n <= CHOL_ONE_N) return launch_chol(G, n, Rinv, Ginv, status, cond_tol, st, sticky);
    if (n > CHOL_MAX_N || !ws) return TTSK_ERR_UNSUPPORTED;
    const int n1 = ((n + 1) / 2 + 15) & ~15, n2 = n - n1;
    double *G11 = ws, *X11 = G11 + (size_t)n1 * n1, *R12 = X11 + (size_t)n1 * n1, *S = R12 + (size_t)n1 * n2;
    double *X22 = S + (size_t)n2 * n2, *Y = X22 + (size_t)n2 * n2, *pm = Y + (size_t)n1 * n2;
    int *st2 = (int *)(pm + 4);
    int rc;
    TTSK_HIP(hipMemcpy2DAsync(G11, (size_t)n1 * 8, G, (size_t)n * 8, (size_t)n1 * 8, n1, hipMemcpyDeviceToDevice, st));
    if ((rc = launch_chol(G11, n1, X11, nullptr, st2, 0.0, st, nullptr, pm))) return rc;
    if ((rc = gemm_plain(n1, n2, n1, X11, 1, n1, G + n1, n, 1, R12, stream))) return rc;           // R12 = X11^T G12
    TTSK_HIP(hipMemcpy2DAsync(S, (size_t)n2 * 8, G + (size_t)n1 * n + n1, (size_t)n * 8, (size_t)n2 * 8, n2, hipMemcpyDeviceToDevice, st));
    if ((rc = gemm_plain(n2, n2, n1, R12, 1, n2, R12, n2, 1, S, stream, -1.0, 1))) return rc;               // S = G22 - R12^T R12
    if ((rc = launch_chol(S, n2, X22, nullptr, st2 + 1, 0.0, st, nullptr, pm + 2))) return rc;
    if ((rc = launch(chol_combine_kernel, dim3(1), dim3(1), 0, st, pm, st2, cond_tol, status, sticky))) return rc;
    if ((rc = gemm_plain(n1, n2, n2, R12, n2, 1, X22, n2, 1, Y, stream))) return rc;                 // Y = R12 X22
    TTSK_HIP(hipMemsetAsync(Rinv, 0, (size_t)n * n * 8, st));
    TTSK_HIP(hipMemcpy2DAsync(Rinv, (size_t)n * 8, X11, (size_t)n1 * 8, (size_t)n1 * 8, n1, hipMemcpyDeviceToDevice, st));
    TTSK_HIP(hipMemcpy2DAsync(Rinv + (size_t)n1 * n + n1, (size_t)n * 8, X22, (size_t)n2 * 8, (size_t)n2 * 8, n2, hipMemcpyDeviceToDevice, st));
    if ((rc = gemm_plain(n1, n2, n1, X11, n1, 1, Y, n2, 1, Rinv + n1, stream, -1.0, 0, n))) return rc;           // X12 = -X11 Y
    if (Ginv && (rc = gemm_plain(n, n, n, Rinv, n, 1, Rinv, 1, n, Ginv, stream))) return rc;          // G^-1 = X X^T
    return TTSK_OK;
}

size_t qr_ws_elems(int64_t m, int n) { return (size_t)m * n + 4 * (size_t)n * n + 16 + chol_ws_elems(n); }

// thin QR by CholeskyQR2 + Householder sign reconstruction; 1 = done, 0 = rejected.  sticky: deferred mode -- the
// factorisation always runs to the end (A is overwritten either way), a rejection is recorded in *sticky.
static int launch_cholqr2_lds(double *M, int64_t m, int n, int *status, double cond_tol, int *sticky, hipStream_t st);

int qr_cholesky(double *A, int64_t m, int64_t n64, int stream, hipStream_t st, double *ws_in, int *sticky, bool unsigned_q)
{
    const int n = (int)n64;
    if (n > CHOL_MAX_N || m < n) return 0;
    if (m < 2 * n64 && (size_t)m * n + n <= SMALL_QR_MAX) {
        // nearly square and small: Householder in one workgroup, no gate to fail
        if (int rc = launch(small_qr_kernel, dim3(1), dim3(1024), ((size_t)m * n + n) * 8, st, A, (int)m, n)) return rc;
        return unsigned_q ? 2 : 1;        // 2: Q carries LAPACK's signs already
    }
    double *ws = ws_in ? ws_in : (double *)scratch(stream, SCRATCH_MISC, qr_ws_elems(m, n) * 8);
    if (!ws) return TTSK_ERR_HIP;
    double *Q1 = ws, *G = Q1 + (size_t)m * n, *R1 = G + n * n, *R2 = R1 + n * n, *Qtop = R2 + n * n;
    int *status = (int *)(Qtop + n * n);
    if (unsigned_q && sticky) {
        // small enough for one workgroup's LDS: the whole CholeskyQR2 in one launch
        const int fr = launch_cholqr2_lds(A, m, n, status, 1e-6, sticky, st);
        if (fr) return fr;
    }
    double *cws = n > CHOL_ONE_N ? Qtop + n * n + 16 : nullptr;
    int rc;
    if ((rc = gemm_plain(n, n, m, A, 1, n, A, n, 1, G, stream))) return rc;              // A^T A
    if ((rc = chol_inv_any(G, n, R1, nullptr, status, 1e-6, stream, st, cws, sticky))) return rc;       // kappa(A) up to ~1e6
    if ((rc = gemm_plain(m, n, n, A, n, 1, R1, n, 1, Q1, stream))) return rc;            // Q1 = A R1^-1
    if ((rc = gemm_plain(n, n, m, Q1, 1, n, Q1, n, 1, G, stream))) return rc;            // Q1^T Q1
    if (unsigned_q && n > CHOL_ONE_N) {
        if ((rc = chol_inv_any(G, n, R2, nullptr, status + 1, 0.5, stream, st, cws, sticky))) return rc;    // must be ~identity
    } else if (unsigned_q) {
        // R with positive diagonal only: the caller reconstructs the signs beside the critical path (qr_signs)
        if ((rc = launch(chol_inv_kernel, dim3(1), dim3(256), (size_t)(n * (n + 1) + n) * 8, st, G, n, R2, (double *)nullptr,
                         status + 1, 0.5, sticky, (double *)nullptr, (const double *)nullptr, 0, 2))) return rc;
    } else if (n <= CHOL_SIGN_MAX) {
        // second factorisation (G ~ identity), top block of Q and the sign reconstruction in ONE kernel
        if ((rc = launch(chol_inv_kernel, dim3(1), dim3(256), (size_t)(3 * n * (n + 1) + 2 * n) * 8, st, G, n, R2, (double *)nullptr,
                         status + 1, 0.5, sticky, (double *)nullptr, (const double *)Q1, m == n64 ? 1 : 0, 1))) return rc;
    } else {
    if ((rc = chol_inv_any(G, n, R2, nullptr, status + 1, 0.5, stream, st, cws, sticky))) return rc;    // must be ~identity
    if ((rc = gemm_plain(n, n, n, Q1, n, 1, R2, n, 1, Qtop, stream))) return rc;         // top block of Q
    if (n <= CHOL_ONE_N)
        rc = launch(hh_sign_scale_kernel, dim3(1), dim3(256), (size_t)(n * (n + 1) + n) * 8, st, Qtop, n,
                    m == n64 ? 1 : 0, R2);
    else        // beyond one workgroup's LDS: the same modified LU with the working copy in global memory (Qtop itself)
        rc = launch(hh_sign_scale_global_kernel, dim3(1), dim3(1024), 0, st, Qtop, n, m == n64 ? 1 : 0, R2);
    if (rc) return rc;
    }
    if (!sticky) {
        int host_status[2] = {1, 1};
        TTSK_HIP(hipMemcpyAsync(host_status, status, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
        TTSK_HIP(hipStreamSynchronize(st));
        if (host_status[0] || host_status[1]) return 0;
    }
    if ((rc = gemm_plain(m, n, n, Q1, n, 1, R2, n, 1, A, stream))) return rc;            // Q = Q1 R2^-1 S
    return 1;
}

// CholeskyQR2 of a SMALL tall matrix in ONE workgroup (m (n + 2) + n (n + 1) + n doubles fit the LDS: the first mode of an
// orthogonalising sketch, 200 x 50 at C3): M (m x n, row-major, in place) -> Q with the signs of CholeskyQR (R's diagonal
// positive; the caller reconstructs Householder's signs with qr_signs).  Both Gram matrices, both factorisations, both
// products without leaving the LDS: one launch instead of eight (Gram + reduce, factorisation, product, twice).
// status[0] / status[1]: verdicts of the two factorisations as chol_inv_kernel gives them (gates cond_tol, 0.5).
constexpr size_t CHOLQR2_LDS_MAX = 19000;       // doubles
__global__ __launch_bounds__(1024) void cholqr2_lds_kernel(double *__restrict__ M, int m, int n, int *__restrict__ status,
                                                           double cond_tol, int *__restrict__ sticky)
{
    extern __shared__ double sm[];
    __shared__ double shadow[2 * 128];
    const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = nthr >> 6, x16 = lane & 15, g = lane >> 4;
    // operands zero-padded to whole tiles, so that the matrix-core loops carry no bounds
    const int nt = (n + 15) >> 4, mt = (m + 15) >> 4, np = 16 * nt, mp = 16 * mt, ldm = np + 2, ld = np + 1;
    double *Ms = sm, *A = sm + (size_t)mp * ldm, *xd = A + (size_t)np * ld;
    const bool core = tid < 256;
    for (int e = tid; e < mp * ldm; e += nthr) Ms[e] = 0.0;
    for (int e = tid; e < np * ld + np; e += nthr) A[e] = 0.0;
    __syncthreads();
    for (int e0 = tid; e0 < m * n; e0 += 8 * nthr) {          // eight loads in flight per thread
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = e0 + u * nthr < m * n ? M[e0 + u * nthr] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + u * nthr;
            if (e < m * n) Ms[(e / n) * ldm + e % n] = v[u];
        }
    }
    __syncthreads();
    // A = Ms^T Ms: one tile pair (t1 <= t2) per wave and turn, the whole column of row blocks
    auto gram = [&]() {
        int q = 0;
        for (int t1 = 0; t1 < nt; ++t1)
            for (int t2 = t1; t2 < nt; ++t2, ++q) {
                if (q % nw != wv) continue;
                v4d acc = {0.0, 0.0, 0.0, 0.0};
                const double *pa = Ms + g * ldm + 16 * t1 + x16, *pb = Ms + g * ldm + 16 * t2 + x16;
                // four k-blocks per step (a row tile of Ms), the next step's operands read before this step's matrix instructions
                double a[4], b[4], an[4], bn[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) { a[u] = pa[4 * u * ldm]; b[u] = pb[4 * u * ldm]; }
                for (int s4 = 0; s4 < mt; ++s4) {
                    const int nx = s4 + 1 < mt ? s4 + 1 : s4;
#pragma unroll
                    for (int u = 0; u < 4; ++u) { an[u] = pa[(16 * nx + 4 * u) * ldm]; bn[u] = pb[(16 * nx + 4 * u) * ldm]; }
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc = mfma16(a[u], b[u], acc);
#pragma unroll
                    for (int u = 0; u < 4; ++u) { a[u] = an[u]; b[u] = bn[u]; }
                }
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int r = 16 * t1 + g + 4 * v, c = 16 * t2 + x16;
                    if (r < n && c < n) { A[r * ld + c] = acc[v]; A[c * ld + r] = acc[v]; }
                }
            }
    };
    // X from chol_lds's storage (strict upper part transposed into the lower triangle, diagonal in xd) to a dense upper
    // triangular matrix in A, in place
    auto densify = [&]() {
        for (int e = tid; e < n * n; e += nthr) {
            const int i = e / n, c = e - i * n;
            if (i < c) { const double t = A[c * ld + i]; A[i * ld + c] = t; A[c * ld + i] = 0.0; }
            else if (i == c) A[i * ld + i] = xd[i];
        }
    };
    // rows of Ms (or of the output) <- rows of Ms times A; a wave owns its row tiles
    auto apply = [&](double *out, int ldo) {
        for (int tile = wv; tile < mt; tile += nw) {
            v4d acc[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = v4d{0.0, 0.0, 0.0, 0.0};
            const double *pa = Ms + (16 * tile + x16) * ldm + g, *pb = A + g * ld + x16;
            // the operands of k-block kb + 1 are read before the matrix instructions of k-block kb
            double a = pa[0], b[4], an, bn[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) b[t] = t < nt ? pb[16 * t] : 0.0;
            for (int kb = 0; kb < 4 * nt; ++kb) {
                const int nx = kb + 1 < 4 * nt ? kb + 1 : kb;
                an = pa[4 * nx];
#pragma unroll
                for (int t = 0; t < 4; ++t) bn[t] = t < nt ? pb[4 * nx * ld + 16 * t] : 0.0;
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    if (t < nt) acc[t] = mfma16(a, b[t], acc[t]);
                a = an;
#pragma unroll
                for (int t = 0; t < 4; ++t) b[t] = bn[t];
            }
#pragma unroll
            for (int t = 0; t < 4; ++t)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int r = 16 * tile + g + 4 * v, c = 16 * t + x16;
                    if (t < nt && r < m && c < n) out[(size_t)r * ldo + c] = acc[t][v];
                }
        }
    };
    gram();
    __syncthreads();
    int bad = 0;
    double pmin = 1e300, pmax = 0.0;
    chol_lds(A, xd, n, ld, shadow, tid, nthr, bad, pmin, pmax);
    if (tid == 0) {
        const int rej = (bad || pmin < cond_tol * cond_tol * pmax) ? 1 : 0;
        status[0] = rej;
        if (rej && sticky) *sticky = 1;
    }
    densify();
    __syncthreads();
    apply(Ms, ldm);                                        // Q1 = M R1^-1 in place
    __syncthreads();
    gram();                                                // overwrites A's n x n block (both triangles)
    __syncthreads();
    // second factor: I - Phi(E) where the Gram matrix is the identity to 1e-8 / n, the recurrence otherwise
    double em = 0.0;
    if (core) {
        for (int e = tid; e < n * n; e += 256) {
            const int i = e / n, c = e - i * n;
            em = fmax(em, fabs(A[i * ld + c] - (i == c ? 1.0 : 0.0)));
        }
        em = fmax(em, jac_dpp<0xB1>(em));
        em = fmax(em, jac_dpp<0x4E>(em));
        if ((tid & 3) == 0) shadow[tid >> 2] = em;
    }
    __syncthreads();
    em = 0.0;
    for (int k = 0; k < 64; ++k) em = fmax(em, shadow[k]);
    __syncthreads();
    if (em * n <= 1e-8) {
        for (int e = tid; e < n * n; e += nthr) {           // dense X2 = I - Phi(E) in place
            const int i = e / n, c = e - i * n;
            if (i < c) A[i * ld + c] = -A[i * ld + c];
            else if (i == c) A[i * ld + i] = 1.0 - 0.5 * (A[i * ld + i] - 1.0);
        }
        __syncthreads();
        for (int e = tid; e < n * n; e += nthr) {
            const int i = e / n, c = e - i * n;
            if (i > c) A[i * ld + c] = 0.0;
        }
        if (tid == 0) status[1] = 0;
    } else {
        bad = 0; pmin = 1e300; pmax = 0.0;
        chol_lds(A, xd, n, ld, shadow, tid, nthr, bad, pmin, pmax);
        if (tid == 0) {
            const int rej = (bad || pmin < 0.25 * pmax) ? 1 : 0;
            status[1] = rej;
            if (rej && sticky) *sticky = 1;
        }
        densify();
    }
    __syncthreads();
    apply(M, n);                                           // Q = Q1 R2^-1
}

// 1 = queued, 0 = does not fit
static int launch_cholqr2_lds(double *M, int64_t m, int n, int *status, double cond_tol, int *sticky, hipStream_t st)
{
    if (n > 64 || m < n || m > 4096) return 0;
    const size_t np = 16 * (size_t)((n + 15) >> 4), mp = 16 * (size_t)((m + 15) >> 4);
    const size_t elems = mp * (np + 2) + np * (np + 1) + np;
    if (elems > CHOLQR2_LDS_MAX) return 0;
    const size_t lds = elems * 8;
    if (int rc = launch(cholqr2_lds_kernel, dim3(1), dim3(1024), lds, st, M, (int)m, n, status, cond_tol, sticky)) return rc;
    return 1;
}

// The Householder column signs of Q = D Qc (Qc: top n x n block of a CholeskyQR factor with positive diagonal R, D a
// +-1 scaling of its rows given per group of `rows_per` rows -- the signs of the previous mode's factor, which scale the
// rows of this mode's unfolding): S[c] for the caller to apply whenever it likes.  One workgroup per matrix, `count` matrices
// of one shape per launch (the tensors of an orthogonalising batch, tt_orth.hip; one for qr_signs).
struct QrSignsBatch {
    const double *Q[QR_BATCH_MAX], *Sprev[QR_BATCH_MAX];
    double *Sout[QR_BATCH_MAX];
};
__global__ __launch_bounds__(1024) void qr_signs_batch_kernel(QrSignsBatch a, int n, int square, int rows_per)
{
    extern __shared__ double sm[];
    const int ld = n + 1, tid = threadIdx.x;
    double *B = sm, *S = sm + n * ld;
    __shared__ double shadow[2 * 128];
    const int nthr = blockDim.x;
    const double *Qtop = a.Q[blockIdx.x], *Sprev = a.Sprev[blockIdx.x];
    double *Sout = a.Sout[blockIdx.x];
    for (int e = tid; e < n * n; e += nthr) {
        const int r = e / n;
        B[r * ld + e % n] = Qtop[e] * (Sprev ? Sprev[r / rows_per] : 1.0);
    }
    __syncthreads();
    hh_signs_lds(B, n, ld, square, S, shadow, tid, nthr);
    for (int c = tid; c < n; c += nthr) Sout[c] = S[c];
}

bool qr_signs_batch_covers(int count, int n) { return n <= CHOL_ONE_N && count >= 1 && count <= QR_BATCH_MAX; }

int qr_signs_batch(int count, const double *const *Qtop, int n, int square, const double *const *Sprev, int rows_per, double *const *Sout,
                   hipStream_t st)
{
    if (!qr_signs_batch_covers(count, n)) return 0;
    QrSignsBatch a{};
    for (int b = 0; b < count; ++b) { a.Q[b] = Qtop[b]; a.Sprev[b] = Sprev ? Sprev[b] : nullptr; a.Sout[b] = Sout[b]; }
    if (int rc = launch(qr_signs_batch_kernel, dim3((unsigned)count), dim3(chol_threads(n)), (size_t)(n * (n + 1) + n) * 8, st, a, n, square, rows_per)) return rc;
    return 1;
}

// the same for 128 < n <= 256: the working copy B (n x n) lives in global memory (L2), one column per step
__global__ __launch_bounds__(1024) void qr_signs_global_kernel(const double *__restrict__ Qtop, int n, int square,
                                                               const double *__restrict__ Sprev, int rows_per,
                                                               double *__restrict__ B, double *__restrict__ Sout)
{
    const int tid = threadIdx.x;
    for (int e = tid; e < n * n; e += 1024) B[e] = Qtop[e] * (Sprev ? Sprev[(e / n) / rows_per] : 1.0);
    __threadfence_block();
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        const double piv = B[j * n + j];
        double sgn = piv >= 0.0 ? -1.0 : 1.0;
        if (square && j == n - 1) sgn = -sgn;
        if (tid == 0) Sout[j] = sgn;
        const double pinv = 1.0 / (piv - sgn);
        const int rem = n - j - 1;
        for (int e = tid; e < rem * rem; e += 1024) {
            const int i = j + 1 + e / rem, c = j + 1 + e % rem;
            B[i * n + c] = fma(-B[i * n + j] * pinv, B[j * n + c], B[i * n + c]);
        }
        __threadfence_block();
        __syncthreads();
    }
}

// work: n * n doubles for n > 128 (may be nullptr otherwise)
int qr_signs(const double *Qtop, int n, int square, const double *Sprev, int rows_per, double *Sout, hipStream_t st, double *work)
{
    if (n <= CHOL_ONE_N) return qr_signs_batch(1, &Qtop, n, square, Sprev ? &Sprev : nullptr, rows_per, &Sout, st);
    if (n > CHOL_MAX_N || !work) return 0;
    if (int rc = launch(qr_signs_global_kernel, dim3(1), dim3(1024), 0, st, Qtop, n, square, Sprev, rows_per, work, Sout)) return rc;
    return 1;
}

size_t qr_batch_ws_elems(int count, int64_t m, int n) { return (size_t)count * ((size_t)m * n + 3 * (size_t)n * n) + (size_t)count + 16; }

bool qr_cholesky_batch_covers(int count, int64_t m, int n) { return count >= 1 && count <= QR_BATCH_MAX && n <= CHOL_ONE_N && m >= 2 * (int64_t)n; }

// CholeskyQR2 of `count` tall matrices of one shape (m x n row-major, in place), UNSIGNED factors (R's diagonal positive: the caller
// reconstructs Householder's signs, qr_signs_batch): two Gram products, two factorisations, two triangular products, each ONE
// launch over all matrices (tensor by tensor where a shape has no batched kernel).  Verdicts into *sticky (deferred).
// 1 = queued, 0 = outside this path -- nothing has been queued then.
int qr_cholesky_batch(int count, double *const *A, int64_t m, int n, int stream, hipStream_t st, double *ws, int *sticky)
{
    if (!qr_cholesky_batch_covers(count, m, n) || !ws || !sticky) return 0;
    double *Q1 = ws, *G = Q1 + (size_t)count * m * n, *R1 = G + (size_t)count * n * n, *R2 = R1 + (size_t)count * n * n;
    int *status = (int *)(R2 + (size_t)count * n * n);
    const double *cA[QR_BATCH_MAX], *cQ1[QR_BATCH_MAX], *cR1[QR_BATCH_MAX], *cR2[QR_BATCH_MAX];
    double *pQ1[QR_BATCH_MAX], *pG[QR_BATCH_MAX];
    for (int b = 0; b < count; ++b) {
        cA[b] = A[b]; pQ1[b] = Q1 + (size_t)b * m * n; cQ1[b] = pQ1[b];
        pG[b] = G + (size_t)b * n * n; cR1[b] = R1 + (size_t)b * n * n; cR2[b] = R2 + (size_t)b * n * n;
    }
    const ttsk_gemm_desc gram = gemm_desc(n, n, m, 1, n, n, 1), tri = gemm_desc(m, n, n, n, 1, n, 1);
    int rc;
    if ((rc = gemm_each(gram, count, cA, cA, pG, stream, st))) return rc;                                     // A^T A
    if ((rc = launch_chol(G, n, R1, nullptr, status, 1e-6, st, sticky, nullptr, count))) return rc;           // kappa(A) up to ~1e6
    if ((rc = gemm_each(tri, count, cA, cR1, pQ1, stream, st))) return rc;                                    // Q1 = A R1^-1
    if ((rc = gemm_each(gram, count, cQ1, cQ1, pG, stream, st))) return rc;                                   // Q1^T Q1 ~ identity
    if ((rc = launch(chol_inv_kernel, dim3((unsigned)count), dim3(256), (size_t)(n * (n + 1) + n) * 8, st, (const double *)G, n, R2, (double *)nullptr,
                     status + count, 0.5, sticky, (double *)nullptr, (const double *)nullptr, 0, 2))) return rc;
    if ((rc = gemm_each(tri, count, cQ1, cR2, A, stream, st))) return rc;                                     // Q = Q1 R2^-1
    return 1;
}

// core[a, i, b] *= sp[a] sn[b] for up to QR_BATCH_MAX cores in one launch (sp / sn may be nullptr = all ones)
struct SignFix {
    double *core[QR_BATCH_MAX];
    const double *sp[QR_BATCH_MAX], *sn[QR_BATCH_MAX];
    int k0[QR_BATCH_MAX], nn[QR_BATCH_MAX], k1[QR_BATCH_MAX];
};
__global__ __launch_bounds__(256) void apply_signs_kernel(SignFix f)
{
    const int q = blockIdx.y;
    double *c = f.core[q];
    const double *sp = f.sp[q], *sn = f.sn[q];
    const int k1 = f.k1[q], rows = f.k0[q] * f.nn[q], nn = f.nn[q];
    // a row (a, i) per 16-lane group and step, its k1 entries 16 at a time
    const int grp = threadIdx.x >> 4, x = threadIdx.x & 15;
    for (int r = blockIdx.x * 16 + grp; r < rows; r += gridDim.x * 16) {
        const double sr = sp ? sp[r / nn] : 1.0;
        double *row = c + (size_t)r * k1;
        for (int b = x; b < k1; b += 16) row[b] *= sn ? sr * sn[b] : sr;
    }
}
int apply_signs(int count, double *const *cores, const double *const *sp, const double *const *sn, const int *k0, const int *nn,
                const int *k1, hipStream_t st)
{
    for (int c0 = 0; c0 < count; c0 += QR_BATCH_MAX) {
        SignFix f{};
        const int cnt = count - c0 < QR_BATCH_MAX ? count - c0 : QR_BATCH_MAX;
        for (int q = 0; q < cnt; ++q) {
            f.core[q] = cores[c0 + q]; f.sp[q] = sp[c0 + q]; f.sn[q] = sn[c0 + q];
            f.k0[q] = k0[c0 + q]; f.nn[q] = nn[c0 + q]; f.k1[q] = k1[c0 + q];
        }
        if (int rc = launch(apply_signs_kernel, dim3(160, cnt), dim3(256), 0, st, f)) return rc;
    }
    return TTSK_OK;
}

}  // namespace ttsk
