// Pieces of the solver files (jacobi.hip, householder.hip, cholesky.hip, pinv.hip) the sketch drivers (tt_orth.hip,
// assemble_batch.hip) build on.
#pragma once
#include <cstddef>
#include <cstdint>
#include <hip/hip_runtime.h>

namespace ttsk {

// the limits of the fast (normal-equations / CholeskyQR2) paths
constexpr int CHOL_MAX_N = 256;                       // largest n of a Cholesky factorisation (two blocks beyond CHOL_ONE_N)
constexpr int CHOL_ONE_N = 128;                       // largest n of one workgroup's factorisation and sign reconstruction in LDS
constexpr int QR_BATCH_MAX = 16;                      // matrices per launch of the batched QR, sign and apply-signs kernels
constexpr double CHOL_GATE = 1.0 / 300.0;             // diag(R) spread the plain normal equations accept: 1 / spread <= kappa(Omega), often by ten
constexpr double CHOL_GATE_REFINED = 1.0 / 3.0e4;     // ... with a Newton-Schulz step behind them
constexpr double PINV_FAST_RCOND = 1e-4;              // truncation rcond beyond which the normal equations do not apply

int *deferred_flag(int stream);          // the stream's sticky rejection word (ttsk_deferred_status reads and clears it)
size_t qr_ws_elems(int64_t m, int n);    // doubles of workspace qr_cholesky needs
// thin QR in place by CholeskyQR2 with LAPACK's column signs; 1 = queued, 0 = outside the fast path, < 0 = error.
// sticky: deferred verdict (no read-back; a rejection sets *sticky)
int qr_cholesky(double *A, int64_t m, int64_t n, int stream, hipStream_t st, double *ws_in = nullptr, int *sticky = nullptr,
                bool unsigned_q = false);
// unsigned_q: Q comes out with the signs of CholeskyQR (R's diagonal positive) and the sign reconstruction is
// left to the caller (qr_signs on the top n x n block of Q, beside the critical path; apply_signs at the end);
// return value 2 = the one-workgroup Householder kernel ran instead: Q carries LAPACK's signs already.
int qr_signs(const double *Qtop, int n, int square, const double *Sprev, int rows_per, double *Sout, hipStream_t st,
             double *work = nullptr);            // work: n * n doubles when n > CHOL_ONE_N
// pinv(Omega) (r x l) through the normal equations + one Newton-Schulz step, verdict deferred to *sticky; min(l, r) <= CHOL_MAX_N.
// 1 = queued, 0 = outside the fast path
size_t pinv_deferred_ws_elems(int64_t l, int64_t r);
int pinv_deferred(const double *omega, int64_t l, int64_t r, double *pinv, int stream, hipStream_t st, double *ws, int *sticky);
int apply_signs(int count, double *const *cores, const double *const *sp, const double *const *sn, const int *k0, const int *nn,
                const int *k1, hipStream_t st);
// the same steps for `count` matrices of one shape per launch; 1 = queued, 0 = outside this path (then nothing was written).
// The *_covers predicates say beforehand whether a call of that shape is queued.
size_t qr_batch_ws_elems(int count, int64_t m, int n);
bool qr_cholesky_batch_covers(int count, int64_t m, int n);
int qr_cholesky_batch(int count, double *const *A, int64_t m, int n, int stream, hipStream_t st, double *ws, int *sticky);
bool qr_signs_batch_covers(int count, int n);
int qr_signs_batch(int count, const double *const *Qtop, int n, int square, const double *const *Sprev, int rows_per, double *const *Sout,
                   hipStream_t st);
// whether the batched fast pseudo-inverse applies to (l x r): min(l, r) <= CHOL_ONE_N and a full-rank truncation rule; and
// whether ttsk_pinv_batch (refine = false) / ttsk_pinv_batch_deferred (refine = true) queue `count` such matrices (every stage
// of the normal equations on the small kernel) rather than return TTSK_ERR_UNSUPPORTED
bool pinv_batch_fast(int64_t l, int64_t r);
bool pinv_batch_covers(int count, int64_t l, int64_t r, bool refine);
// ttsk_tt_assemble_batch: batched Cholesky inverse of `count` n x n matrices lying one after another (n <= CHOL_ONE_N, the gate of
// ttsk_pinv_batch) and the predicated Jacobi kernel over equally spaced matrices in ONE launch (1 = queued, 0 = outside its LDS,
// nothing queued)
int chol_inv_batch(const double *G, int n, double *Rinv, double *Ginv, int *status, int count, hipStream_t st);
int jacobi_pinv_spaced(int count, const double *omega, int64_t os, int64_t l, int64_t r, double *P, int64_t ps,
                       const int *status, hipStream_t st);
}  // namespace ttsk
