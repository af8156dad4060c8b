// What the solver files (jacobi.hip, householder.hip, cholesky.hip, pinv.hip) share among themselves: the small device
// helpers of their kernels and the host pieces one of them offers the others.  The drivers see linalg_int.h only.
#pragma once
#include "common.h"
#include "linalg_int.h"

namespace ttsk {

// max that keeps a NaN (fmax returns the other operand)
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

// sum over the 16 lanes of a DPP row, result in every lane: x += ror(x, 8), 4, 2, 1 (v_mov_dpp row_ror)
template <int CTRL>
__device__ __forceinline__ double jac_dpp(double v)
{
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_mov_dpp(lo, CTRL, 0xF, 0xF, false);
    hi = __builtin_amdgcn_mov_dpp(hi, CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double row_sum16(double x)
{
    x += jac_dpp<0x120 + 8>(x);
    x += jac_dpp<0x120 + 4>(x);
    x += jac_dpp<0x120 + 2>(x);
    x += jac_dpp<0x120 + 1>(x);
    return x;
}

// cholesky.hip: the Cholesky inverse of `count` n x n matrices lying one after another (n <= CHOL_ONE_N), and the same contract
// for one matrix up to CHOL_MAX_N (ws: chol_ws_elems(n) doubles beyond CHOL_ONE_N)
int launch_chol(const double *G, int n, double *Rinv, double *Ginv, int *status, double cond_tol, hipStream_t st,
                int *sticky = nullptr, double *pminmax = nullptr, int count = 1);
size_t chol_ws_elems(int n);
int chol_inv_any(const double *G, int n, double *Rinv, double *Ginv, int *status, double cond_tol, int stream,
                 hipStream_t st, double *ws, int *sticky = nullptr);

// jacobi.hip: the one-workgroup Jacobi kernel over `count` workgroups (workgroup b: omega + b * om_stride -> P + b * p_stride),
// the template instance of its LDS mode for an mW x nW working set; jacobi_fits_lds: W and V both in LDS (no global scratch)
int launch_jacobi(int count, const double *omega, int64_t l, int64_t r, int transposed, double *Wc, double *V, double rcond,
                  double *P, int *rank_out, double *svd_US, double *svd_S, double *svd_Vt, const int *run_if_nonzero,
                  int64_t om_stride, int64_t p_stride, hipStream_t st);
bool jacobi_fits_lds(int64_t mW, int64_t nW);

}  // namespace ttsk
