// The bond solve of Gram-SVD rounding: every bond of a tensor train truncated at once from the Gram
// matrices GL_b, GR_b of its left and right parts.
//
//  launch 1, one workgroup per Gram:  G = V Lambda V^T by one-sided Jacobi on the Gram itself (W = G, V = I: V converges
//            to the eigenvectors, W = G V to their multiples); eigenpairs with lambda > r eps_machine lambda_max are kept.
//  launch 2, one workgroup per bond:  A = Lambda_R^{1/2} V_R^T V_L Lambda_L^{1/2} (the transpose of DESIGN's M), the same
//            Jacobi on A: its V holds the left singular vectors U of M.  Q = U^T Lambda_L^{1/2} V_L^T for every column,
//            sigma_c^2 = q_c^T GR q_c, the rank rule, then P = V_L Lambda_L^{-1/2} U_rho and the first rho rows of Q.
//  Each Jacobi runs to convergence, scales the columns of V back to unit length, forms W afresh from its input and runs
//  again (grb_unit_columns, grb_refresh): what keeps the result at the accuracy of LAPACK at ranks in the hundreds.
//
// The pair step and the convergence rules are those of jacobi.hip (jacobi_pair.h).  No atomics and a fixed order of every
// sum: the same bits on every call.  Where a bond's W and V live -- LDS or the workspace -- is grb_place of
// gram_round_plan.h, decided per bond and taken here per workgroup, so bonds of every size share the two launches.
#include <cfloat>
#include <cmath>
#include "gram_round_plan.h"
#include "jacobi_pair.h"
#include "prof.h"

namespace ttsk {

namespace {

// squared column norms of Wc (mW x nW column-major) into s_val, one 16-lane group per column
__device__ __forceinline__ void grb_norms2(const double *Wc, const int mW, const int nW, double *s_val)
{
    const int grp = threadIdx.x >> 4, gl = threadIdx.x & 15, ngrp = blockDim.x >> 4;
    for (int j = grp; j < nW; j += ngrp) {
        const double *wj = Wc + (size_t)j * mW;
        double a = 0;
        for (int i = gl; i < mW; i += 16) a = fma(wj[i], wj[i], a);
        a = row_sum16(a);
        if (gl == 0) s_val[j] = a;
    }
}

// One-sided Jacobi on Wc (mW x nW column-major, either may be the longer side) and V (nW x nW, the identity on entry), both
// written and a barrier passed before the call: the round-robin sweeps of jacobi_pinv_kernel's factor mode with its
// tolerance sqrt(m) eps, m the longer side, and its noise rule taken further: a column at noise level (norm below 4 m eps of
// the largest) is rotated against no other (ONE_TINY of jac_pair).  Ends after a sweep without a rotation; a barrier follows.
__device__ __forceinline__ void grb_sweeps(double *Wc, double *V, const int mW, const int nW, double *s_val, int *s_rot, double *s_smax)
{
    const int tid = threadIdx.x, grp = tid >> 4, gl = tid & 15, ngrp = blockDim.x >> 4;
    const int np = nW + (nW & 1), nm1 = np - 1;  // players (one dummy if odd)
    const int big = mW > nW ? mW : nW;
    const double tol = fmax(4.0, sqrt((double)big)) * DBL_EPSILON, tol2 = tol * tol;
    const int itc = big <= 64 ? 4 : (big <= 128 ? 8 : 0);
    for (int sweep = 0; sweep < 60; ++sweep) {
        if (tid == 0) *s_rot = 0;
        grb_norms2(Wc, mW, nW, s_val);
        __syncthreads();
        if (tid == 0) {
            double mx = 0;
            for (int j = 0; j < nW; ++j) mx = fmax(mx, s_val[j]);
            *s_smax = mx;
        }
        __syncthreads();
        const double tiny = 4.0 * big * DBL_EPSILON, tiny2 = tiny * tiny * *s_smax;
        for (int round = 0; round < np - 1; ++round) {
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
                if (itc == 4) jac_pair<4, true, true>(wp, wq, vp, vq, mW, nW, gl, tol2, tiny2, s_rot);
                else if (itc == 8) jac_pair<8, true, true>(wp, wq, vp, vq, mW, nW, gl, tol2, tiny2, s_rot);
                else jac_pair<0, true, true>(wp, wq, vp, vq, mW, nW, gl, tol2, tiny2, s_rot);
            }
            __syncthreads();
        }
        const int rot = *s_rot;
        __syncthreads();
        if (!rot) break;
    }
}

// s_ord = the indices 0 .. n - 1 by descending s_val (equal values: the lower index first), every thread counting the
// entries that come before its own: n steps instead of one thread's n^2 / 4.  A barrier follows.
__device__ __forceinline__ void grb_order(const double *s_val, int *s_ord, const int n)
{
    for (int j = threadIdx.x; j < n; j += blockDim.x) s_ord[j] = j;      // every slot a valid index even if a NaN breaks the count
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        const double v = s_val[j];
        int pos = 0;
        for (int k = 0; k < n; ++k) {
            const double vk = s_val[k];
            pos += (vk > v || (vk == v && k < j)) ? 1 : 0;
        }
        s_ord[pos] = j;
    }
    __syncthreads();
}

// The columns of V (n x n) back to unit length.  A rotation keeps the length of a column to rounding only, and over the
// thousands of a run of sweeps the lengths drift one way (6e-14 at n = 300) while the angles between columns stay at 4e-15.
__device__ __forceinline__ void grb_unit_columns(double *V, const int n)
{
    const int grp = threadIdx.x >> 4, gl = threadIdx.x & 15, ngrp = blockDim.x >> 4;
    for (int j = grp; j < n; j += ngrp) {
        double *vj = V + (size_t)j * n;
        double a = 0;
        for (int i = gl; i < n; i += 16) a = fma(vj[i], vj[i], a);
        a = row_sum16(a);
        const double s = a > 0.0 ? 1.0 / sqrt(a) : 0.0;
        for (int i = gl; i < n; i += 16) vj[i] *= s;
    }
    __syncthreads();
}

// W = A V afresh: Wc (mW x nW column-major) from A (mW x nW column-major, global; element (i, k) at A[i * a_i + k * a_k]) and
// V (nW x nW).  The rotations of a run of sweeps leave rounding of the largest column in every column of W; between a large and
// a small singular direction that much is then taken for convergence.  A fresh product has the rounding of one sum.
__device__ __forceinline__ void grb_refresh(double *Wc, const double *A, const size_t a_i, const size_t a_k, const double *V, const int mW, const int nW)
{
    for (int t = threadIdx.x; t < mW * nW; t += blockDim.x) {
        const int j = t / mW, i = t - j * mW;
        const double *v = V + (size_t)j * nW;
        double acc = 0.0;
        for (int k = 0; k < nW; ++k) acc = fma(A[i * a_i + k * a_k], v[k], acc);
        Wc[t] = acc;
    }
    __syncthreads();
}

// x^T G x by one 16-lane group, the value in every lane: G (r x r row-major, global), lane gl the columns gl, gl + 16, ... of every row
__device__ __forceinline__ double grb_quad16(const double *G, const double *x, const int r, const int gl)
{
    double acc = 0;
    for (int a = 0; a < r; ++a) {
        const double *g = G + (size_t)a * r;
        double t = 0;
        for (int b = gl; b < r; b += 16) t = fma(g[b], x[b], t);
        acc = fma(x[a], t, acc);
    }
    return row_sum16(acc);
}

// launch 1: the eigenpairs of one Gram of bond B into the bond's slice `ws` of the workspace
template <int LM>
__device__ __forceinline__ void grb_eig(const GrbBond &B, double *ws, const int side, int *s_rot, double *s_smax)
{
    extern __shared__ double grb_lds[];
    const int r = B.r, tid = threadIdx.x, nt = blockDim.x;
    const GrbLayout L = grb_layout(r, LM);
    double *s_val = grb_lds;
    int *s_ord = reinterpret_cast<int *>(grb_lds + r);
    double *mat = grb_lds + grb_small_elems(r);
    double *Vg = ws + (side ? L.v_r : L.v_l);
    // LM is a template parameter so that a pointer is LDS or global at compile time (ds_read / ds_write, not FLAT: jacobi.hip)
    double *Wc, *V;
    if constexpr (LM >= 1) Wc = mat; else Wc = ws + (side ? L.w_r : L.w_l);
    if constexpr (LM >= 2) V = mat + (size_t)r * r; else V = Vg;
    const double *G = side ? B.gr : B.gl;
    // the chain forms G symmetric up to rounding: take its symmetric part
    for (int t = tid; t < r * r; t += nt) {
        const int i = t / r, j = t - i * r;
        Wc[t] = 0.5 * (G[t] + G[(size_t)j * r + i]);
        V[t] = i == j ? 1.0 : 0.0;
    }
    __syncthreads();
    grb_sweeps(Wc, V, r, r, s_val, s_rot, s_smax);
    grb_unit_columns(V, r);
    grb_refresh(Wc, G, 1, (size_t)r, V, r, r);               // G is symmetric: its rows as columns
    grb_sweeps(Wc, V, r, r, s_val, s_rot, s_smax);           // two or three more sweeps
    grb_unit_columns(V, r);
    // lambda_j = v_j^T G v_j from the Gram itself, signed: W = G V has drifted by the rounding of its thousands of rotations, which
    // a fresh product has not; and a Gram that rounding left indefinite has its negative eigenvalues dropped below
    {
        const int grp = tid >> 4, gl = tid & 15, ngrp = nt >> 4;
        for (int j = grp; j < r; j += ngrp) {
            const double a = grb_quad16(G, V + (size_t)j * r, r, gl);
            if (gl == 0) s_val[j] = a;
        }
    }
    __syncthreads();
    grb_order(s_val, s_ord, r);
    if (tid == 0) {
        const double thr = (double)r * DBL_EPSILON * s_val[s_ord[0]];
        int k = 0;
        while (k < r && s_val[s_ord[k]] > thr && s_val[s_ord[k]] > 0.0) ++k;
        reinterpret_cast<int *>(ws + L.kept)[side] = k > 0 ? k : 1;       // a zero Gram keeps one pair of eigenvalue 0
    }
    double *lam = ws + (side ? L.lam_r : L.lam_l);
    int *ord = reinterpret_cast<int *>(ws + (side ? L.ord_r : L.ord_l));
    for (int j = tid; j < r; j += nt) { lam[j] = s_val[j]; ord[j] = s_ord[j]; }
    if constexpr (LM >= 2)
        for (int t = tid; t < r * r; t += nt) Vg[t] = V[t];
}

// launch 2: bond B from the eigenpairs of its two Grams
template <int LM>
__device__ __forceinline__ void grb_bond(const GrbBond &B, double *ws, const double eps, int *rank_out, int *s_rot, double *s_smax, int *s_rho)
{
    extern __shared__ double grb_lds[];
    const int r = B.r, tid = threadIdx.x, nt = blockDim.x;
    const int grp = tid >> 4, gl = tid & 15, ngrp = nt >> 4;
    const GrbLayout L = grb_layout(r, LM);
    double *s_val = grb_lds;
    int *s_ord = reinterpret_cast<int *>(grb_lds + r);
    double *mat = grb_lds + grb_small_elems(r);
    double *Wc, *V;
    if constexpr (LM >= 1) Wc = mat; else Wc = ws + L.w_l;
    if constexpr (LM >= 2) V = mat + (size_t)r * r; else V = ws + L.u;
    const double *VL = ws + L.v_l, *VR = ws + L.v_r, *lamL = ws + L.lam_l;
    double *lamR = ws + L.lam_r;
    const int *oL = reinterpret_cast<const int *>(ws + L.ord_l), *oR = reinterpret_cast<const int *>(ws + L.ord_r);
    const int *kept = reinterpret_cast<const int *>(ws + L.kept);
    const int nA = min(max(kept[0], 1), r), mA = min(max(kept[1], 1), r);       // A is kept_R x kept_L, column-major
    double *Ag = ws + L.qa;                                  // A itself, kept for the fresh product; the slot is Q's afterwards
    for (int e = grp; e < mA * nA; e += ngrp) {
        const int i = e / mA, j = e - i * mA;
        const double *vl = VL + (size_t)oL[i] * r, *vr = VR + (size_t)oR[j] * r;
        double acc = 0;
        for (int a = gl; a < r; a += 16) acc = fma(vr[a], vl[a], acc);
        acc = row_sum16(acc);
        if (gl == 0) {
            acc *= sqrt(fmax(lamR[oR[j]], 0.0)) * sqrt(fmax(lamL[oL[i]], 0.0));
            Ag[e] = acc;
            Wc[e] = acc;
        }
    }
    for (int t = tid; t < nA * nA; t += nt) V[t] = (t / nA == t % nA) ? 1.0 : 0.0;
    __syncthreads();
    grb_sweeps(Wc, V, mA, nA, s_val, s_rot, s_smax);
    grb_unit_columns(V, nA);
    grb_refresh(Wc, Ag, 1, (size_t)mA, V, mA, nA);
    grb_sweeps(Wc, V, mA, nA, s_val, s_rot, s_smax);
    grb_unit_columns(V, nA);
    // Lambda_L^{1/2} over the right eigenvalues, which are used up
    for (int i = tid; i < nA; i += nt) lamR[i] = sqrt(fmax(lamL[oL[i]], 0.0));
    __syncthreads();
    // every row of Q, in the order of the Jacobi's columns: Qa[c][a] = sum_i u_c[i] sqrt(lambda_i) VL[a][i]
    double *Qa = Ag;
    for (int t = tid; t < nA * r; t += nt) {
        const int c = t / r, a = t - c * r;
        const double *u = V + (size_t)c * nA;
        double q = 0.0;
        for (int i = 0; i < nA; ++i) q = fma(VL[(size_t)oL[i] * r + a] * u[i], lamR[i], q);
        Qa[t] = q;
    }
    __syncthreads();
    // sigma_c^2 = q_c^T GR q_c from the Gram itself (the column norms of W = A V carry the drift of the rotations); of a wide
    // A only the mA largest are singular values, the others the noise of its null space
    for (int c = grp; c < nA; c += ngrp) {
        const double a = grb_quad16(B.gr, Qa + (size_t)c * r, r, gl);
        if (gl == 0) s_val[c] = fmax(a, 0.0);
    }
    __syncthreads();
    grb_order(s_val, s_ord, nA);
    const int ns = mA < nA ? mA : nA;
    if (tid == 0) {
        const double s1 = sqrt(s_val[s_ord[0]]);
        int cnt = 0;
        while (cnt < ns && sqrt(s_val[s_ord[cnt]]) > s1 * eps) ++cnt;
        const int rho = max(1, min(cnt, B.cap));
        *s_rho = rho;
        *rank_out = rho;
    }
    for (int c = tid; c < r; c += nt) B.sigma[c] = c < ns ? sqrt(s_val[s_ord[c]]) : 0.0;
    __syncthreads();
    // Lambda_L^{-1/2} over sigma^2 (0 for the pair of a zero Gram)
    for (int i = tid; i < nA; i += nt) s_val[i] = lamR[i] > 0.0 ? 1.0 / lamR[i] : 0.0;
    __syncthreads();
    const int rho = *s_rho;
    // row c of Q: that of the c-th largest sigma;  P^T[c][a] = sum_i VL[a][i] u_c[i] / sqrt(lambda_i);  rows beyond the rank zero
    for (int t = tid; t < r * r; t += nt) {
        const int c = t / r, a = t - c * r;
        double p = 0.0, q = 0.0;
        if (c < rho) {
            const double *u = V + (size_t)s_ord[c] * nA;
            for (int i = 0; i < nA; ++i) p = fma(VL[(size_t)oL[i] * r + a] * u[i], s_val[i], p);
            q = Qa[(size_t)s_ord[c] * r + a];
        }
        B.pt[t] = p;
        B.q[t] = q;
    }
}

__global__ __launch_bounds__(GRB_THREADS) void gram_round_eig_kernel(const GramRoundArgs a)
{
    __shared__ int s_rot;
    __shared__ double s_smax;
    const int b = blockIdx.x >> 1, side = blockIdx.x & 1;
    const GrbBond &B = a.b[b];
    size_t bytes = 0;
    const int place = grb_place(B.r, &bytes);
    double *ws = a.ws + B.ws;
    if (place == 2) grb_eig<2>(B, ws, side, &s_rot, &s_smax);
    else if (place == 1) grb_eig<1>(B, ws, side, &s_rot, &s_smax);
    else grb_eig<0>(B, ws, side, &s_rot, &s_smax);
}

__global__ __launch_bounds__(GRB_THREADS) void gram_round_bond_kernel(const GramRoundArgs a)
{
    __shared__ int s_rot, s_rho;
    __shared__ double s_smax;
    const int b = blockIdx.x;
    const GrbBond &B = a.b[b];
    size_t bytes = 0;
    const int place = grb_place(B.r, &bytes);
    double *ws = a.ws + B.ws;
    if (place == 2) grb_bond<2>(B, ws, a.eps, a.rank_out + b, &s_rot, &s_smax, &s_rho);
    else if (place == 1) grb_bond<1>(B, ws, a.eps, a.rank_out + b, &s_rot, &s_smax, &s_rho);
    else grb_bond<0>(B, ws, a.eps, a.rank_out + b, &s_rot, &s_smax, &s_rho);
}

}  // namespace

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_gram_round_bonds(const double *const *dev_gl, const double *const *dev_gr, const int64_t *ranks, const int64_t *caps, int count,
                          double eps, double *const *dev_pt, double *const *dev_q, double *const *dev_sigma, int *dev_rank_out, int stream)
{
    TTSK_STREAM(st, stream);
    GramRoundPlan p;
    if (int rc = gram_round_plan(dev_gl, dev_gr, ranks, caps, count, eps, dev_pt, dev_q, dev_sigma, dev_rank_out, &p)) {
        set_error("%s", p.msg);
        return rc;
    }
    p.a.ws = (double *)scratch(stream, SCRATCH_MISC, p.scratch);
    if (!p.a.ws) return TTSK_ERR_HIP;
    {
        ProfBracket prof(st, PROF_SOLVE, p.work * 2.0 / 3.0, "gram_round_eig_kernel");
        if (int rc = launch(gram_round_eig_kernel, dim3(p.grid_eig), dim3(GRB_THREADS), p.lds, st, p.a)) return rc;
    }
    ProfBracket prof(st, PROF_SOLVE, p.work / 3.0, "gram_round_bond_kernel");
    return launch(gram_round_bond_kernel, dim3(p.grid_bond), dim3(GRB_THREADS), p.lds, st, p.a);
}

}  // extern "C"
