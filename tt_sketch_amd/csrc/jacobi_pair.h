// The pair step of the one-sided Jacobi kernels (jacobi.hip, gram_round.hip): one definition for both.
#pragma once
#include "solver.h"

namespace ttsk {

// One Jacobi pair step by a 16-lane group: columns wp, wq (length mW) of W and vp, vq (length nW) of V.
// IT > 0: mW, nW <= 16 IT -- the columns stay in registers between the inner products and the rotation
// (one LDS read instead of two) and the loops are straight-line code; IT = 0: any length.
// ONE_TINY: a pair is left alone as soon as ONE of its columns is at rounding-noise level (gram_round.hip: a wide W
// has more columns than rows, so the columns of its null space cannot become orthogonal to all the others; each
// rotation against a large column only shrinks them, by eps a sweep, until the sweep limit).
template <int IT, bool WITH_V = true, bool ONE_TINY = false>
__device__ __forceinline__ void jac_pair(double *wp, double *wq, double *vp, double *vq, const int mW, const int nW,
                                         const int gl, const double tol2, const double tiny2, int *s_rot)
{
    constexpr int ITC = IT ? IT : 1;
    double x[ITC], y[ITC];
    double a = 0, b = 0, g = 0, a1 = 0, b1 = 0, g1 = 0;
    if constexpr (IT > 0) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = gl + 16 * it;
            x[it] = i < mW ? wp[i] : 0.0;
            y[it] = i < mW ? wq[i] : 0.0;
        }
#pragma unroll
        for (int it = 0; it < IT; it += 2) {
            a = fma(x[it], x[it], a); b = fma(y[it], y[it], b); g = fma(x[it], y[it], g);
            if (it + 1 < IT) {
                a1 = fma(x[it + 1], x[it + 1], a1); b1 = fma(y[it + 1], y[it + 1], b1); g1 = fma(x[it + 1], y[it + 1], g1);
            }
        }
        a += a1; b += b1; g += g1;
    } else {
        for (int i = gl; i < mW; i += 16) {
            const double xx = wp[i], yy = wq[i];
            a = fma(xx, xx, a); b = fma(yy, yy, b); g = fma(xx, yy, g);
        }
    }
    a = row_sum16(a); b = row_sum16(b); g = row_sum16(g);
    // both columns at rounding-noise level (norm^2 <= tiny2 = (4 m eps)^2 x the largest column norm^2 of this
    // sweep): directions the rank rule drops anyway; rotating noise against noise never converges in the
    // relative sense and kept rank-deficient sketches sweeping until the limit.  W = A V holds regardless.
    if (g * g <= tol2 * (a * b) || g == 0.0 || (ONE_TINY ? (a <= tiny2 || b <= tiny2) : (a <= tiny2 && b <= tiny2))) return;
    if (gl == 0) *s_rot = 1;
    const double zeta = (b - a) / (2.0 * g);
    const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
    const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
    if constexpr (IT > 0) {
#pragma unroll
        for (int it = 0; it < IT; ++it) {
            const int i = gl + 16 * it;
            if (i < mW) { wp[i] = c * x[it] - s * y[it]; wq[i] = s * x[it] + c * y[it]; }
        }
        if constexpr (WITH_V) {
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int i = gl + 16 * it;
                x[it] = i < nW ? vp[i] : 0.0;
                y[it] = i < nW ? vq[i] : 0.0;
            }
#pragma unroll
            for (int it = 0; it < IT; ++it) {
                const int i = gl + 16 * it;
                if (i < nW) { vp[i] = c * x[it] - s * y[it]; vq[i] = s * x[it] + c * y[it]; }
            }
        }
    } else {
        for (int i = gl; i < mW; i += 16) {
            const double xx = wp[i], yy = wq[i];
            wp[i] = c * xx - s * yy; wq[i] = s * xx + c * yy;
        }
        if constexpr (WITH_V)
            for (int i = gl; i < nW; i += 16) {
                const double xx = vp[i], yy = vq[i];
                vp[i] = c * xx - s * yy; vq[i] = s * xx + c * yy;
            }
    }
}

}  // namespace ttsk
