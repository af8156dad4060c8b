// What the batched bond solve of Gram-SVD rounding (gram_round.hip) is launched with, decided on the host: the argument
// checks and the cover of ttsk_gram_round_bonds, where each bond's Jacobi working set lives, the layout of each bond's
// slice of the workspace, the two grids and the dynamic LDS of the launches.
//
// Plain C++: no HIP types, so that the plan is compiled and checked by the host compiler alone
// (tests/test_gram_round_host.py) before any kernel reads it.  The place and the layout are host and device code under the
// device compiler only.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "ttsk.h"
#include "plan_common.h"

#ifdef __HIPCC__
#define GRB_HD __host__ __device__
#else
#define GRB_HD
#endif

namespace ttsk {

constexpr int GRB_MAX_BONDS = 64;                // the bonds travel as the kernel's argument (below 4 KB)
constexpr int GRB_MAX_RANK = 1024;               // one workgroup per Jacobi: the limit of round_dev's ttsk_svd_small
constexpr int GRB_THREADS = 1024;
constexpr size_t GRB_LDS_CAP = 160 * 1024 - 256; // 160 KB per CU minus the kernels' few static bytes: the cap of jacobi.hip

// the small arrays every Jacobi keeps in LDS in front of its matrices: n values and the sort order (n ints, padded)
GRB_HD inline size_t grb_small_elems(int r) { return (size_t)r + ((size_t)r + 1) / 2; }

// where the Jacobi working set of a bond of rank r lives (W and V are at most r x r each, in both launches):
// 2 = W and V in LDS, 1 = W only (V in the workspace), 0 = both in the workspace.  The rule of jacobi_lds_mode for a
// square matrix: the edges are r = 100 / 101 and 142 / 143.  *bytes: the dynamic LDS the bond needs.
GRB_HD inline int grb_place(int r, size_t *bytes)
{
    const size_t small = grb_small_elems(r) * 8, mat = (size_t)r * r * 8;
    if (small + 2 * mat <= GRB_LDS_CAP) { *bytes = small + 2 * mat; return 2; }
    if (small + mat <= GRB_LDS_CAP) { *bytes = small + mat; return 1; }
    *bytes = small;
    return 0;
}

// A bond's slice of the workspace, offsets in doubles from its start.  The first launch leaves the eigenvectors (all r
// columns, column-major), the eigenvalues, their descending order and the number kept of either Gram; the second reads
// them.  qa holds the second launch's A for the fresh product W = A V, then every row of Q.  u is the V of the second
// launch's Jacobi where it is not in LDS (place < 2), w_l / w_r the W of the two eigenproblems where it is not (place 0);
// the second launch's W reuses w_l.  An absent piece has offset -1.
struct GrbLayout {
    int64_t v_l, v_r;            // r x r each
    int64_t lam_l, lam_r;        // r each
    int64_t ord_l, ord_r;        // r ints each, in (r + 1) / 2 doubles
    int64_t kept;                // two ints: kept eigenpairs of GL, of GR
    int64_t qa;                  // r x r
    int64_t u, w_l, w_r;
    int64_t total;
};

GRB_HD inline GrbLayout grb_layout(int r, int place)
{
    const int64_t mat = (int64_t)r * r, ints = ((int64_t)r + 1) / 2;
    GrbLayout L;
    int64_t at = 0;
    L.v_l = at; at += mat;
    L.v_r = at; at += mat;
    L.lam_l = at; at += r;
    L.lam_r = at; at += r;
    L.ord_l = at; at += ints;
    L.ord_r = at; at += ints;
    L.kept = at; at += 1;
    L.qa = at; at += mat;
    L.u = L.w_l = L.w_r = -1;
    if (place < 2) { L.u = at; at += mat; }
    if (place < 1) { L.w_l = at; at += mat; L.w_r = at; at += mat; }
    L.total = at;
    return L;
}

// one bond of the call
struct GrbBond {
    const double *gl, *gr;       // the two Grams, r x r row-major
    double *pt, *q, *sigma;      // P^T and Q (r x r row-major each, rows >= rank zero), Sigma (r, zero beyond the values found)
    int64_t ws;                  // start of the bond's slice of the workspace, in doubles
    int r, cap;
};

// the kernels' argument
struct GramRoundArgs {
    GrbBond b[GRB_MAX_BONDS];
    double *ws;
    int *rank_out;
    double eps;
    int count;
};
static_assert(sizeof(GramRoundArgs) <= 4096, "the bonds travel as a kernel argument");

struct GramRoundPlan {
    GramRoundArgs a;
    unsigned grid_eig, grid_bond;     // one workgroup per Gram, then one per bond
    size_t lds;                       // dynamic LDS of both launches: the largest need among the bonds
    size_t scratch;                   // bytes of the workspace
    int place[GRB_MAX_BONDS];
    double work;                      // flops of one sweep over every Jacobi of the call (the unit of the profiling class)
    char msg[200];                    // why not, when the status is not TTSK_OK
};

inline int gram_round_plan(const double *const *dev_gl, const double *const *dev_gr, const int64_t *ranks, const int64_t *caps, int count,
                           double eps, double *const *dev_pt, double *const *dev_q, double *const *dev_sigma, int *dev_rank_out,
                           GramRoundPlan *p)
{
    *p = GramRoundPlan{};
    if (!dev_gl || !dev_gr || !ranks || !caps || !dev_pt || !dev_q || !dev_sigma || !dev_rank_out)
        PLAN_FAIL(TTSK_ERR_ARG, "ttsk_gram_round_bonds: NULL argument");
    if (count < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_gram_round_bonds: count = %d must be positive", count);
    if (!(eps >= 0.0) || std::isinf(eps)) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_gram_round_bonds: eps = %g must be finite and not negative", eps);
    if (count > GRB_MAX_BONDS)
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_gram_round_bonds: %d bonds, at most %d are covered", count, GRB_MAX_BONDS);
    for (int b = 0; b < count; ++b) {
        if (ranks[b] < 1 || caps[b] < 1)
            PLAN_FAIL(TTSK_ERR_ARG, "ttsk_gram_round_bonds: bond %d has rank %lld and cap %lld", b, (long long)ranks[b], (long long)caps[b]);
        if (!dev_gl[b] || !dev_gr[b] || !dev_pt[b] || !dev_q[b] || !dev_sigma[b])
            PLAN_FAIL(TTSK_ERR_ARG, "ttsk_gram_round_bonds: a NULL pointer at bond %d", b);
    }
    for (int b = 0; b < count; ++b)
        if (ranks[b] > GRB_MAX_RANK)
            PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_gram_round_bonds: bond %d has rank %lld, at most %d is covered (one workgroup per bond)", b,
                      (long long)ranks[b], GRB_MAX_RANK);
    GramRoundArgs &a = p->a;
    int64_t at = 0;
    for (int b = 0; b < count; ++b) {
        GrbBond &B = a.b[b];
        B.gl = dev_gl[b]; B.gr = dev_gr[b];
        B.pt = dev_pt[b]; B.q = dev_q[b]; B.sigma = dev_sigma[b];
        B.r = (int)ranks[b];
        B.cap = (int)(caps[b] < ranks[b] ? caps[b] : ranks[b]);
        size_t bytes = 0;
        p->place[b] = grb_place(B.r, &bytes);
        if (bytes > p->lds) p->lds = bytes;
        B.ws = at;
        at += grb_layout(B.r, p->place[b]).total;
        // a sweep rotates r (r - 1) / 2 pairs of W and V columns of length r, six flops per element and column pair; three Jacobis per bond
        p->work += 3.0 * 6.0 * (double)B.r * (double)B.r * (double)(B.r - 1);
    }
    a.rank_out = dev_rank_out;
    a.eps = eps;
    a.count = count;
    p->grid_eig = 2u * (unsigned)count;
    p->grid_bond = (unsigned)count;
    p->scratch = (size_t)at * 8;
    return TTSK_OK;
}

}  // namespace ttsk
