// What the closing step of the inner product of two operator-times-train products (op_close.hip) is launched with,
// decided on the host: the argument checks and the cover of ttsk_op_close, the kernel's argument, the split of the summed
// mode index over the grid, the slab of partial tiles and the flops of the call.
//
// Plain C++: no HIP types, so that the plan is compiled and checked by the host compiler alone
// (tests/test_op_close_host.py) before any kernel reads it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "ttsk.h"
#include "plan_common.h"
#include "hadamard_plan.h"
#include "hadamard_close_plan.h"

namespace ttsk {

// The stages are those of hadamard_stages.h with the constants of hadamard_plan.h: c in chunks of HD_KC through LDS at
// HD_PITCH, HD_COLS values of c' per workgroup, HD_LDS bytes.  The kernel sums over j, the in-index of the second operator,
// which is cut by the filling rule of hadamard_close_plan.h (hc_cut, HC_FILL): the cut depends on the extents alone.

// the kernel's argument
struct OpCloseArgs {
    const double *Wl, *N, *Y;
    double *work;
    int64_t sN[4];               // element strides of N over (gamma, j, i, gamma')
    int64_t sY[3];               // of Y over (c, j, c')
    int64_t sNk;                 // stride of N over its inner index (gamma, i), one run
    int S, S1, s, s1, n_in, n_out, P;
    int ptiles, gtiles, cblocks; // workgroups are (j chunk, p tile, gamma' tile, c' block), the last fastest
    int jchunks, jper;           // chunk q sums j = q jper .. min(n_in, (q + 1) jper)
};

struct OpClosePlan {
    OpCloseArgs a;
    int64_t blocks;              // workgroups of the launch
    int64_t slab;                // doubles of `work`: jchunks x P x s' S'
    double flops;                // 2 n_in P S' (s S n_out + s s')
    char msg[200];               // why not, when the status is not TTSK_OK
};

// The part of the plan that needs no pointers: dims are S, S', s, s', n_in, n_out, P.  ttsk_op_close_layout is this.
inline int op_close_layout(const int64_t *dims, OpClosePlan *p)
{
    static const char *const names[7] = {"S", "S'", "s", "s'", "n_in", "n_out", "P"};
    *p = OpClosePlan{};
    if (!dims) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_close: NULL argument");
    bool wide = false;
    if (const int rc = hadamard_extents("ttsk_op_close", names, dims, &wide, p, 7)) return rc;
    // ---- the cover
    if (wide) return hadamard_wide("ttsk_op_close", p);
    if (dims[0] * dims[5] > PLAN_MAX_EXTENT)
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_op_close: S n_out = %lld; below 2^31 is covered", (long long)(dims[0] * dims[5]));
    OpCloseArgs &a = p->a;
    a.S = (int)dims[0]; a.S1 = (int)dims[1]; a.s = (int)dims[2]; a.s1 = (int)dims[3];
    a.n_in = (int)dims[4]; a.n_out = (int)dims[5]; a.P = (int)dims[6];
    a.ptiles = (int)cdiv(dims[6], 16);
    a.gtiles = (int)cdiv(dims[1], 16);
    a.cblocks = (int)cdiv(dims[3], HD_COLS);
    const int64_t tiles = (int64_t)a.ptiles * a.gtiles;             // below 2^56
    if (tiles > PLAN_MAX_EXTENT || tiles * a.cblocks > PLAN_MAX_EXTENT)
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_op_close: 2^31 workgroups or more");
    p->blocks = hc_cut(tiles * a.cblocks, dims[4], &a.jper, &a.jchunks);
    if (p->blocks > PLAN_MAX_EXTENT) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_op_close: 2^31 workgroups or more");
    // a workgroup covers at most 16 x 16 x HD_COLS elements of its slice: the slab is below 2^14 x 2^31 doubles
    p->slab = dims[1] * dims[3] * dims[6] * a.jchunks;
    p->flops = 2.0 * (double)dims[4] * (double)dims[6] * (double)dims[1] *
               ((double)dims[2] * dims[0] * dims[5] + (double)dims[2] * dims[3]);
    return TTSK_OK;
}

// strides in elements: N (gamma, j, i, gamma') then Y (c, j, c'); work_doubles: what the caller's slab holds
inline int op_close_plan(const double *Wl, const double *N, const double *Y, const int64_t *dims, const int64_t *strides, double *out,
                         int accumulate, double *work, int64_t work_doubles, OpClosePlan *p)
{
    *p = OpClosePlan{};
    if (!Wl || !N || !Y || !dims || !strides || !out || !work) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_close: NULL argument");
    if (accumulate != 0 && accumulate != 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_close: accumulate = %d, 0 or 1", accumulate);
    const int rc = op_close_layout(dims, p);
    if (rc) return rc;
    if (work_doubles < p->slab)
        PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_close: a slab of %lld doubles, the plan needs %lld", (long long)work_doubles, (long long)p->slab);
    OpCloseArgs &a = p->a;
    // the stages walk (gamma, i) as one index: an extent of 1 leaves the other's stride as that of the run
    if (a.S > 1 && a.n_out > 1 && strides[0] != a.n_out * strides[2])
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_op_close: (gamma, i) of N is not one run: strides %lld and %lld at n_out = %d; pack N as (S, n_out, n_in, S')",
                  (long long)strides[0], (long long)strides[2], a.n_out);
    a.Wl = Wl; a.N = N; a.Y = Y; a.work = work;
    for (int i = 0; i < 4; ++i) a.sN[i] = strides[i];
    for (int i = 0; i < 3; ++i) a.sY[i] = strides[4 + i];
    a.sNk = a.n_out > 1 ? strides[2] : strides[0];
    return TTSK_OK;
}

}  // namespace ttsk
