// What the Hadamard-product pass (hadamard_apply.hip) is launched with, decided on the host: the argument checks and the
// cover of ttsk_hadamard_apply, the kernel's argument, the grid, the LDS of a workgroup and the flops of the call.
//
// Plain C++: no HIP types, so that the plan is compiled and checked by the host compiler alone
// (tests/test_hadamard_host.py) before any kernel reads it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "ttsk.h"
#include "plan_common.h"
#include "op_apply_plan.h"

namespace ttsk {

constexpr int HD_KC = 32;                        // beta rows of T1 held in LDS at once
constexpr int HD_COL_TILES = 4;                  // 16-column tiles of beta' a workgroup accumulates: 16 l x 4 = 64 tiles, two waves per SIMD
constexpr int HD_COLS = 16 * HD_COL_TILES;
constexpr int HD_PITCH = OP_PITCH;               // one beta row of T1 is a 16 x 16 tile of (l, a'), at op_apply's conflict-free pitch
constexpr size_t HD_LDS = (size_t)HD_KC * HD_PITCH * 8;

// the kernel's argument
struct HadamardArgs {
    const double *L, *X, *Y;
    double *W;
    int64_t sX[3];               // element strides of X over (beta, i, beta')
    int64_t sY[3];               // of Y over (a, i, a')
    int64_t w_cols, w_off;
    int R, R1, r, r1, n, l;
    int ltiles, atiles, cblocks; // workgroups are (i, l tile, a' tile, beta' block), the last fastest
};

struct HadamardPlan {
    HadamardArgs a;
    int64_t blocks;              // workgroups of the launch
    double flops;                // 2 l n (R r r' + R R' r')
    char msg[200];               // why not, when the status is not TTSK_OK
};

// The extents of `entry` (six of hadamard_apply or hadamard_close, seven of op_close), named for its messages: each is
// positive, or the plan fails; *wide is set where one is 2^31 or more, which hadamard_wide refuses once the argument checks
// are through.
template <class Plan>
inline int hadamard_extents(const char *entry, const char *const *names, const int64_t *dims, bool *wide, Plan *p, int count = 6)
{
    for (int i = 0; i < count; ++i)
        if (dims[i] < 1) PLAN_FAIL(TTSK_ERR_ARG, "%s: %s = %lld must be positive", entry, names[i], (long long)dims[i]);
    for (int i = 0; i < count; ++i)
        if (dims[i] > PLAN_MAX_EXTENT) *wide = true;
    return TTSK_OK;
}

template <class Plan>
inline int hadamard_wide(const char *entry, Plan *p)
{
    PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "%s: an extent of 2^31 or more; below 2^31 is covered", entry);
}

// dims: R, R', r, r', n, l; strides in elements: X (beta, i, beta') then Y (a, i, a')
inline int hadamard_apply_plan(const double *L, const double *X, const double *Y, const int64_t *dims, const int64_t *strides,
                               double *W, int64_t w_cols, int64_t w_off, HadamardPlan *p)
{
    static const char *const names[6] = {"R", "R'", "r", "r'", "n", "l"};
    *p = HadamardPlan{};
    if (!L || !X || !Y || !dims || !strides || !W) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_hadamard_apply: NULL argument");
    bool wide = w_cols > PLAN_MAX_EXTENT;
    if (const int rc = hadamard_extents("ttsk_hadamard_apply", names, dims, &wide, p)) return rc;
    if (w_cols < 1 || w_off < 0)
        PLAN_FAIL(TTSK_ERR_ARG, "ttsk_hadamard_apply: w_cols = %lld, w_off = %lld", (long long)w_cols, (long long)w_off);
    // (extents below 2^31: the product below is below 2^62)
    if (!wide && (w_off > w_cols || dims[1] * dims[3] > w_cols - w_off))
        PLAN_FAIL(TTSK_ERR_ARG, "ttsk_hadamard_apply: columns %lld + %lld x %lld pass w_cols = %lld", (long long)w_off, (long long)dims[1],
                  (long long)dims[3], (long long)w_cols);
    // ---- the cover
    if (wide) return hadamard_wide("ttsk_hadamard_apply", p);
    HadamardArgs &a = p->a;
    a.L = L; a.X = X; a.Y = Y; a.W = W;
    for (int i = 0; i < 3; ++i) { a.sX[i] = strides[i]; a.sY[i] = strides[3 + i]; }
    a.w_cols = w_cols; a.w_off = w_off;
    a.R = (int)dims[0]; a.R1 = (int)dims[1]; a.r = (int)dims[2]; a.r1 = (int)dims[3]; a.n = (int)dims[4]; a.l = (int)dims[5];
    a.ltiles = (int)cdiv(dims[5], 16);
    a.atiles = (int)cdiv(dims[3], 16);
    a.cblocks = (int)cdiv(dims[1], HD_COLS);
    const int64_t tiles = (int64_t)a.ltiles * a.atiles;             // below 2^56
    if (tiles > PLAN_MAX_EXTENT || tiles * a.cblocks > PLAN_MAX_EXTENT || tiles * a.cblocks * dims[4] > PLAN_MAX_EXTENT)
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_hadamard_apply: 2^31 workgroups or more");
    p->blocks = tiles * a.cblocks * dims[4];
    p->flops = 2.0 * (double)dims[5] * (double)dims[4] * ((double)dims[0] * dims[2] * dims[3] + (double)dims[0] * dims[1] * dims[3]);
    return TTSK_OK;
}

}  // namespace ttsk
