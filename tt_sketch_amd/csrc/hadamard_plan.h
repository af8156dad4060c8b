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
constexpr int64_t HD_MAX_EXTENT = (1ll << 31) - 1;

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

#define HD_PLAN_FAIL(status, ...) do { snprintf(p->msg, sizeof(p->msg), __VA_ARGS__); return status; } while (0)

// dims: R, R', r, r', n, l; strides in elements: X (beta, i, beta') then Y (a, i, a')
inline int hadamard_apply_plan(const double *L, const double *X, const double *Y, const int64_t *dims, const int64_t *strides,
                               double *W, int64_t w_cols, int64_t w_off, HadamardPlan *p)
{
    static const char *const names[6] = {"R", "R'", "r", "r'", "n", "l"};
    *p = HadamardPlan{};
    if (!L || !X || !Y || !dims || !strides || !W) HD_PLAN_FAIL(TTSK_ERR_ARG, "ttsk_hadamard_apply: NULL argument");
    for (int i = 0; i < 6; ++i)
        if (dims[i] < 1) HD_PLAN_FAIL(TTSK_ERR_ARG, "ttsk_hadamard_apply: %s = %lld must be positive", names[i], (long long)dims[i]);
    if (w_cols < 1 || w_off < 0)
        HD_PLAN_FAIL(TTSK_ERR_ARG, "ttsk_hadamard_apply: w_cols = %lld, w_off = %lld", (long long)w_cols, (long long)w_off);
    bool wide = w_cols > HD_MAX_EXTENT;
    for (int i = 0; i < 6; ++i)
        if (dims[i] > HD_MAX_EXTENT) wide = true;
    // (extents below 2^31: the product below is below 2^62)
    if (!wide && (w_off > w_cols || dims[1] * dims[3] > w_cols - w_off))
        HD_PLAN_FAIL(TTSK_ERR_ARG, "ttsk_hadamard_apply: columns %lld + %lld x %lld pass w_cols = %lld", (long long)w_off, (long long)dims[1],
                     (long long)dims[3], (long long)w_cols);
    // ---- the cover
    if (wide) HD_PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_hadamard_apply: an extent of 2^31 or more; below 2^31 is covered");
    HadamardArgs &a = p->a;
    a.L = L; a.X = X; a.Y = Y; a.W = W;
    for (int i = 0; i < 3; ++i) { a.sX[i] = strides[i]; a.sY[i] = strides[3 + i]; }
    a.w_cols = w_cols; a.w_off = w_off;
    a.R = (int)dims[0]; a.R1 = (int)dims[1]; a.r = (int)dims[2]; a.r1 = (int)dims[3]; a.n = (int)dims[4]; a.l = (int)dims[5];
    a.ltiles = (int)cdiv(dims[5], 16);
    a.atiles = (int)cdiv(dims[3], 16);
    a.cblocks = (int)cdiv(dims[1], HD_COLS);
    const int64_t tiles = (int64_t)a.ltiles * a.atiles;             // below 2^56
    if (tiles > HD_MAX_EXTENT || tiles * a.cblocks > HD_MAX_EXTENT || tiles * a.cblocks * dims[4] > HD_MAX_EXTENT)
        HD_PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_hadamard_apply: 2^31 workgroups or more");
    p->blocks = tiles * a.cblocks * dims[4];
    p->flops = 2.0 * (double)dims[5] * (double)dims[4] * ((double)dims[0] * dims[2] * dims[3] + (double)dims[0] * dims[1] * dims[3]);
    return TTSK_OK;
}

#undef HD_PLAN_FAIL

}  // namespace ttsk
