// What the closing step of many pairs of operator-times-train products in one launch (ttsk_op_close_batch, op_close.hip)
// is launched with, decided on the host: the argument checks, the table of pairs that travels as the kernel's argument,
// each pair's share of the grid and of the slab, and the flops of the call.
//
// A pair is planned by op_close_plan itself: its cut of j, its tiles and its slab are by construction those of a
// ttsk_op_close call with the same dims.  What this header adds per pair is the row pitch of its Wl, its first workgroup
// and its first double of the slab.
//
// Plain C++: no HIP types, so that the plan is compiled and checked by the host compiler alone
// (tests/test_op_close_batch_host.py) before any kernel reads it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "ttsk.h"
#include "plan_common.h"
#include "op_close_plan.h"

namespace ttsk {

// one pair as the kernels see it
struct OpClosePair {
    OpCloseArgs a;               // of the pair alone; a.work is the pair's part of the slab
    double *out;
    int64_t ldw;                 // elements between consecutive (l, i) rows of Wl, at least P
    int64_t slice;               // doubles of one slice of the pair's slab: P x s' S'
    int block0;                  // first workgroup of the pair in the closing launch
    int sum0;                    // and in the launch that adds its slices
};

constexpr int OP_CLOSE_MAX_PAIRS = 23;           // pairs of one call: the table below travels as the kernel's argument
constexpr int64_t OP_CLOSE_SUM_BLOCKS = 8192;    // workgroups a pair has at most in the adding launch (those of ttsk_sum_slices)

struct OpCloseBatchArgs {
    OpClosePair t[OP_CLOSE_MAX_PAIRS];
    int npairs, accumulate;
};
static_assert(sizeof(OpCloseBatchArgs) <= 4096, "the table of pairs is a kernel argument: 4 KB at most");

struct OpCloseBatchPlan {
    OpCloseBatchArgs a;
    int64_t blocks;              // workgroups of the closing launch
    int64_t sum_blocks;          // of the adding launch
    int64_t slab;                // doubles of `work`: the pairs' slabs one after the other
    double flops;                // summed over the pairs
    char msg[280];               // why not, when the status is not TTSK_OK
};

// The pair a workgroup of the closing launch belongs to (uniform over the workgroup; constexpr so that the kernel and the
// host check run the same lookup).
constexpr int op_close_pair_of(const OpCloseBatchArgs &g, const int block)
{
    int p = 0;
    while (p + 1 < g.npairs && block >= g.t[p + 1].block0) ++p;
    return p;
}

constexpr int op_close_sum_pair_of(const OpCloseBatchArgs &g, const int block)
{
    int p = 0;
    while (p + 1 < g.npairs && block >= g.t[p + 1].sum0) ++p;
    return p;
}

// workgroup b of a pair is (j chunk, p tile, gamma' tile, c' block), the last fastest
struct OpCloseTile {
    int jc, pt, gt, cb;
};

constexpr OpCloseTile op_close_tile_of(const OpCloseArgs &g, int b)
{
    OpCloseTile t = {0, 0, 0, 0};
    t.cb = b % g.cblocks;
    b /= g.cblocks;
    t.gt = b % g.gtiles;
    b /= g.gtiles;
    t.pt = b % g.ptiles;
    t.jc = b / g.ptiles;
    return t;
}

// The part that needs no pointers: offsets[p] is the first double of pair p in the slab, offsets[npairs] the size of the
// slab.  ttsk_op_close_batch_layout is this.
inline int op_close_batch_layout(int npairs, const int64_t *dims, int64_t *offsets, OpCloseBatchPlan *p)
{
    *p = OpCloseBatchPlan{};
    if (!dims || !offsets) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_close_batch: NULL argument");
    if (npairs < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_close_batch: %d pairs", npairs);
    int64_t slab = 0;
    for (int t = 0; t < npairs; ++t) {
        OpClosePlan one;
        if (const int rc = op_close_layout(dims + 7 * t, &one)) PLAN_FAIL(rc, "ttsk_op_close_batch: pair %d: %s", t, one.msg);
        offsets[t] = slab;
        slab += one.slab;                                          // each below 2^45: no list a host holds overflows
    }
    offsets[npairs] = p->slab = slab;
    return TTSK_OK;
}

// dims: npairs x 7 (S, S', s, s', n_in, n_out, P); strides: npairs x 7 in elements, N (gamma, j, i, gamma') then Y (c, j, c')
inline int op_close_batch_plan(int npairs, const double *const *Wl, const double *const *N, const double *const *Y, const int64_t *dims,
                               const int64_t *strides, const int64_t *ldw, double *const *out, int accumulate, double *work,
                               int64_t work_doubles, OpCloseBatchPlan *p)
{
    *p = OpCloseBatchPlan{};
    if (!Wl || !N || !Y || !dims || !strides || !ldw || !out || !work) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_close_batch: NULL argument");
    if (npairs < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_close_batch: %d pairs", npairs);
    if (accumulate != 0 && accumulate != 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_close_batch: accumulate = %d, 0 or 1", accumulate);
    for (int t = 0; t < npairs; ++t) {
        if (!Wl[t] || !N[t] || !Y[t] || !out[t]) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_close_batch: pair %d: NULL pointer", t);
        if (ldw[t] < dims[7 * t + 6])
            PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_close_batch: pair %d: ldw = %lld below P = %lld", t, (long long)ldw[t], (long long)dims[7 * t + 6]);
    }
    // ---- the pairs, each planned as the single call plans it; an argument error of any pair comes before a refusal
    int refused = 0, refused_pair = -1;
    char why[200] = "";
    OpCloseBatchArgs &a = p->a;
    for (int t = 0; t < npairs; ++t) {
        OpClosePlan one;
        const int rc = op_close_plan(Wl[t], N[t], Y[t], dims + 7 * t, strides + 7 * t, out[t], accumulate, work, INT64_MAX, &one);
        if (rc == TTSK_ERR_UNSUPPORTED) {
            if (!refused) { refused = rc; refused_pair = t; snprintf(why, sizeof(why), "%s", one.msg); }
            continue;
        }
        if (rc) PLAN_FAIL(rc, "ttsk_op_close_batch: pair %d: %s", t, one.msg);
        const int64_t slice = one.slab / one.a.jchunks, sb = cdiv(slice, 256);
        if (t < OP_CLOSE_MAX_PAIRS) {                              // a longer list is refused below, after its argument errors
            OpClosePair &T = a.t[t];
            T.a = one.a;
            T.a.work = work + p->slab;
            T.out = out[t];
            T.ldw = ldw[t];
            T.slice = slice;
            T.block0 = (int)(p->blocks < PLAN_MAX_EXTENT ? p->blocks : PLAN_MAX_EXTENT);      // past it the call is refused below
            T.sum0 = (int)p->sum_blocks;
        }
        p->blocks += one.blocks;
        p->sum_blocks += sb < OP_CLOSE_SUM_BLOCKS ? sb : OP_CLOSE_SUM_BLOCKS;
        p->slab += one.slab;
        p->flops += one.flops;
    }
    if (!refused && work_doubles < p->slab)
        PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_close_batch: a slab of %lld doubles, the plan needs %lld", (long long)work_doubles, (long long)p->slab);
    // ---- the cover
    if (npairs > OP_CLOSE_MAX_PAIRS)
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_op_close_batch: %d pairs in one call, up to %d are covered", npairs, OP_CLOSE_MAX_PAIRS);
    if (refused) PLAN_FAIL(refused, "ttsk_op_close_batch: pair %d: %s", refused_pair, why);
    if (p->blocks > PLAN_MAX_EXTENT) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_op_close_batch: 2^31 workgroups or more in all");
    a.npairs = npairs;
    a.accumulate = accumulate;
    return TTSK_OK;
}

}  // namespace ttsk
