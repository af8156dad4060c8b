// Compute-unit budgets of the one-call TT sketch (tt_fused.hip): plain C++, no HIP include, checked on the host by
// tests/test_sketch_split_host.py.
//
// Every batched launch of the sketch used to be planned for the whole device (chain_fused_plan: wpp = n_cu / nb;
// psi_stream_plan: wpp = n_cu / (nb nac)): at 32 tensors on 256 CUs that is one workgroup per CU, and a workgroup of the
// right step (160 KB of LDS), of the left step (84 KB) or of the Psi product (93 KB) leaves no room for another one on its
// CU -- the kernels of the two chains took the chip in turns although they sit on different streams.  A budget is the CU
// count handed to the plan function INSTEAD of the device's: the grid shrinks to it, and the kernels of the other streams
// find free CUs beside it.  Nothing else of a plan changes; 0 stands for the whole device.
//
// What was measured (MI355X, 256 CUs, bench.py's C3: d = 6, n = 200, TT rank 100, l = 50 / r = 100, 32 tensors;
// profiles/split_curve.json, DESIGN.md "CU budgets"):
//  - alone on the chip every kernel takes LESS CU-time the narrower it is planned (256 -> 64 CUs: right step -10 %, left
//    step -20 %, Psi -25 %);
//  - with ONE step in flight a split only lengthens the step: it ends with the slower chain, wpp is whole so the chains
//    cannot be levelled (right 160 / left 64: +7 %, 192 / 64: +10 %), and Psi waits for both;
//  - with TWO steps in flight on two stream pairs the other step's kernels fill what a chain leaves: 160 / 64 with Psi at
//    full width is 2.9 % faster than full width, 192 / 64 2 %, every budget for Psi is no better than none;
//  - at r = 53 (the chains' work nearly equal; budgets forced, the right chain is on chain_wide_kernel there and gets none
//    from the policy) 192 / 64 is 5 % SLOWER with two steps in flight and 54 % slower with one, 128 / 96 and 128 / 128 2-3 %
//    faster with two: the split has to follow the work of the two chains.
// Hence the rule below: only for a caller that keeps sketches in flight on more than one stream pair, one workgroup per
// tensor left free, the others shared out by the chains' work.
#pragma once
#include <cstdint>

namespace ttsk {

struct SketchSplit {
    int right, left, psi;        // CU budgets of the right step, the left step, the Psi product; 0 = the whole device
};

enum SketchFamily { SKETCH_FUSED = 0, SKETCH_OTHER = 1 };   // every interior chain step on chain_step_kernel, or not

struct SketchSplitIn {
    int n_cu, nb, d;
    const int64_t *n;            // mode sizes, d of them
    const int64_t *s, *lt, *rt;  // TT ranks (d + 1), left DRM ranks (d), right DRM ranks in walking order (d): ttsk_tt_sketch's
    bool two_streams;            // the chains run on two streams (false: TTSK_SINGLE_STREAM=1, or one chain only)
    bool pipelined;              // the caller keeps sketches in flight on more than one stream pair
    SketchFamily family;
};

// Below this many tensors nothing was measured (and one tensor's grid, n workgroups, does not fill the chip): full width.
constexpr int SPLIT_MIN_NB = 8;
// One workgroup per tensor stays free for the other step in flight (measured at C3: 160 / 64 of 256 beats 192 / 64), and
// each chain needs one: no split below three.
constexpr int SPLIT_MIN_WPP = 3;

constexpr SketchSplit SKETCH_SPLIT_FULL{0, 0, 0};

// flops of the interior steps of the two chains (both products of a step, per tensor)
inline void sketch_chain_work(const SketchSplitIn &in, double &right, double &left)
{
    right = left = 0;
    for (int mu = 1; mu < in.d - 1; ++mu) {
        const int j = in.d - 1 - mu;
        const double n = (double)in.n[mu], sn = (double)in.s[mu], sp = (double)in.s[mu + 1];
        right += n * sn * (sp * in.rt[j] + (double)in.rt[j] * in.rt[j + 1]);
        left += n * sp * (sn * in.lt[mu] + (double)in.lt[mu] * in.lt[mu + 1]);
    }
}

// Budgets are whole multiples of nb, so that budget / nb is the plan's wpp with no CU left over; the right and left
// budgets together stay within n_cu.  (256 CUs, 32 tensors, C3) gives the measured 160 / 64; other sizes scale it: of the
// wpp = n_cu / nb workgroups a tensor has at full width one stays free, the others go to the chains by their work,
// rounded to the nearest whole one, each chain keeping at least one.  The Psi products stay at full width.
inline SketchSplit sketch_split_policy(const SketchSplitIn &in)
{
    if (!in.two_streams || !in.pipelined || in.family != SKETCH_FUSED) return SKETCH_SPLIT_FULL;
    if (in.nb < SPLIT_MIN_NB || in.n_cu < 1 || in.d < 3) return SKETCH_SPLIT_FULL;
    int wpp = in.n_cu / in.nb;
    // a tensor has at most n workgroups (one slice each): what the smallest interior mode cannot use is not dealt out
    for (int mu = 1; mu < in.d - 1; ++mu)
        if (in.n[mu] < wpp) wpp = (int)in.n[mu];
    if (wpp < SPLIT_MIN_WPP) return SKETCH_SPLIT_FULL;        // a budget would fall below nb
    double wr_flops, wl_flops;
    sketch_chain_work(in, wr_flops, wl_flops);
    if (!(wr_flops > 0) || !(wl_flops > 0)) return SKETCH_SPLIT_FULL;
    const int share = wpp - 1;
    int wr = (int)((double)share * wr_flops / (wr_flops + wl_flops) + 0.5);
    if (wr > share - 1) wr = share - 1;
    if (wr < 1) wr = 1;
    return SketchSplit{wr * in.nb, (share - wr) * in.nb, 0};
}

// What the driver uses: the process-wide setting of ttsk_tt_sketch_split per class (-1: the policy's value, 0: the whole
// device, > 0: that many CUs, at most the device's) over the policy's answer.
inline SketchSplit sketch_split_resolve(const SketchSplitIn &in, const int set[3])
{
    const SketchSplit pol = (set[0] < 0 || set[1] < 0 || set[2] < 0) ? sketch_split_policy(in) : SKETCH_SPLIT_FULL;
    auto pick = [&](int s, int p) { return s < 0 ? p : (s > in.n_cu ? in.n_cu : s); };
    return SketchSplit{pick(set[0], pol.right), pick(set[1], pol.left), pick(set[2], pol.psi)};
}

}  // namespace ttsk
