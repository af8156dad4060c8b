// What ttsk_tt_assemble_batch (assemble_batch.hip) launches for the pairs of one Omega shape, decided on the host: the
// cover of the fused path, the runs of equally spaced tensors (the groups), the layout of the staging scratch, and per
// launch of the Gram and of the apply stage the group table's `first` / `chunks`, the grid and the LDS.
//
// Plain C++: no HIP types, so that the plan is compiled and checked by the host compiler alone
// (tests/test_assemble_batch_cover.py) before any kernel reads it.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "plan_common.h"

namespace ttsk {

constexpr int AB_TM = 32;            // rows of a tile
constexpr int AB_THREADS = 256;
constexpr int AB_MAXG = 16;          // groups per launch (kernel argument)
constexpr int AB_TILES_PER_WG = 16;  // row tiles a workgroup sweeps (P', Omega' are loaded once for them)
constexpr int AB_COVER_MIN = 56, AB_COVER_MAX = 112;
constexpr size_t AB_LDS_MAX = 160 * 1024;

constexpr int ab_up4(int x) { return (x + 3) & ~3; }
constexpr int ab_up16(int x) { return (x + 15) & ~15; }

// ---------------------------------------------------------------------------------------------------------------------------
// The pairs of one Omega shape (l x r), `T` of them.  Inside the cover the staging scratch holds, in doubles from its start,
//     Os [szO]  Ps [szO]  Gm [szG]  Rinv [szG]  Ginv [szG]  status (T ints, in a block of blk(T) doubles)
// with szO = blk(T l r), szG = blk(T n n), n = min(l, r), blk = round up to 32 doubles.
struct AbShapePlan {
    bool covered;                // the fused path; else every pair goes through ttsk_pinv_begin / _end and ttsk_gemm
    int T, n, K;                 // pairs, min(l, r), max(l, r)
    size_t lr, nn;               // elements of an Omega / a pseudo-inverse, of a Gram matrix
    size_t szO, szG;             // doubles of the Os / Ps regions, of the Gm / Rinv / Ginv regions
    size_t off_Os, off_Ps, off_Gm, off_Rinv, off_Ginv, off_status, bytes;   // offsets in doubles; bytes of the whole
    size_t gram_lds, solve_lds;  // bytes: W (K x n); W and G^-1
    int a, b;                    // fused apply: columns of the Psi tile (right: r, left: l), columns of C
    size_t apply_lds;            // bytes: P' (up4(a) x up16(b)), Omega' (up4(b) x up16(a)), Psi tile, C tile
    bool apply_lds_ok;
};

// pinv_fast: pinv_batch_fast(l, r) of pinv.hip (min(l, r) <= CHOL_ONE_N and a full-rank truncation rule)
inline void ab_shape_plan(int64_t l, int64_t r, int direction, int T, bool pinv_fast, AbShapePlan *p)
{
    *p = AbShapePlan{};
    p->covered = std::min(l, r) <= AB_COVER_MIN && std::max(l, r) <= AB_COVER_MAX && pinv_fast;
    p->T = T;
    if (!p->covered) return;
    p->n = (int)std::min(l, r);
    p->K = (int)std::max(l, r);
    p->lr = (size_t)l * r;
    p->nn = (size_t)p->n * p->n;
    auto blk = [](size_t v) { return (v + 31) & ~(size_t)31; };
    p->szO = blk(T * p->lr);
    p->szG = blk(T * p->nn);
    p->off_Os = 0;
    p->off_Ps = p->off_Os + p->szO;
    p->off_Gm = p->off_Ps + p->szO;
    p->off_Rinv = p->off_Gm + p->szG;
    p->off_Ginv = p->off_Rinv + p->szG;
    p->off_status = p->off_Ginv + p->szG;
    p->bytes = (2 * p->szO + 3 * p->szG + blk((size_t)T)) * 8;
    p->gram_lds = (size_t)p->K * p->n * 8;
    p->solve_lds = ((size_t)p->K * p->n + p->nn) * 8;
    p->a = (int)(direction == 0 ? r : l);
    p->b = (int)(direction == 0 ? l : r);
    p->apply_lds = (size_t)(ab_up4(p->a) * ab_up16(p->b) + ab_up4(p->b) * ab_up16(p->a) + AB_TM * (ab_up16(p->a) + 2) +
                            AB_TM * (ab_up16(p->b) + 2)) * 8;
    p->apply_lds_ok = p->apply_lds <= AB_LDS_MAX;
}

// the two refusals of the fused path, in the order the driver meets them (buf: 200 chars)
inline void ab_msg_jacobi(char *buf, size_t len, int64_t l, int64_t r)
{
    snprintf(buf, len, "ttsk_tt_assemble_batch: Jacobi kernel outside its LDS cover (%lld x %lld)", (long long)l, (long long)r);
}
inline void ab_msg_lds(char *buf, size_t len) { snprintf(buf, len, "ttsk_tt_assemble_batch: LDS of the fused apply"); }

// ---------------------------------------------------------------------------------------------------------------------------
// The grouping.  One pair's operands as element offsets (doubles) from any common origin; `k` its mode, `m` its rows.
struct AbPairOff {
    int64_t psi, om, c, work;
    int64_t m;
    int k;
};
// a run of `count` tensors of one mode whose operands are equally spaced: pair first + t at (offset of pair first) + t * stride
struct AbGroupPlan {
    int first, count;            // index of its first pair (= its place in the staging buffers), tensors
    int64_t s_psi, s_om, s_c, s_work;
    int64_t m;
};

inline std::vector<AbGroupPlan> ab_make_groups(const std::vector<AbPairOff> &pairs)
{
    std::vector<AbGroupPlan> out;
    for (size_t i = 0; i < pairs.size();) {
        size_t j = i + 1;
        const AbPairOff &p0 = pairs[i];
        int64_t dpsi = 0, dom = 0, dc = 0, dw = 0;
        if (j < pairs.size() && pairs[j].k == p0.k) {
            dpsi = pairs[j].psi - p0.psi; dom = pairs[j].om - p0.om; dc = pairs[j].c - p0.c; dw = pairs[j].work - p0.work;
        }
        while (j < pairs.size() && pairs[j].k == p0.k && pairs[j].psi - pairs[j - 1].psi == dpsi && pairs[j].om - pairs[j - 1].om == dom &&
               pairs[j].c - pairs[j - 1].c == dc && pairs[j].work - pairs[j - 1].work == dw)
            ++j;
        AbGroupPlan g{};
        g.first = (int)i; g.count = (int)(j - i);
        g.s_psi = dpsi; g.s_om = dom; g.s_c = dc; g.s_work = dw;
        g.m = p0.m;
        out.push_back(g);
        i = j;
    }
    return out;
}

// ---------------------------------------------------------------------------------------------------------------------------
// One launch: the groups [g0, g0 + ng) of the shape, ng <= AB_MAXG.
struct AbLaunchPlan {
    int g0, ng;
    int base;                    // Gram stage: the pair index of the launch's first tensor (the staging regions are rebased by it)
    int wgs;                     // workgroups
    int first[AB_MAXG];          // per group: its first workgroup (Gram: = its first pair - base)
    int chunks[AB_MAXG];         // per group: workgroups per tensor (Gram: 1)
};

inline int ab_launches(size_t groups) { return (int)((groups + AB_MAXG - 1) / AB_MAXG); }

// Gram stage: workgroup = pair; the groups of a launch follow one another in the pair order
inline void ab_gram_launch(const std::vector<AbGroupPlan> &groups, size_t g0, AbLaunchPlan *t)
{
    *t = AbLaunchPlan{};
    t->g0 = (int)g0;
    t->ng = (int)std::min<size_t>(AB_MAXG, groups.size() - g0);
    const AbGroupPlan &last = groups[g0 + t->ng - 1];
    t->wgs = last.first + last.count - groups[g0].first;
    t->base = groups[g0].first;
    for (int i = 0; i < t->ng; ++i) {
        t->first[i] = groups[g0 + i].first - t->base;
        t->chunks[i] = 1;
    }
}

// apply stage: a tensor of a group gets `chunks` workgroups, chunk ch sweeping the row tiles ch, ch + chunks, ...
inline int64_t ab_ntiles(int64_t m) { return (m + AB_TM - 1) / AB_TM; }
inline int ab_chunks(int64_t m) { return (int)std::max<int64_t>(1, (ab_ntiles(m) + AB_TILES_PER_WG - 1) / AB_TILES_PER_WG); }

inline void ab_apply_launch(const std::vector<AbGroupPlan> &groups, size_t g0, AbLaunchPlan *t)
{
    *t = AbLaunchPlan{};
    t->g0 = (int)g0;
    t->ng = (int)std::min<size_t>(AB_MAXG, groups.size() - g0);
    int wgs = 0;
    for (int i = 0; i < t->ng; ++i) {
        const AbGroupPlan &g = groups[g0 + i];
        t->chunks[i] = ab_chunks(g.m);
        t->first[i] = wgs;
        wgs += g.count * t->chunks[i];
    }
    t->wgs = wgs;
}

}  // namespace ttsk
