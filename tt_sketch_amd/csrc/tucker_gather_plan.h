// What the evaluation of a Tucker tensor at an index list (tucker_gather.hip) is launched with, decided on the host: the
// argument checks and the cover of ttsk_tucker_gather, the split of the modes into a row group (the leading modes, P =
// prod s_k: the contracted index of the matrix product) and a column group (the trailing modes, Q = prod s_k: its
// columns), the chunks of the core through LDS, the LDS bytes, the grid and the summation depth the tests build their
// bound from.
//
// Plain C++: no HIP types, so that the plan is compiled and checked by the host compiler alone
// (tests/test_tucker_gather_host.py) before any kernel reads it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "ttsk.h"
#include "plan_common.h"

namespace ttsk {

constexpr int TKG_MAX_MODES = 8;                 // the cover: d
constexpr int64_t TKG_MAX_CORE = 1ll << 20;      // ... entries of the core
constexpr int TKG_TILES = 4;                     // tiles of 16 tuples a wave carries: a wave owns 64 tuples, one per lane
constexpr int TKG_BATCH = 4 * 16 * TKG_TILES;    // tuples of a workgroup (four waves) at a time: one residency of a chunk serves them all
constexpr int TKG_MAX_CT = 4;                    // column tiles: Q padded to 16, 32 or 64
constexpr int TKG_KC = 16;                       // rows p of the core (P x Q) in LDS at once: four k-blocks
constexpr int TKG_A_PITCH = 80;                  // doubles per row of a wave's A chunk (64 tuples): 16 modulo 32, so the two rows a half-wave reads fall on disjoint banks
constexpr int TKG_WG_PER_CU = 3;                 // grid cap: workgroups per compute unit, which the LDS allows
constexpr size_t TKG_LDS_LIMIT = 64 * 1024 - 512;   // what the plan stays under: the launcher's limit is the device's LDS per workgroup less the kernel's static LDS
// additions a term passes after the matrix instructions: the column tiles one by one, the 4 butterfly steps over 16 lanes
constexpr int TKG_TAIL_SUMS = TKG_MAX_CT + 4;
// ... and a tuple's term of a statistic: the thread's batches in order, block_total (6 + 2), the closing sum (ceil(G / 256) + 6 + 2)
constexpr int TKG_BLOCK_SUMS = 6 + 2;

// doubles per row of the core chunk: Q padded to 16 ct, 16 modulo 32
inline int tkg_b_pitch(int ct) { return ct == 1 ? 16 : 16 * ct + 16; }

// the kernel's argument
struct TuckerGatherArgs {
    const double *core;                          // (P, Q) contiguous
    const double *fac[TKG_MAX_MODES];            // U_k (s_k, n_k) contiguous: column i read with stride n_k
    int64_t n[TKG_MAX_MODES];
    int s[TKG_MAX_MODES];
    int d, m;                                    // modes 0 .. m - 1 are the row group, m .. d - 1 the column group
    int P, Q;
};

struct TuckerGatherPlan {
    TuckerGatherArgs a;
    int row[TKG_MAX_MODES];      // physical row of the index matrix of logical mode k
    int ct;                      // column tiles: ceil(Q / 16), 1, 2 or 4 (3 runs as 4)
    int chunks;                  // ceil(P / TKG_KC) residencies of the core per batch
    size_t lds;                  // dynamic LDS bytes of a workgroup
    unsigned grid;               // workgroups = partials: min(ceil(N / TKG_BATCH), TKG_WG_PER_CU x CUs); workgroup g owns the batches g, g + grid, ...
    int64_t run;                 // the longest run of batches of one workgroup
    double flops;                // 2 |C| N
    int64_t depth;               // additions and products a term of an entry passes
    int64_t stat_depth;          // ... a term of a statistic, beyond those of its entry
    char msg[200];               // why not, when the status is not TTSK_OK
};

// the cost of a split in cycles of a wave per tuple, up to a common factor: the matrix instructions (P padded to 4 times
// the column tiles) against the strided factor reads (P for the A operand, Q (d - m) for the epilogue), four of which
// cost about what one matrix-instruction cycle does
inline int64_t tkg_split_cost(int64_t P, int64_t Q, int d, int m)
{
    const int64_t ct = cdiv(Q, 16) == 3 ? 4 : cdiv(Q, 16);
    return 4 * (cdiv(P, 4) * 4) * ct + P + Q * (d - m);
}

inline int tucker_gather_plan(const void *dev_core, const void *const *dev_factors, const int64_t *ranks, const int64_t *shape, int d,
                              const void *dev_idx, int64_t row_stride, const int *row_order, size_t N, const void *dev_val,
                              const void *dev_out, const void *dev_stats, int n_cu, TuckerGatherPlan *p)
{
    *p = TuckerGatherPlan{};
    if (!dev_core || !dev_factors || !ranks || !shape) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_tucker_gather: NULL core / factors / ranks / shape");
    if (d < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_tucker_gather: d = %d < 1", d);
    if (!dev_out && !dev_stats) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_tucker_gather: neither dev_out nor dev_stats given");
    if (dev_stats && !dev_val) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_tucker_gather: the statistics need dev_val");
    if (!dev_idx && N != 0) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_tucker_gather: NULL index matrix");
    if (row_stride < 0 || (size_t)row_stride < N)
        PLAN_FAIL(TTSK_ERR_ARG, "ttsk_tucker_gather: row_stride %lld below N = %zu", (long long)row_stride, N);
    if (d > TKG_MAX_MODES) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_tucker_gather: %d modes, at most %d are covered", d, TKG_MAX_MODES);
    for (int k = 0; k < d; ++k) {
        if (!dev_factors[k]) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_tucker_gather: factor %d is NULL", k);
        if (shape[k] < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_tucker_gather: mode %d has size %lld", k, (long long)shape[k]);
        if (ranks[k] < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_tucker_gather: rank %d is %lld", k, (long long)ranks[k]);
        const int row = row_order ? row_order[k] : k;
        if (row < 0) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_tucker_gather: row_order[%d] = %d", k, row);
        p->row[k] = row;
    }
    // ---- the cover
    int64_t core = 1;
    for (int k = 0; k < d; ++k) {
        if (shape[k] > PLAN_MAX_EXTENT)
            PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_tucker_gather: mode %d of size %lld, below 2^31 is covered", k, (long long)shape[k]);
        if (ranks[k] > TKG_MAX_CORE || (core *= ranks[k]) > TKG_MAX_CORE)
            PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_tucker_gather: a core of more than 2^20 entries; up to 2^20 is covered");
    }
    TuckerGatherArgs &a = p->a;
    a.core = (const double *)dev_core;
    for (int k = 0; k < d; ++k) {
        a.fac[k] = (const double *)dev_factors[k];
        a.n[k] = shape[k];
        a.s[k] = (int)ranks[k];
    }
    a.d = d;
    // ---- the split: the cheapest m in 1 .. d with Q <= 64; of equal ones the largest m (m = d, Q = 1, always qualifies)
    int64_t best = -1, Q = 1;
    for (int m = d; m >= 1; --m) {
        if (m < d) Q *= ranks[m];
        if (Q > 16 * TKG_MAX_CT) break;
        const int64_t cost = tkg_split_cost(core / Q, Q, d, m);
        if (best < 0 || cost < best) { best = cost; a.m = m; a.Q = (int)Q; }
    }
    a.P = (int)(core / a.Q);
    p->ct = (int)cdiv(a.Q, 16) == 3 ? 4 : (int)cdiv(a.Q, 16);
    p->chunks = (int)cdiv(a.P, TKG_KC);
    p->lds = ((size_t)TKG_KC * tkg_b_pitch(p->ct) + (size_t)4 * TKG_KC * TKG_A_PITCH + 256) * 8 + (size_t)4 * d * 64 * 4;
    if (p->lds > TKG_LDS_LIMIT) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_tucker_gather: %zu bytes of LDS", p->lds);   // not reached inside the cover
                                          if (n_cu < 1) n_cu = 1;
    const size_t batches = (N + TKG_BATCH - 1) / TKG_BATCH, cap = (size_t)TKG_WG_PER_CU * n_cu;
    p->grid = (unsigned)(batches < cap ? batches : cap);
    p->run = p->grid ? (int64_t)((batches + p->grid - 1) / p->grid) : 0;
    p->flops = 2.0 * (double)core * (double)N;
    // an entry: the d factor products, P terms through the matrix instructions (ascending k-blocks of four), the tail
    p->depth = d + cdiv(a.P, 4) * 4 + TKG_TAIL_SUMS;
    p->stat_depth = 2 + p->run + TKG_BLOCK_SUMS + cdiv(p->grid, 256) + TKG_BLOCK_SUMS;
    return TTSK_OK;
}

}  // namespace ttsk
