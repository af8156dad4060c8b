// What the inner product of two CP tensors (cp_gram.hip) is launched with, decided on the host: the argument checks and the
// cover of ttsk_cp_gram, the kernel's argument, the tiles of (j, j') pairs and their weights, the grid, the partials, the
// flops of the call and the summation depth the tests build their bound from.
//
// Plain C++: no HIP types, so that the plan is compiled and checked by the host compiler alone
// (tests/test_cp_gram_host.py) before any kernel reads it.  The tile map is host and device code under the device
// compiler only.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "ttsk.h"
#include "plan_common.h"

#ifdef __HIPCC__
#define CPG_HD __host__ __device__
#else
#define CPG_HD
#endif

namespace ttsk {

constexpr int CPG_MAX_MODES = 32;                // the factor pointers travel as the kernel's argument
constexpr int CPG_TILE = 64;                     // a workgroup's tile: 64 j x 64 j', wave w the rows 16 w .. 16 w + 15
constexpr int CPG_KC = 16;                       // rows i of a mode's two slabs in LDS at once: four k-blocks
constexpr int CPG_PITCH = 80;                    // doubles per slab row: 32 modulo 64 dwords, so the two rows a half-wave reads fall on disjoint banks
constexpr int CPG_WG_PER_CU = 3;                 // grid cap: three workgroups (three waves per SIMD) per compute unit, which registers and LDS allow
constexpr size_t CPG_LDS = (size_t)2 * 2 * CPG_KC * CPG_PITCH * 8;      // two buffers of (A slab, B slab)
// additions a term passes inside one tile: 16 accumulator registers of a lane one by one, the 6 butterfly steps of a
// wave, the four waves as (w0 + w1) + (w2 + w3)
constexpr int CPG_TILE_SUMS = 16 + 6 + 2;
// ... and in the closing sum of reduce.hip over G partials: ceil(G / 256) per thread, then one workgroup total
constexpr int CPG_CLOSE_SUMS = 6 + 2;

// the kernel's argument
struct CpGramArgs {
    const double *a[CPG_MAX_MODES], *b[CPG_MAX_MODES];      // A_k (n_k x N), B_k (n_k x M): element (i, j) at a[k] + i lda[k] + j
    int64_t lda[CPG_MAX_MODES], ldb[CPG_MAX_MODES];
    int n[CPG_MAX_MODES];
    int d, sym, N, M;
    int tn, tm;                  // tiles along j and along j'
    int64_t tiles;               // sym: those with tile(j) <= tile(j')
    int64_t steps;               // of one tile: sum_k ceil(n_k / CPG_KC) slabs through LDS
    double *part;                // one partial per workgroup
};

// tile t of the launch: rows j0 .. j0 + 63 of A against columns j1 .. j1 + 63 of B, its total counted `weight` times
struct CpGramTile { int ti, tj, weight; };

// first tile index of tile row ti of the upper triangle of tn x tn tiles, rows in ascending order
CPG_HD inline int64_t cp_gram_row_start(int64_t tn, int64_t ti) { return ti * tn - ti * (ti - 1) / 2; }

CPG_HD inline CpGramTile cp_gram_tile(int tn, int tm, int sym, int64_t t)
{
    CpGramTile T;
    if (!sym) {
        T.ti = (int)(t / tm); T.tj = (int)(t - (int64_t)T.ti * tm); T.weight = 1;
        return T;
    }
    // (2 tn + 1)^2 - 8 t < 2^53: exact in a double; the root is off by rounding at most, which the two loops mend
    const double s = 2.0 * tn + 1.0;
    int64_t ti = (int64_t)((s - sqrt(s * s - 8.0 * (double)t)) * 0.5);
    if (ti < 0) ti = 0;
    if (ti > tn - 1) ti = tn - 1;
    while (cp_gram_row_start(tn, ti) > t) --ti;
    while (ti + 1 < tn && cp_gram_row_start(tn, ti + 1) <= t) ++ti;
    T.ti = (int)ti; T.tj = (int)(ti + (t - cp_gram_row_start(tn, ti)));
    T.weight = T.tj > T.ti ? 2 : 1;
    return T;
}

struct CpGramPlan {
    CpGramArgs a;
    unsigned grid;               // workgroups = partials: min(tiles, CPG_WG_PER_CU x CUs); workgroup g owns the tiles g, g + grid, ...
    int64_t run;                 // the longest run of tiles of one workgroup
    double flops;                // 2 sum_k n_k per pair; sym: the N (N + 1) / 2 pairs with j <= j'
    int64_t depth;               // additions and products a term passes: sum_k n_k + (d - 1) + tile + run + closing sum
    size_t scratch;              // bytes of the partials
    char msg[200];               // why not, when the status is not TTSK_OK
};

inline int cp_gram_plan(const double *const *dev_a, const int64_t *lda, int64_t N, const double *const *dev_b, const int64_t *ldb, int64_t M,
                        const int64_t *shape, int d, int sym, double *dev_out, int n_cu, CpGramPlan *p)
{
    *p = CpGramPlan{};
    if (!dev_a || !lda || !dev_b || !ldb || !shape || !dev_out) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_gram: NULL argument");
    if (d < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_gram: d = %d must be positive", d);
    if (d > CPG_MAX_MODES) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_cp_gram: %d modes, at most %d are covered", d, CPG_MAX_MODES);
    if (N < 1 || M < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_gram: N = %lld, M = %lld must be positive", (long long)N, (long long)M);
    for (int k = 0; k < d; ++k)
        if (shape[k] < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_gram: mode %d has size %lld", k, (long long)shape[k]);
    for (int k = 0; k < d; ++k) {
        if (!dev_a[k] || !dev_b[k]) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_gram: factor %d is NULL", k);
        if (lda[k] < N || ldb[k] < M)
            PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_gram: leading dimensions %lld, %lld of mode %d below N = %lld, M = %lld", (long long)lda[k],
                      (long long)ldb[k], k, (long long)N, (long long)M);
    }
    if (sym) {
        if (M != N) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_gram: sym with N = %lld, M = %lld", (long long)N, (long long)M);
        for (int k = 0; k < d; ++k)
            if (dev_b[k] != dev_a[k] || ldb[k] != lda[k]) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_gram: sym, but factor %d of b is not that of a", k);
    }
    // ---- the cover
    if (N > PLAN_MAX_EXTENT || M > PLAN_MAX_EXTENT) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_cp_gram: N or M of 2^31 or more; below 2^31 is covered");
    for (int k = 0; k < d; ++k)
        if (shape[k] > PLAN_MAX_EXTENT)
            PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_cp_gram: mode %d of size %lld, below 2^31 is covered", k, (long long)shape[k]);
    CpGramArgs &a = p->a;
    int64_t sum_n = 0;
    for (int k = 0; k < d; ++k) {
        a.a[k] = dev_a[k]; a.b[k] = dev_b[k];
        a.lda[k] = lda[k]; a.ldb[k] = ldb[k];
        a.n[k] = (int)shape[k];
        sum_n += shape[k];
        a.steps += cdiv(shape[k], CPG_KC);
    }
    a.d = d; a.sym = sym ? 1 : 0; a.N = (int)N; a.M = (int)M;
    a.tn = (int)cdiv(N, CPG_TILE); a.tm = (int)cdiv(M, CPG_TILE);                // below 2^25
    a.tiles = a.sym ? (int64_t)a.tn * (a.tn + 1) / 2 : (int64_t)a.tn * a.tm;       // below 2^50
    if (n_cu < 1) n_cu = 1;
    const int64_t cap = (int64_t)CPG_WG_PER_CU * n_cu;
    p->grid = (unsigned)(a.tiles < cap ? a.tiles : cap);
    p->run = cdiv(a.tiles, p->grid);
    p->scratch = (size_t)p->grid * 8;
    p->flops = 2.0 * (double)sum_n * (a.sym ? 0.5 * (double)N * ((double)N + 1.0) : (double)N * (double)M);
    p->depth = sum_n + (d - 1) + CPG_TILE_SUMS + p->run + cdiv(p->grid, 256) + CPG_CLOSE_SUMS;
    return TTSK_OK;
}

}  // namespace ttsk
