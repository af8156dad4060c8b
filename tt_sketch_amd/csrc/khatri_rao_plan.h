// What the two Khatri-Rao entry points (khatri_rao.hip) are launched with, decided on the host: the argument checks of
// ttsk_kr_rows and ttsk_kr_step, the number of elements each writes and the grid against its cap.  The entry points call the
// plan, set the error and launch; blocks == 0 is a call with nothing to do (TTSK_OK, no launch).
//
// Plain C++: no HIP types, so that the plans are compiled and checked by the host compiler alone
// (tests/test_khatri_rao_plan.py) before any kernel reads them.  Pointers are tested for NULL, never dereferenced.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "ttsk.h"
#include "plan_common.h"

namespace ttsk {

constexpr int KR_THREADS = 256;                  // threads of a workgroup, both kernels
constexpr int64_t KR_BLOCKS_MAX = 8192;          // workgroups at most: beyond, the grid-stride loop

struct KrPlan {
    int64_t rows;                // rows of `out` the launch writes: n * P (rows), N (step)
    int64_t total;               // elements: rows * w
    int64_t blocks;              // workgroups; 0: nothing to do
    char msg[200];               // why not, when the status is not TTSK_OK
};

// rows * w elements, one thread each up to the cap; the kernels' index runs one grid stride past `total` before the loop ends
inline int kr_grid(const char *who, int64_t rows, int64_t w, KrPlan *p)
{
    int64_t total;
    if (__builtin_mul_overflow(rows, w, &total) || total > INT64_MAX - KR_BLOCKS_MAX * KR_THREADS)
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "%s: %lld rows of %lld columns and one grid stride do not fit in int64_t", who, (long long)rows, (long long)w);
    p->rows = rows;
    p->total = total;
    p->blocks = cdiv(total, KR_THREADS);
    if (p->blocks > KR_BLOCKS_MAX) p->blocks = KR_BLOCKS_MAX;
    return TTSK_OK;
}

// out[i * P + p, c] = prev[p, c] * g[i, c]: prev (P, w) or NULL (P = 1, ones), g (n, w), out (n * P, w)
inline int kr_rows_plan(const double *prev, int64_t P, const double *g, int64_t n, int64_t w, const double *out, KrPlan *p)
{
    *p = KrPlan{};
    if (!g || !out) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_kr_rows: NULL g or out");
    if (n < 1 || w < 1 || P < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_kr_rows: n = %lld, w = %lld, P = %lld must be positive", (long long)n, (long long)w, (long long)P);
    if (!prev && P != 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_kr_rows: NULL prev means P = 1, not %lld", (long long)P);
    int64_t rows;
    if (__builtin_mul_overflow(n, P, &rows)) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_kr_rows: n * P does not fit in int64_t");
    return kr_grid("ttsk_kr_rows", rows, w, p);
}

// out[e, c] = (v ? v[e, c] : 1) * g[idx ? idx[e] : e, c]: v, out (N, w), g (n, w); without idx row e of g is row e of out
inline int kr_step_plan(const double *v, const double *g, int64_t n, int64_t w, const int64_t *idx, size_t N, const double *out, KrPlan *p)
{
    (void)v;
    *p = KrPlan{};
    if (n < 1 || w < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_kr_step: n = %lld, w = %lld must be positive", (long long)n, (long long)w);
    if (N > (size_t)INT64_MAX) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_kr_step: N does not fit in int64_t");
    if (N == 0) return TTSK_OK;
    if (!g || !out) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_kr_step: NULL g or out");
    if (!idx && (int64_t)N > n) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_kr_step: without an index %lld rows are read from a g of %lld", (long long)N, (long long)n);
    return kr_grid("ttsk_kr_step", (int64_t)N, w, p);
}

}  // namespace ttsk
