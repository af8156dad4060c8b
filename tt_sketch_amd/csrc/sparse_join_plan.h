// What the sorted-key join of sparse tensors (sparse_join.hip) is launched with, decided on the host: the argument checks and
// the cover of ttsk_sparse_key_index / ttsk_sparse_join / ttsk_dense_join, the C-order multipliers of the key, the bits the
// sort has to look at, the splitter stride and count, the fixed step counts of the two searches, the grid, the run of
// queries a workgroup owns and the summation depth the tests build their bound from.
//
// Plain C++: no HIP types, so that the plan is compiled and checked by the host compiler alone
// (tests/test_sparse_join_host.py) before any kernel reads it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "ttsk.h"
#include "plan_common.h"

namespace ttsk {

constexpr int SJ_MAX_MODES = 32;                 // rows and multipliers travel as the kernel's argument
// Splitters of a table kept in one workgroup's LDS.  A measured choice between 8192 (64 KB: two workgroups per compute unit)
// and 16384 (128 KB: one): profiles/sparse_join_bench.json, DESIGN section 19.
constexpr int SJ_MAX_SPLIT = 8192;
constexpr int SJ_SPLIT_LIMIT = 16384;            // the largest count a caller may ask for instead (the A/B of the measurement)
constexpr int SJ_THREADS = 256;
constexpr int SJ_QPT = 8;                        // queries of one thread in flight: their dependent probes overlap
constexpr int SJ_WG_PER_CU = 2;                  // grid cap per compute unit: what 64 KB of splitters leave room for
constexpr int64_t SJ_MAX_N = (1ll << 31) - 1;    // nonzeros of a table (the sort counts in int)
// additions a term passes after its thread's serial share: the 6 butterfly steps of a wave, the four waves as
// (w0 + w1) + (w2 + w3) (block_total, wave.h) ...
constexpr int SJ_BLOCK_SUMS = 6 + 2;
// ... and in the closing sum of reduce.hip over the workgroups' totals: ceil(grid / 256) per thread, then one workgroup total
constexpr int SJ_CLOSE_SUMS = 6 + 2;

// key of an index tuple: sum_k idx[row[k] * row_stride + e] * mult[k], the C-order flat index in the logical shape
struct SjKeyMap {
    int64_t mult[SJ_MAX_MODES];
    int64_t row_stride;
    int64_t total;               // prod(shape): every key of an index inside the shape is below it
    int row[SJ_MAX_MODES];       // physical row of logical mode k
    int d;
};

// the index of a table
struct SjIndexPlan {
    SjKeyMap km;
    int bits;                    // low bits of a key the sort looks at: those of total - 1
    int64_t stride;              // splitter j is sorted key j * stride; ceil(N / max_split), 1 for N = 0
    int64_t n_split;             // ceil(N / stride) <= max_split; 0 for N = 0
    char msg[200];               // why not, when the status is not TTSK_OK
};

// the lookup
struct SjJoinPlan {
    SjKeyMap km;                 // of the queries
    int64_t stride, n_split;     // of the table, as in its SjIndexPlan
    int lds_steps;               // halvings that take n_split candidates down to one: ceil(log2(n_split))
    int seg_steps;               // the same for a segment of `stride` keys
    unsigned grid;               // workgroups = partials: min(ceil(Nq / SJ_THREADS), SJ_WG_PER_CU x CUs)
    int64_t run;                 // queries of one workgroup, contiguous: ceil(Nq / grid); thread t takes lo + t, lo + t + 256, ...
    int64_t depth;               // longest chain of additions of the dot: ceil(run / 256) + block + ceil(grid / 256) + closing sum
    size_t lds;                  // bytes of the splitter image
    size_t scratch;              // bytes of the partials
    char msg[200];
};

inline int sj_ceil_log2(int64_t n)
{
    int s = 0;
    while (((int64_t)1 << s) < n) ++s;
    return s;
}

// the checks and the key map every entry shares; `who` names the entry in the message
template <typename Plan>
inline int sj_key_map(const char *who, const int64_t *shape, int d, const void *dev_idx, int64_t row_stride, const int *row_order, uint64_t N,
                      SjKeyMap *km, Plan *p)
{
    if (!shape) PLAN_FAIL(TTSK_ERR_ARG, "%s: NULL shape", who);
    if (d < 1) PLAN_FAIL(TTSK_ERR_ARG, "%s: d = %d must be positive", who, d);
    if (d > SJ_MAX_MODES) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "%s: %d modes, at most %d are covered", who, d, SJ_MAX_MODES);
    if (!dev_idx && N) PLAN_FAIL(TTSK_ERR_ARG, "%s: NULL index matrix", who);
    if (row_stride < 0 || (uint64_t)row_stride < N)
        PLAN_FAIL(TTSK_ERR_ARG, "%s: row_stride %lld below N = %llu", who, (long long)row_stride, (unsigned long long)N);
    for (int k = 0; k < d; ++k) {
        if (shape[k] < 1) PLAN_FAIL(TTSK_ERR_ARG, "%s: mode %d has size %lld", who, k, (long long)shape[k]);
        const int row = row_order ? row_order[k] : k;
        if (row < 0) PLAN_FAIL(TTSK_ERR_ARG, "%s: row_order[%d] = %d", who, k, row);
        km->row[k] = row;
    }
    int64_t total = 1;
    for (int k = d - 1; k >= 0; --k) {
        km->mult[k] = total;
        if (__builtin_mul_overflow(total, shape[k], &total))
            PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "%s: the shape has more than 2^63 - 1 entries, a key is an int64", who);
    }
    km->total = total;
    km->row_stride = row_stride;
    km->d = d;
    return TTSK_OK;
}

inline int sj_check_split(const char *who, int max_split, char *msg, size_t len)
{
    if (max_split < 0 || max_split > SJ_SPLIT_LIMIT) {
        snprintf(msg, len, "%s: max_split = %d, 0 (the default %d) .. %d are covered", who, max_split, SJ_MAX_SPLIT, SJ_SPLIT_LIMIT);
        return TTSK_ERR_ARG;
    }
    return TTSK_OK;
}

// stride and splitter count of a table of N nonzeros
inline void sj_split(uint64_t N, int max_split, int64_t *stride, int64_t *n_split)
{
    const int64_t cap = max_split ? max_split : SJ_MAX_SPLIT;
    *stride = N ? cdiv((int64_t)N, cap) : 1;
    *n_split = cdiv((int64_t)N, *stride);
}

inline int sparse_key_index_plan(const int64_t *shape, int d, const void *dev_idx, int64_t row_stride, const int *row_order, uint64_t N,
                                 const void *dev_val, int max_split, const void *dev_keys, const void *dev_vals, const void *dev_split,
                                 SjIndexPlan *p)
{
    *p = SjIndexPlan{};
    const char *who = "ttsk_sparse_key_index";
    if (N > (uint64_t)SJ_MAX_N) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "%s: %llu nonzeros, below 2^31 is covered", who, (unsigned long long)N);
    if (int rc = sj_key_map(who, shape, d, dev_idx, row_stride, row_order, N, &p->km, p)) return rc;
    if (N && (!dev_val || !dev_keys || !dev_vals || !dev_split)) PLAN_FAIL(TTSK_ERR_ARG, "%s: NULL entries or output", who);
    if (int rc = sj_check_split(who, max_split, p->msg, sizeof(p->msg))) return rc;
    p->bits = 1;
    while (p->bits < 63 && ((int64_t)1 << p->bits) < p->km.total) ++p->bits;
    sj_split(N, max_split, &p->stride, &p->n_split);
    return TTSK_OK;
}

// `dense`: ttsk_dense_join (no table arrays; N_table is not read)
inline int sparse_join_plan(int dense, const void *dev_keys, const void *dev_vals, const void *dev_split, uint64_t N_table, int max_split,
                            const int64_t *shape, int d, const void *dev_qidx, int64_t q_stride, const int *q_row_order, uint64_t Nq,
                            const void *dev_qval, const void *dev_out, const void *dev_dot, int n_cu, SjJoinPlan *p)
{
    *p = SjJoinPlan{};
    const char *who = dense ? "ttsk_dense_join" : "ttsk_sparse_join";
    if (!dense && N_table > (uint64_t)SJ_MAX_N)
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "%s: a table of %llu nonzeros, below 2^31 is covered", who, (unsigned long long)N_table);
    if (int rc = sj_key_map(who, shape, d, dev_qidx, q_stride, q_row_order, Nq, &p->km, p)) return rc;
    if (dense ? !dev_keys : (N_table && (!dev_keys || !dev_vals || !dev_split))) PLAN_FAIL(TTSK_ERR_ARG, "%s: NULL table", who);
    if (!dev_out && !dev_dot) PLAN_FAIL(TTSK_ERR_ARG, "%s: neither dev_out nor dev_dot given", who);
    if (dev_dot && !dev_qval && Nq) PLAN_FAIL(TTSK_ERR_ARG, "%s: the dot needs dev_qval", who);
    if (int rc = sj_check_split(who, max_split, p->msg, sizeof(p->msg))) return rc;
    if (dense) { p->stride = 1; p->n_split = 0; }
    else sj_split(N_table, max_split, &p->stride, &p->n_split);
    p->lds_steps = sj_ceil_log2(p->n_split);
    p->seg_steps = sj_ceil_log2(p->stride);
    if (n_cu < 1) n_cu = 1;
    const int64_t cap = (int64_t)SJ_WG_PER_CU * n_cu, want = cdiv((int64_t)Nq, SJ_THREADS);
    p->grid = (unsigned)(want < cap ? want : cap);
    p->run = p->grid ? cdiv((int64_t)Nq, p->grid) : 0;
    p->depth = cdiv(p->run, SJ_THREADS) + SJ_BLOCK_SUMS + cdiv(p->grid, 256) + SJ_CLOSE_SUMS;
    p->lds = (size_t)p->n_split * 8;
    p->scratch = (size_t)p->grid * 8;
    return TTSK_OK;
}

}  // namespace ttsk
