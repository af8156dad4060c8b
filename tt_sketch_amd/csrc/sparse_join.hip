// A sparse tensor against another explicit tensor: SparseTensor.gather (tensor.py:275-286 of the reference, a Python dict
// of every nonzero and a loop over the queries) and with it SparseTensor.dot against a sparse or a dense tensor
// (tensor.py:250-255), as a join on sorted keys.  The plan (sparse_join_plan.h) decides everything a launch depends on.
//
// Index of a table (ttsk_sparse_key_index): the key of a nonzero is its C-order flat index in the logical shape; the
// (key, position) pairs are sorted stably (hipcub radix sort over the bits the shape needs), the entries are permuted
// along, and every stride-th sorted key is kept as a splitter.
//
// Lookup (ttsk_sparse_join): a workgroup copies the splitters to LDS once and owns a contiguous run of queries; a thread
// takes SJ_QPT queries at a time, forms their keys in registers and runs the two searches of all of them step by step, so
// that the dependent probes of different queries overlap.  Both searches find the LAST position whose key is <= the query
// (upper_bound stepped back by one) in a fixed number of branch-free halvings: first over the splitters, which leaves one
// segment of at most `stride` sorted keys, then over that segment.  An equal key there is a hit: the last of a run of
// equal keys is, by the stable sort, the last occurrence in the table -- the dict semantics of the reference.
// ttsk_dense_join is the same pass with the key as the element offset of a contiguous dense tensor.
//
// The dot: a thread adds its queries lo + t, lo + t + 256, ... in that order (fma), block_total (wave.h) gives the
// workgroup's total, sum_partials (reduce.hip) adds the workgroups: no atomics, the same bits on every call.
#include <hipcub/hipcub.hpp>
#include "common.h"
#include "sparse_join_plan.h"

namespace ttsk {

__device__ __forceinline__ int64_t sj_key(const int64_t *__restrict__ idx, const SjKeyMap &km, int64_t e)
{
    int64_t key = 0;
    for (int k = 0; k < km.d; ++k) key += idx[(int64_t)km.row[k] * km.row_stride + e] * km.mult[k];
    return key;
}

__global__ __launch_bounds__(256) void sj_key_kernel(const int64_t *__restrict__ idx, SjKeyMap km, int64_t N, uint64_t *__restrict__ keys,
                                                     int *__restrict__ iota)
{
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < N; e += (int64_t)gridDim.x * 256) {
        keys[e] = (uint64_t)sj_key(idx, km, e);
        iota[e] = (int)e;
    }
}

// vals_sorted[i] = val[perm[i]]; splitter j = sorted key j * stride
__global__ __launch_bounds__(256) void sj_finish_kernel(const int *__restrict__ perm, const double *__restrict__ val, const int64_t *__restrict__ keys_sorted,
                                                        int64_t N, int64_t stride, int64_t n_split, double *__restrict__ vals_sorted,
                                                        int64_t *__restrict__ splitters)
{
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
        vals_sorted[i] = val[perm[i]];
        if (i < n_split) splitters[i] = keys_sorted[i * stride];
    }
}

struct SjTable {
    const int64_t *keys;         // DENSE: not read
    const double *vals;          // DENSE: the tensor, km.total entries
    const int64_t *splitters;
    int64_t N, stride;
    int n_split, lds_steps, seg_steps;
};

template <bool DENSE>
__global__ __launch_bounds__(256) void sj_join_kernel(SjTable tb, SjKeyMap km, const int64_t *__restrict__ qidx, int64_t Nq, int64_t run,
                                                      const double *__restrict__ qval, double *__restrict__ out, double *__restrict__ part)
{
    extern __shared__ int64_t spl[];
    if (!DENSE) {
        for (int i = threadIdx.x; i < tb.n_split; i += SJ_THREADS) spl[i] = tb.splitters[i];
        __syncthreads();
    }
    const int64_t lo = (int64_t)blockIdx.x * run, hi = lo + run < Nq ? lo + run : Nq;
    double acc[1] = {0.0};
    for (int64_t e0 = lo + threadIdx.x; e0 < hi; e0 += (int64_t)SJ_THREADS * SJ_QPT) {
        int64_t key[SJ_QPT], pos[SJ_QPT];
        double v[SJ_QPT];
#pragma unroll
        for (int j = 0; j < SJ_QPT; ++j) {
            const int64_t e = e0 + (int64_t)j * SJ_THREADS;
            key[j] = sj_key(qidx, km, e < hi ? e : e0);          // beyond the run: the thread's first query again, never stored
        }
        if (DENSE) {
#pragma unroll
            for (int j = 0; j < SJ_QPT; ++j) v[j] = (uint64_t)key[j] < (uint64_t)km.total ? tb.vals[key[j]] : 0.0;
        } else {
            // the last splitter <= key (splitter 0 if none is: its segment then holds no equal key either)
            int base[SJ_QPT];
#pragma unroll
            for (int j = 0; j < SJ_QPT; ++j) base[j] = 0;
            int len = tb.n_split;
            for (int s = 0; s < tb.lds_steps; ++s) {
                const int half = len >> 1;
#pragma unroll
                for (int j = 0; j < SJ_QPT; ++j) base[j] += spl[base[j] + half] <= key[j] ? half : 0;
                len -= half;
            }
            // the last key <= the query inside the segment that splitter opens
            int64_t glen[SJ_QPT];
#pragma unroll
            for (int j = 0; j < SJ_QPT; ++j) {
                pos[j] = (int64_t)base[j] * tb.stride;
                glen[j] = tb.N - pos[j] < tb.stride ? tb.N - pos[j] : tb.stride;
            }
            for (int s = 0; s < tb.seg_steps; ++s) {
#pragma unroll
                for (int j = 0; j < SJ_QPT; ++j) {
                    const int64_t half = glen[j] >> 1;
                    pos[j] += tb.keys[pos[j] + half] <= key[j] ? half : 0;
                    glen[j] -= half;
                }
            }
#pragma unroll
            for (int j = 0; j < SJ_QPT; ++j) v[j] = tb.keys[pos[j]] == key[j] ? tb.vals[pos[j]] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < SJ_QPT; ++j) {
            const int64_t e = e0 + (int64_t)j * SJ_THREADS;
            if (e < hi) {
                if (out) out[e] = v[j];
                if (part) acc[0] = fma(qval[e], v[j], acc[0]);
            }
        }
    }
    if (part) {
        const double total = block_total(acc);
        if (threadIdx.x == 0) part[blockIdx.x] = total;
    }
}

static unsigned sj_grid(int64_t N)
{
    const int64_t b = cdiv(N, 256);
    return (unsigned)(b > 65536 ? 65536 : b);
}

// what both lookups end in: room for the partials, the kernel over the plan's grid, the closing sum
template <bool DENSE>
static int sj_run(const SjJoinPlan &p, const SjTable &tb, const int64_t *dev_qidx, size_t Nq, const double *dev_qval, double *dev_out,
                  double *dev_dot, int stream, hipStream_t st)
{
    double *part = nullptr;
    if (dev_dot && p.grid) {
        part = (double *)scratch(stream, SCRATCH_MISC, p.scratch);
        if (!part) return TTSK_ERR_HIP;
    }
    if (p.grid)
        if (int rc = launch(sj_join_kernel<DENSE>, dim3(p.grid), dim3(SJ_THREADS), DENSE ? 0 : p.lds, st, tb, p.km, dev_qidx, (int64_t)Nq, p.run,
                            dev_qval, dev_out, part)) return rc;
    return dev_dot ? sum_partials(part, p.grid, 1, dev_dot, 0, st) : TTSK_OK;
}

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_sparse_join_layout(size_t N_table, size_t Nq, int max_split, int64_t *out)
{
    TTSK_ARG(out, "ttsk_sparse_join_layout: NULL argument");
    const int n_cu = device_num_cu();
    if (n_cu < 1) return TTSK_ERR_ARG;
    SjJoinPlan p;
    const int64_t one = 1;
    const void *some = &one;                     // addresses that are only compared with NULL
    if (int rc = sparse_join_plan(0, some, some, some, N_table, max_split, &one, 1, some, (int64_t)Nq, nullptr, Nq, some, some, some, n_cu, &p)) {
        set_error("%s", p.msg);
        return rc;
    }
    const int64_t v[8] = {SJ_MAX_SPLIT, p.stride, p.n_split, p.lds_steps, p.seg_steps, (int64_t)p.grid, p.run, p.depth};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return TTSK_OK;
}

int ttsk_sparse_key_index(const int64_t *shape, int d, const int64_t *dev_idx, int64_t row_stride, const int *row_order, size_t N,
                          const double *dev_val, int max_split, int64_t *dev_keys_sorted, double *dev_vals_sorted, int64_t *dev_splitters,
                          int stream)
{
    SjIndexPlan p;
    if (int rc = sparse_key_index_plan(shape, d, dev_idx, row_stride, row_order, N, dev_val, max_split, dev_keys_sorted, dev_vals_sorted,
                                       dev_splitters, &p)) {
        set_error("%s", p.msg);
        return rc;
    }
    TTSK_STREAM(st, stream);
    if (N == 0) return TTSK_OK;
    size_t temp_bytes = 0;
    TTSK_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, temp_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const int *)nullptr,
                                                (int *)nullptr, (int)N, 0, p.bits, st));
    // scratch: the keys in input order, the positions before and after the sort, hipcub's temporary storage
    const size_t n8 = (N + 1) / 2 * 2;           // the int arrays in units that keep what follows 8-byte aligned
    char *ws = (char *)scratch(stream, SCRATCH_MISC, N * 8 + 2 * n8 * 4 + temp_bytes + 256);
    if (!ws) return TTSK_ERR_HIP;
    uint64_t *keys = (uint64_t *)ws;
    int *iota = (int *)(ws + N * 8), *perm = iota + n8;
    void *temp = ws + N * 8 + 2 * n8 * 4;
    if (int rc = launch(sj_key_kernel, dim3(sj_grid((int64_t)N)), dim3(256), 0, st, dev_idx, p.km, (int64_t)N, keys, iota)) return rc;
    TTSK_HIP(hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys, (uint64_t *)dev_keys_sorted, iota, perm, (int)N, 0, p.bits, st));
    return launch(sj_finish_kernel, dim3(sj_grid((int64_t)N)), dim3(256), 0, st, perm, dev_val, dev_keys_sorted, (int64_t)N, p.stride, p.n_split,
                  dev_vals_sorted, dev_splitters);
}

int ttsk_sparse_join(const int64_t *dev_keys_sorted, const double *dev_vals_sorted, const int64_t *dev_splitters, size_t N_table,
                     int max_split, const int64_t *shape, int d, const int64_t *dev_qidx, int64_t q_row_stride, const int *q_row_order,
                     size_t Nq, const double *dev_qval, double *dev_out, double *dev_dot, int stream)
{
    SjJoinPlan p;
    const int n_cu = device_num_cu();
    if (n_cu < 1) return TTSK_ERR_ARG;
    if (int rc = sparse_join_plan(0, dev_keys_sorted, dev_vals_sorted, dev_splitters, N_table, max_split, shape, d, dev_qidx, q_row_stride,
                                  q_row_order, Nq, dev_qval, dev_out, dev_dot, n_cu, &p)) {
        set_error("%s", p.msg);
        return rc;
    }
    TTSK_STREAM(st, stream);
    if (N_table == 0) {                          // an empty table: every query misses
        if (dev_out && Nq) TTSK_HIP(hipMemsetAsync(dev_out, 0, Nq * 8, st));
        return dev_dot ? sum_partials(nullptr, 0, 1, dev_dot, 0, st) : TTSK_OK;
    }
    SjTable tb{dev_keys_sorted, dev_vals_sorted, dev_splitters, (int64_t)N_table, p.stride, (int)p.n_split, p.lds_steps, p.seg_steps};
    return sj_run<false>(p, tb, dev_qidx, Nq, dev_qval, dev_out, dev_dot, stream, st);
}

int ttsk_dense_join(const double *dev_x, const int64_t *shape, int d, const int64_t *dev_qidx, int64_t q_row_stride, const int *q_row_order,
                    size_t Nq, const double *dev_qval, double *dev_out, double *dev_dot, int stream)
{
    SjJoinPlan p;
    const int n_cu = device_num_cu();
    if (n_cu < 1) return TTSK_ERR_ARG;
    if (int rc = sparse_join_plan(1, dev_x, nullptr, nullptr, 0, 0, shape, d, dev_qidx, q_row_stride, q_row_order, Nq, dev_qval, dev_out, dev_dot,
                                  n_cu, &p)) {
        set_error("%s", p.msg);
        return rc;
    }
    TTSK_STREAM(st, stream);
    SjTable tb{nullptr, dev_x, nullptr, 0, 1, 0, 0, 0};
    return sj_run<true>(p, tb, dev_qidx, Nq, dev_qval, dev_out, dev_dot, stream, st);
}

}  // extern "C"
