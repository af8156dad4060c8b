// What the gather kernels (tt_gather.hip, tucker_gather.hip) share: the index matrix as a kernel argument, the staging of
// a wave's 64 tuples, the value / statistics of a lane's own tuple, the workgroup's partial sums and the host tail
// (partials in SCRATCH_MISC, the launch, the closing sum).
#pragma once
#include "common.h"

namespace ttsk {

constexpr int MAX_MODES = 32;

struct GatherIdx {
    const int64_t *idx;
    int64_t row_stride;
    int d;
    int row[MAX_MODES];     // physical row of logical mode k
};

// indices of the lanes' own tuples (e: the lane's tuple, `own`: it has one): sidx[k * 64 + lane]; no tuple, or one beyond
// N, reads as index 0 (valid in every mode), its value is never stored
__device__ __forceinline__ void stage_indices(const GatherIdx &ix, size_t e, bool own, size_t N, int lane, int *sidx)
{
    for (int k = 0; k < ix.d; ++k)
        sidx[k * 64 + lane] = own && e < N ? (int)ix.idx[(int64_t)ix.row[k] * ix.row_stride + (int64_t)e] : 0;
}

// value / statistics of the lane's own tuple of the batch
__device__ __forceinline__ void emit(double t, size_t e, bool own, size_t N, const double *__restrict__ val,
                                     double *__restrict__ out, bool stats, double &s_xt, double &s_tt, double &s_rr)
{
    if (!own || e >= N) return;
    if (out) out[e] = t;
    if (stats) {
        const double x = val[e], r = t - x;
        s_xt = fma(x, t, s_xt);
        s_tt = fma(t, t, s_tt);
        s_rr = fma(r, r, s_rr);
    }
}

// part[block][3]: the workgroup's sums (block_total: the stated order)
__device__ __forceinline__ void store_block_stats(double (&s)[3], double *__restrict__ part)
{
    const double v = block_total(s);
    if (threadIdx.x < 3) part[(size_t)blockIdx.x * 3 + threadIdx.x] = v;
}

// What the entries end in: room for the workgroups' partial sums in SCRATCH_MISC (only if statistics are wanted), the
// gather kernel through `run(part)` (no launch for an empty list), the closing sum of the partials.
template <typename Run>
static int gather_run(unsigned blocks, double *dev_stats, int stream, hipStream_t st, Run &&run)
{
    double *part = nullptr;
    if (dev_stats && blocks) {
        part = (double *)scratch(stream, SCRATCH_MISC, (size_t)blocks * 3 * 8);
        if (!part) return TTSK_ERR_HIP;
    }
    if (blocks)
        if (int rc = run(part)) return rc;
    return dev_stats ? sum_partials(part, blocks, 3, dev_stats, 0, st) : TTSK_OK;
}

}  // namespace ttsk
