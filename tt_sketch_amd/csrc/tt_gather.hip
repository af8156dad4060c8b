// Evaluation of a tensor train / a CP tensor at a list of index tuples: TensorTrain.gather (tensor.py:414-440),
// CPTensor.gather (tensor.py:726-732) and, from the same pass, the sums SparseTensor.dot (tensor.py:250-255) and the
// error on the support need.  One launch walks all d modes of a tuple; the running vector of the chain lives in LDS, so
// nothing of size (N x rank) touches HBM (ttsk_sparse_ttdrm_step writes and re-reads such a panel per mode).
//
// Work layout.  A wave takes 64 consecutive tuples at a time: their indices are staged mode by mode, one tuple per lane
// (coalesced 8-byte loads), as 32-bit values in LDS.  The wave is cut into 64 / G groups of G lanes (G = 16 / 32 / 64 by the
// widest rank); group g evaluates tuples g G .. g G + G - 1 of the batch one after the other, and lane s of the group keeps
// the value of the group's s-th tuple -- so after G steps lane t of the wave holds tuple t, and the result is stored, and
// the statistics are accumulated, one tuple per lane again.  (A short list is cut into smaller batches, S < G tuples per
// group, so that it still spreads over the chip: lanes S .. G - 1 of a group then own no tuple.)  Inside a step lane b forms
// out[b] = sum_a v[a] G_k[a, i_k, b] (b strided by G; every a reads one contiguous row of the core through L2); the last
// mode (r_d = 1) is a dot product spread over the lanes and summed by a butterfly.  Every sum has a fixed order: the same
// bits on every call.
#include "gather_common.h"

namespace ttsk {

constexpr int GATHER_MAX_RANK = 256;            // LDS: 4 groups x 2 vectors x 256 doubles = 16 KB at G = 64
constexpr unsigned GATHER_MAX_BLOCKS = 4096;    // a function of N alone, so that the partial sums are too

struct TTCores {
    const double *core[MAX_MODES];
    int n[MAX_MODES];
    int rank[MAX_MODES + 1];
};
struct CPFactors {
    const double *fac[MAX_MODES];
    int rank;
};

template <int G>
__global__ __launch_bounds__(256) void tt_gather_kernel(TTCores tc, GatherIdx ix, size_t N, const double *__restrict__ val,
                                                        double *__restrict__ out, double *__restrict__ part, int rv, int S)
{
    extern __shared__ double sm[];
    constexpr int GPW = 64 / G;                 // groups per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lg = lane & (G - 1), grp = lane / G;
    double *const va = sm + (size_t)((wave * GPW + grp) * 2) * rv, *const vb = va + rv;
    const int d = ix.d;
    int *const sidx = (int *)(sm + (size_t)4 * GPW * 2 * rv) + wave * d * 64;
    double sums[3] = {0.0, 0.0, 0.0};           // x.t, t.t, |t - x|^2
    const size_t tb = (size_t)GPW * S, nbatch = (N + tb - 1) / tb;      // S tuples per group and batch
    const bool own = lg < S;
    for (size_t bt = (size_t)blockIdx.x * 4 + wave; bt < nbatch; bt += (size_t)gridDim.x * 4) {
        const size_t e0 = bt * tb, e_own = e0 + (size_t)grp * S + lg;
        stage_indices(ix, e_own, own, N, lane, sidx);
        wave_lds_sync();
        double mine = 0.0;
        for (int s = 0; s < S; ++s) {
            if (e0 + s >= N) break;             // the first group's tuple is the lowest of the step: wave-uniform
            const int t = grp * G + s;          // the lane that owns this step's tuple
            double *cur = va, *nxt = vb;
            double p = 0.0;
            if (d == 1) {
                p = lg == 0 ? tc.core[0][sidx[t]] : 0.0;
            } else {
                {
                    const int r1 = tc.rank[1];
                    const double *c = tc.core[0] + (int64_t)sidx[t] * r1;
                    for (int b = lg; b < r1; b += G) cur[b] = c[b];
                }
                for (int k = 1; k < d - 1; ++k) {
                    wave_lds_sync();
                    const int r = tc.rank[k], rn = tc.rank[k + 1];
                    const int64_t as = (int64_t)tc.n[k] * rn;
                    const double *c = tc.core[k] + (int64_t)sidx[k * 64 + t] * rn;
                    for (int b = lg; b < rn; b += G) {
                        const double *cb = c + b;
                        double acc = 0.0;
#pragma unroll 4
                        for (int a = 0; a < r; ++a) acc = fma(cur[a], cb[a * as], acc);
                        nxt[b] = acc;
                    }
                    double *sw = cur; cur = nxt; nxt = sw;
                }
                wave_lds_sync();
                const int k = d - 1, r = tc.rank[k];
                const int64_t n = tc.n[k];
                const double *c = tc.core[k] + sidx[k * 64 + t];
#pragma unroll 4
                for (int a = lg; a < r; a += G) p = fma(cur[a], c[a * n], p);
            }
            for (int o = G / 2; o > 0; o >>= 1) p += __shfl_xor(p, o, G);
            if (lg == s) mine = p;
            wave_lds_sync();
        }
        emit(mine, e_own, own, N, val, out, part != nullptr, sums[0], sums[1], sums[2]);
    }
    if (part) store_block_stats(sums, part);
}

// t_e = sum_rho prod_k A_k[i_k(e), rho]: lane rho of the group (strided by G) forms the product over the modes
template <int G>
__global__ __launch_bounds__(256) void cp_gather_kernel(CPFactors cf, GatherIdx ix, size_t N, const double *__restrict__ val,
                                                        double *__restrict__ out, double *__restrict__ part, int S)
{
    extern __shared__ double sm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lg = lane & (G - 1), grp = lane / G;
    const int d = ix.d, R = cf.rank;
    int *const sidx = (int *)sm + wave * d * 64;
    double sums[3] = {0.0, 0.0, 0.0};           // x.t, t.t, |t - x|^2
    const size_t tb = (size_t)(64 / G) * S, nbatch = (N + tb - 1) / tb;
    const bool own = lg < S;
    for (size_t bt = (size_t)blockIdx.x * 4 + wave; bt < nbatch; bt += (size_t)gridDim.x * 4) {
        const size_t e0 = bt * tb, e_own = e0 + (size_t)grp * S + lg;
        wave_lds_sync();
        stage_indices(ix, e_own, own, N, lane, sidx);
        wave_lds_sync();
        double mine = 0.0;
        for (int s = 0; s < S; ++s) {
            if (e0 + s >= N) break;
            const int t = grp * G + s;
            double p = 0.0;
            for (int rho = lg; rho < R; rho += G) {
                double q = cf.fac[0][(int64_t)sidx[t] * R + rho];
                for (int k = 1; k < d; ++k) q *= cf.fac[k][(int64_t)sidx[k * 64 + t] * R + rho];
                p += q;
            }
            for (int o = G / 2; o > 0; o >>= 1) p += __shfl_xor(p, o, G);
            if (lg == s) mine = p;
        }
        emit(mine, e_own, own, N, val, out, part != nullptr, sums[0], sums[1], sums[2]);
    }
    if (part) store_block_stats(sums, part);
}

// what both entries check and set up alike; TTSK_OK with `ix` filled
static int gather_args(const char *who, const void *const *ptrs, const int64_t *shape, int d, const int64_t *dev_idx,
                       int64_t row_stride, const int *row_order, size_t N, const double *dev_val, const double *dev_out,
                       const double *dev_stats, GatherIdx &ix)
{
    TTSK_ARG(ptrs && shape && d >= 1, "%s: NULL cores / shape or d = %d < 1", who, d);
    TTSK_ARG(dev_out || dev_stats, "%s: neither dev_out nor dev_stats given", who);
    TTSK_ARG(!dev_stats || dev_val, "%s: the statistics need dev_val", who);
    TTSK_ARG(dev_idx || N == 0, "%s: NULL index matrix", who);
    TTSK_ARG(row_stride >= 0 && (size_t)row_stride >= N, "%s: row_stride %lld below N = %zu", who, (long long)row_stride, N);
    if (d > MAX_MODES) {
        set_error("%s: %d modes, at most %d are covered", who, d, MAX_MODES);
        return TTSK_ERR_UNSUPPORTED;
    }
    for (int k = 0; k < d; ++k) {
        TTSK_ARG(ptrs[k], "%s: core %d is NULL", who, k);
        TTSK_ARG(shape[k] >= 1, "%s: mode %d has size %lld", who, k, (long long)shape[k]);
        const int row = row_order ? row_order[k] : k;
        TTSK_ARG(row >= 0, "%s: row_order[%d] = %d", who, k, row);
        if (shape[k] >= (1ll << 31)) {
            set_error("%s: mode %d of size %lld, below 2^31 is covered", who, k, (long long)shape[k]);
            return TTSK_ERR_UNSUPPORTED;
        }
        ix.row[k] = row;
    }
    ix.idx = dev_idx;
    ix.row_stride = row_stride;
    ix.d = d;
    return TTSK_OK;
}

// tuples a group takes per batch: G for a long list (one tuple per lane: coalesced index loads and stores), fewer when
// that would leave the list on under ~2048 waves; and the workgroups (four waves, one batch each at a time) for it.
// Both depend on N and G alone, as the order of the partial sums must.
static int gather_steps(size_t N, int G)
{
    const size_t spread = (size_t)2048 * (64 / G), per = (N + spread - 1) / spread;
    return per < 1 ? 1 : per > (size_t)G ? G : (int)per;
}
static unsigned gather_blocks(size_t N, int G, int S)
{
    const size_t tb = (size_t)(64 / G) * S, b = ((N + tb - 1) / tb + 3) / 4;
    return (unsigned)(b > GATHER_MAX_BLOCKS ? GATHER_MAX_BLOCKS : b);
}

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_tt_gather(const double *const *dev_cores, const int64_t *ranks, const int64_t *shape, int d, const int64_t *dev_idx,
                   int64_t row_stride, const int *row_order, size_t N, const double *dev_val, double *dev_out,
                   double *dev_stats, int stream)
{
    TTSK_STREAM(st, stream);
    GatherIdx ix;
    TTSK_ARG(ranks, "ttsk_tt_gather: NULL ranks");
    if (int rc = gather_args("ttsk_tt_gather", (const void *const *)dev_cores, shape, d, dev_idx, row_stride, row_order, N,
                             dev_val, dev_out, dev_stats, ix)) return rc;
    TTSK_ARG(ranks[0] == 1 && ranks[d] == 1, "ttsk_tt_gather: boundary ranks (%lld, %lld) are not 1", (long long)ranks[0],
             (long long)ranks[d]);
    TTCores tc;
    int64_t widest = 1;
    for (int k = 0; k <= d; ++k) {
        TTSK_ARG(ranks[k] >= 1, "ttsk_tt_gather: rank %d is %lld", k, (long long)ranks[k]);
        if (ranks[k] > widest) widest = ranks[k];
    }
    if (widest > GATHER_MAX_RANK) {
        set_error("ttsk_tt_gather: rank %lld, up to %d is covered", (long long)widest, GATHER_MAX_RANK);
        return TTSK_ERR_UNSUPPORTED;
    }
    for (int k = 0; k < d; ++k) {
        tc.core[k] = dev_cores[k];
        tc.n[k] = (int)shape[k];
        tc.rank[k] = (int)ranks[k];
    }
    tc.rank[d] = 1;
    const int G = widest <= 16 ? 16 : widest <= 32 ? 32 : 64, S = gather_steps(N, G);
    const unsigned blocks = gather_blocks(N, G, S);
    const int rv = (int)widest;
    const size_t lds = (size_t)4 * (64 / G) * 2 * rv * 8 + (size_t)4 * d * 64 * 4;
    auto kern = G == 16 ? tt_gather_kernel<16> : G == 32 ? tt_gather_kernel<32> : tt_gather_kernel<64>;
    return gather_run(blocks, dev_stats, stream, st, [&](double *part) {
        return launch(kern, dim3(blocks), dim3(256), lds, st, tc, ix, N, dev_val, dev_out, part, rv, S);
    });
}

int ttsk_cp_gather(const double *const *dev_factors, int64_t rank, const int64_t *shape, int d, const int64_t *dev_idx,
                   int64_t row_stride, const int *row_order, size_t N, const double *dev_val, double *dev_out,
                   double *dev_stats, int stream)
{
    TTSK_STREAM(st, stream);
    GatherIdx ix;
    if (int rc = gather_args("ttsk_cp_gather", (const void *const *)dev_factors, shape, d, dev_idx, row_stride, row_order, N,
                             dev_val, dev_out, dev_stats, ix)) return rc;
    TTSK_ARG(rank >= 1, "ttsk_cp_gather: rank %lld", (long long)rank);
    if (rank >= (1ll << 31)) {
        set_error("ttsk_cp_gather: rank %lld, below 2^31 is covered", (long long)rank);
        return TTSK_ERR_UNSUPPORTED;
    }
    CPFactors cf;
    for (int k = 0; k < d; ++k) cf.fac[k] = dev_factors[k];
    cf.rank = (int)rank;
    const int G = rank <= 16 ? 16 : rank <= 32 ? 32 : 64, S = gather_steps(N, G);
    const unsigned blocks = gather_blocks(N, G, S);
    const size_t lds = (size_t)4 * d * 64 * 4;
    auto kern = G == 16 ? cp_gather_kernel<16> : G == 32 ? cp_gather_kernel<32> : cp_gather_kernel<64>;
    return gather_run(blocks, dev_stats, stream, st, [&](double *part) {
        return launch(kern, dim3(blocks), dim3(256), lds, st, cf, ix, N, dev_val, dev_out, part, S);
    });
}

}  // extern "C"
