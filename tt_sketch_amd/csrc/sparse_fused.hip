// SparseTensor x SparseGaussianDRM, streaming sketch, without the (nnz x rank) panels.
//
//   reference: sparse_gaussian_drm.py:29-44 (G[e, k] = ndtri(u(hash(flat_e + hash(k) + seed)))),
//              sparse_sketch.py:8-69      (Psi[:, j, :] = sum_{e: idx_mu[e] = j} val_e L[:, e] R[:, e]^T,
//                                          Omega = (L o val) R^T)
//
// The generator path (sampler.hip + sparse.hip) materialises every L_mu / R_mu as an (nnz x rank) matrix and
// reads it back through the mode permutation: ~18 GB of traffic at C4 for 480 MB of input.  Here one PASS per
// mode mu walks the nonzeros in mode-mu order ONCE and produces Psi_mu -- and one Omega riding along -- with
// every DRM row made where it is consumed:
//   * the nonzeros of a mode are a resident STREAM of records (flat prefix index, flat suffix index, mode
//     index, value) in mode order, built once per tensor (ttsk_sparse_mode_stream): 28 bytes per nonzero and
//     pass, read sequentially; the flat index of the prefix one mode longer (for the Omega that shares the right
//     factor) follows from the record by one multiply-add;
//   * a DRM factor with few possible prefixes / suffixes (the shallow modes: 200 or 30 000 rows at C4) is a
//     TABLE sampled once per sketch and gathered from L2; a deep one is SAMPLED in the pass, bit-identically
//     (same hash, same Cephes ndtri): a wave stages 32 nonzeros, computes the central branch of ndtri in place
//     and queues the tail samples in LDS so that only full waves pay for the tail code (as sample_rows_kernel);
//   * the products run on the matrix cores from the staged tile: lane (x, q) of k-block b holds val A[e][x] and
//     B[e][x] of nonzero e = 4 b + q, the operand layout of v_mfma_f64_16x16x4 (ranks <= 16 per factor);
//   * NO atomics: a wave stores the slices that lie inside its stretch, its first and last (shared) slices go to
//     per-wave partial blocks that a second kernel adds in wave order -- the sketch is bit-reproducible.
// The pass kernel is sparse_pass.h, the plan of its launch sparse_plan.h; here are the kernels that add the partial blocks and
// build the streams, and the entry points.
#include <cstdlib>
#include <hipcub/hipcub.hpp>
#include "sparse_pass.h"
#include "prof.h"

namespace ttsk {

// Psi[:, j, :] += the partial blocks of slice j, waves in ascending order (first-slice partials, then last-slice
// partials): one workgroup per slice, one thread per (a, c); the waves of a slice by bisection (part_j is sorted).
__global__ __launch_bounds__(256) void sg_psi_reduce_kernel(const double *__restrict__ part, const int *__restrict__ pj, int waves,
                                                            int wA, int wB, int64_t n, double *__restrict__ psi)
{
    const int cells = wA * wB;
    for (int64_t j = blockIdx.x; j < n; j += gridDim.x) {
        auto lower = [&](int col, int64_t key) {           // first wave with pj[w][col] >= key
            int lo = 0, hi = waves;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (pj[mid * 3 + col] < key) lo = mid + 1; else hi = mid; }
            return lo;
        };
        const int f0 = lower(0, j), f1 = lower(0, j + 1), l0 = lower(1, j), l1 = lower(1, j + 1);
        if (f0 == f1 && l0 == l1) continue;
        for (int cell = threadIdx.x; cell < cells; cell += 256) {
            double acc = 0.0;
            for (int w = f0; w < f1; ++w) acc += part[((size_t)w * 2) * cells + cell];
            for (int w = l0; w < l1; ++w)
                if (pj[w * 3 + 2]) acc += part[((size_t)w * 2 + 1) * cells + cell];
            const int aa = cell / wB, c = cell - aa * wB;
            psi[((size_t)aa * n + j) * wB + c] += acc;
        }
    }
}

// out[t] += sum_w part[w][t] in wave order.  A 256-wide LDS tree (128, 64, ..., 1), unlike block_total; kept for
// bit-compatibility
__global__ __launch_bounds__(256) void sg_om_reduce_kernel(const double *__restrict__ part, int waves, int cells, double *__restrict__ out)
{
    const int t = blockIdx.x;
    double acc = 0.0;
    for (int w = threadIdx.x; w < waves; w += 256) acc += part[(size_t)w * cells + t];
    __shared__ double red[256];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[t] += red[0];
}

// the resident stream of one mode: record pos = nonzero perm[pos]
template <typename FLAT>
__global__ void sg_stream_kernel(const int64_t *__restrict__ idx, IndexMap lm, IndexMap rm, int64_t mode_off,
                                 const int64_t *__restrict__ perm, const double *__restrict__ val, size_t N, FLAT *__restrict__ fl,
                                 FLAT *__restrict__ fr, int32_t *__restrict__ jj, double *__restrict__ vv)
{
    for (size_t pos = (size_t)blockIdx.x * blockDim.x + threadIdx.x; pos < N; pos += (size_t)gridDim.x * blockDim.x) {
        const size_t e = perm ? (size_t)perm[pos] : pos;
        fl[pos] = (FLAT)(lm.m ? flat_index(idx, lm, e) : 0);
        fr[pos] = (FLAT)(rm.m ? flat_index(idx, rm, e) : 0);
        jj[pos] = (int32_t)idx[mode_off + (int64_t)e];
        vv[pos] = val[e];
    }
}

// sort key of the mode order: (mode index, low 40 bits of the suffix flat index) -- slices in ascending order and,
// inside a slice, the nonzeros in the order of the suffix they share: the rows of a right-hand DRM table are then
// visited in ascending order within every slice (each line fetched once per slice instead of once per nonzero)
__global__ void sg_key_kernel(const int64_t *__restrict__ idx, IndexMap rm, int64_t mode_off, size_t N, uint64_t *__restrict__ keys,
                              int64_t *__restrict__ iota)
{
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < N; e += (size_t)gridDim.x * blockDim.x) {
        const uint64_t suffix = rm.m ? flat_index(idx, rm, e) : 0;
        keys[e] = ((uint64_t)idx[mode_off + (int64_t)e] << 40) | (suffix & ((1ull << 40) - 1));
        iota[e] = (int64_t)e;
    }
}

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_sparse_flat_mult(const uint64_t *shape, int m, uint64_t *mult_out)
{
    TTSK_ARG(shape && mult_out, "ttsk_sparse_flat_mult: NULL argument");
    IndexMap im;
    int rc = make_index_map(shape, m, 0, nullptr, &im);
    if (rc) return rc;
    for (int i = 0; i < m; ++i) mult_out[i] = im.mult[i];
    return TTSK_OK;
}

// perm: the nonzeros in ascending (mode index, suffix flat index) order.  The radix sort is the library's
// (hipcub::DeviceRadixSort, stable): once per tensor and mode, off the per-sketch path.
int ttsk_sparse_mode_order(const int64_t *dev_idx, int64_t row_stride, size_t N, const int *r_rows, const uint64_t *r_shape, int r_m,
                           int mode_row, int64_t n, int64_t *dev_perm, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(dev_idx && dev_perm && r_m >= 0 && mode_row >= 0 && n >= 1, "ttsk_sparse_mode_order: bad argument");
    TTSK_ARG(N < (1ull << 31), "ttsk_sparse_mode_order: more than 2^31 nonzeros");
    // the key holds the mode index in its upper 24 bits (sg_key_kernel): a longer mode would leave index bits out of the
    // sort and the stream out of slice order, which the passes rely on -- refuse it, the panel path takes over
    if (n > (1ll << 24)) {
        set_error("ttsk_sparse_mode_order: mode of %lld entries, the sort key holds 2^24", (long long)n);
        return TTSK_ERR_UNSUPPORTED;
    }
    if (N == 0) return TTSK_OK;
    IndexMap rm{};
    int rc;
    if (r_m && (rc = make_index_map(r_shape, r_m, row_stride, r_rows, &rm))) return rc;
    int bits = 1;
    while ((1ll << bits) < n && bits < 24) ++bits;
    size_t temp_bytes = 0;
    TTSK_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, temp_bytes, (const uint64_t *)nullptr, (uint64_t *)nullptr,
                                                (const int64_t *)nullptr, (int64_t *)nullptr, (int)N, 0, 40 + bits, st));
    char *ws = (char *)scratch(stream, SCRATCH_MISC, 3 * N * 8 + temp_bytes + 256);
    if (!ws) return TTSK_ERR_HIP;
    uint64_t *keys = (uint64_t *)ws, *keys_out = keys + N;
    int64_t *iota = (int64_t *)(keys_out + N);
    void *temp = ws + 3 * N * 8;
    size_t blocks = (N + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    if ((rc = launch(sg_key_kernel, dim3((unsigned)blocks), dim3(256), 0, st, dev_idx, rm, (int64_t)mode_row * row_stride, N, keys, iota))) return rc;
    TTSK_HIP(hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys, keys_out, iota, dev_perm, (int)N, 0, 40 + bits, st));
    return TTSK_OK;
}

static int sg_mode_stream(const int64_t *dev_idx, int64_t row_stride, const int64_t *dev_perm, size_t N, const int *l_rows,
                          const uint64_t *l_shape, int l_m, const int *r_rows, const uint64_t *r_shape, int r_m, int mode_row,
                          const double *dev_val, void *dev_fl, void *dev_fr, int w32, int32_t *dev_j, double *dev_v, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(dev_idx && dev_val && dev_fl && dev_fr && dev_j && dev_v, "ttsk_sparse_mode_stream: NULL argument");
    TTSK_ARG(l_m >= 0 && r_m >= 0 && mode_row >= 0, "ttsk_sparse_mode_stream: bad argument");
    IndexMap lm{}, rm{};
    int rc;
    if (l_m && (rc = make_index_map(l_shape, l_m, row_stride, l_rows, &lm))) return rc;
    if (r_m && (rc = make_index_map(r_shape, r_m, row_stride, r_rows, &rm))) return rc;
    if (N == 0) return TTSK_OK;
    size_t blocks = (N + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    if (w32) {
        // 32-bit records only where every flat index fits (no wrap of the reference's 32-bit running product either)
        double pl = 1.0, pr = 1.0;
        for (int i = 0; i < l_m; ++i) pl *= (double)l_shape[i];
        for (int i = 0; i < r_m; ++i) pr *= (double)r_shape[i];
        if (!(pl < 2147483648.0) || !(pr < 2147483648.0)) {
            set_error("ttsk_sparse_mode_stream_u32: %g prefixes / %g suffixes do not fit 32-bit records", pl, pr);
            return TTSK_ERR_UNSUPPORTED;
        }
        return launch(sg_stream_kernel<uint32_t>, dim3((unsigned)blocks), dim3(256), 0, st, dev_idx, lm, rm, (int64_t)mode_row * row_stride,
                      dev_perm, dev_val, N, (uint32_t *)dev_fl, (uint32_t *)dev_fr, dev_j, dev_v);
    }
    return launch(sg_stream_kernel<uint64_t>, dim3((unsigned)blocks), dim3(256), 0, st, dev_idx, lm, rm, (int64_t)mode_row * row_stride,
                  dev_perm, dev_val, N, (uint64_t *)dev_fl, (uint64_t *)dev_fr, dev_j, dev_v);
}

int ttsk_sparse_mode_stream(const int64_t *dev_idx, int64_t row_stride, const int64_t *dev_perm, size_t N, const int *l_rows,
                            const uint64_t *l_shape, int l_m, const int *r_rows, const uint64_t *r_shape, int r_m, int mode_row,
                            const double *dev_val, uint64_t *dev_fl, uint64_t *dev_fr, int32_t *dev_j, double *dev_v, int stream)
{
    return sg_mode_stream(dev_idx, row_stride, dev_perm, N, l_rows, l_shape, l_m, r_rows, r_shape, r_m, mode_row, dev_val, dev_fl, dev_fr, 0,
                          dev_j, dev_v, stream);
}

int ttsk_sparse_mode_stream_u32(const int64_t *dev_idx, int64_t row_stride, const int64_t *dev_perm, size_t N, const int *l_rows,
                                const uint64_t *l_shape, int l_m, const int *r_rows, const uint64_t *r_shape, int r_m, int mode_row,
                                const double *dev_val, uint32_t *dev_fl, uint32_t *dev_fr, int32_t *dev_j, double *dev_v, int stream)
{
    return sg_mode_stream(dev_idx, row_stride, dev_perm, N, l_rows, l_shape, l_m, r_rows, r_shape, r_m, mode_row, dev_val, dev_fl, dev_fr, 1,
                          dev_j, dev_v, stream);
}

static int sg_gauss_pass(const void *dev_fl, const void *dev_fr, int w32, const int32_t *dev_j, const double *dev_val, size_t N,
                         int64_t n, const ttsk_sg_factor *A, const ttsk_sg_factor *B, const ttsk_sg_factor *C, int c_left,
                         double *dev_psi, double *dev_omega, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(dev_val && dev_psi && n >= 1, "ttsk_sparse_gauss_pass: NULL argument");
    TTSK_ARG(dev_j || n == 1, "ttsk_sparse_gauss_pass: a NULL mode index means a single slice");
    TTSK_ARG(!C || dev_omega, "ttsk_sparse_gauss_pass: an Omega factor needs an output");
    if (N == 0) return TTSK_OK;
    static const size_t n_cu = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        return (size_t)v;
    }();
    SgPlan p;
    int rc = sg_plan(A, B, C, c_left, N, n_cu, &p, w32);
    if (rc) { set_error("%s", p.msg); return rc; }
    SgPass a{};
    a.fl = (const uint64_t *)dev_fl; a.fr = (const uint64_t *)dev_fr; a.w32 = w32; a.jj = dev_j; a.val = dev_val; a.N = N; a.n = n;
    a.chunk = p.chunk; a.c_left = c_left; a.has_om = C != nullptr; a.tcols = p.tcols; a.tab = p.tab; a.qcols = p.qcols; a.psi = dev_psi;
    a.chain = p.chain;
    const ttsk_sg_factor *fs[3] = {A, B, C};
    for (int i = 0; i < 3; ++i) {
        SgF &F = a.f[i];
        F.kind = p.f[i].kind; F.w = p.f[i].w; F.units = p.f[i].units; F.rcp = p.f[i].rcp; a.off[i] = p.f[i].off;
        if (!fs[i]) continue;
        F.rank_min = fs[i]->rank_min; F.src = fs[i]->src; F.mul = fs[i]->mul; F.seed = fs[i]->seed; F.table = fs[i]->table;
        F.full = fs[i]->full; F.nnz = fs[i]->nnz;
        TTSK_ARG(F.kind != 1 || F.table, "ttsk_sparse_gauss_pass: table factor without a table");
        if (F.kind == 4) {
            a.ch[i] = p.ch[i];
            for (int s = 0; s < p.ch[i].steps; ++s) a.core[i][s] = fs[i]->chain->core[s];
            TTSK_ARG(!p.ch[i].has_table == !F.table, "ttsk_sparse_gauss_pass: factor %d: a chain starts at a table exactly when it states its rows", i);
        }
        TTSK_ARG(!((F.src & 1) ? !dev_fr : !dev_fl) || F.kind == 0, "ttsk_sparse_gauss_pass: factor %d needs a flat index stream", i);
    }
#ifdef TTSK_LAB
    { const char *e = getenv("TTSK_SG_LAB"); a.lab = e ? atoi(e) : 0; }
#endif
    char *ws = (char *)scratch(stream, SCRATCH_MISC, p.scratch);
    if (!ws) return TTSK_ERR_HIP;
    a.part_psi = (double *)(ws + p.psi_off);
    a.part_om = (double *)(ws + p.om_off);
    a.part_j = (int *)(ws + p.j_off);
    const int wtot = (int)(p.blocks * 4);
    ProfBracket prof(st, PROF_SPARSE, (w32 ? 20.0 : 28.0) * (double)N, "sg_pass_kernel");
    auto kern = p.NT == 1    ? sg_pass_kernel<1, 0, 32>
                : p.T == 32  ? (p.NS == 1 ? sg_pass_kernel<2, 1, 32> : p.NS == 2 ? sg_pass_kernel<2, 2, 32> : sg_pass_kernel<2, 0, 32>)
                             : (p.NS == 1 ? sg_pass_kernel<2, 1, 16> : p.NS == 2 ? sg_pass_kernel<2, 2, 16> : sg_pass_kernel<2, 0, 16>);
    // the same seven with the chain stage, for a pass with a chain factor
    if (p.has_chain)
        kern = p.NT == 1    ? sg_pass_kernel<1, 0, 32, true>
               : p.T == 32  ? (p.NS == 1 ? sg_pass_kernel<2, 1, 32, true> : p.NS == 2 ? sg_pass_kernel<2, 2, 32, true> : sg_pass_kernel<2, 0, 32, true>)
                            : (p.NS == 1 ? sg_pass_kernel<2, 1, 16, true> : p.NS == 2 ? sg_pass_kernel<2, 2, 16, true> : sg_pass_kernel<2, 0, 16, true>);
    if ((rc = launch(kern, dim3((unsigned)p.blocks), dim3(256), p.lds, st, a))) return rc;
    const int64_t rb = n < 4096 ? n : 4096;
    if ((rc = launch(sg_psi_reduce_kernel, dim3((unsigned)rb), dim3(256), 0, st, a.part_psi, a.part_j, wtot, a.f[0].w, a.f[1].w, n, dev_psi))) return rc;
    if (a.has_om && (rc = launch(sg_om_reduce_kernel, dim3((unsigned)p.cellsO), dim3(256), 0, st, a.part_om, wtot, p.cellsO, dev_omega))) return rc;
    return TTSK_OK;
}

int ttsk_sparse_gauss_pass(const uint64_t *dev_fl, const uint64_t *dev_fr, const int32_t *dev_j, const double *dev_val, size_t N,
                           int64_t n, const ttsk_sg_factor *A, const ttsk_sg_factor *B, const ttsk_sg_factor *C, int c_left,
                           double *dev_psi, double *dev_omega, int stream)
{
    return sg_gauss_pass(dev_fl, dev_fr, 0, dev_j, dev_val, N, n, A, B, C, c_left, dev_psi, dev_omega, stream);
}

int ttsk_sparse_gauss_pass_u32(const uint32_t *dev_fl, const uint32_t *dev_fr, const int32_t *dev_j, const double *dev_val, size_t N,
                               int64_t n, const ttsk_sg_factor *A, const ttsk_sg_factor *B, const ttsk_sg_factor *C, int c_left,
                               double *dev_psi, double *dev_omega, int stream)
{
    return sg_gauss_pass(dev_fl, dev_fr, 1, dev_j, dev_val, N, n, A, B, C, c_left, dev_psi, dev_omega, stream);
}

}  // extern "C"
