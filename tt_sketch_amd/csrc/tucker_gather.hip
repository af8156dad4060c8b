// Evaluation of a Tucker tensor at a list of index tuples (TuckerTensor.to_numpy at single indices, reference
// tensor.py:771-780) and, from the same pass, the sums SparseTensor.dot and the error on the support need:
//   t_e = sum_{a_1..a_d} C[a_1..a_d] prod_k U_k[a_k, i_k(e)]
// 2 |C| flops per tuple, on v_mfma_f64_16x16x4.  All d modes in one launch; nothing of size N x prod(ranks of some modes)
// goes to HBM.
//
// The product.  The plan (tucker_gather_plan.h) cuts the modes into a row group (modes 0 .. m - 1, P = prod s_k) and a
// column group (modes m .. d - 1, Q = prod s_k <= 64).  The core, contiguous in C order, IS the P x Q matrix.  For a tile
// of 16 tuples
//   D[e, q] = sum_p K_e[p] C[p, q],    K_e[p] = prod_{k < m} U_k[a_k(p), i_k(e)]      (A: 16 x P, B: P x Q)
//   t_e     = sum_q D[e, q] W_e[q],    W_e[q] = prod_{k >= m} U_k[b_k(q), i_k(e)]     (the epilogue, vector ALU)
//
// Work layout.  A workgroup of four waves takes TKG_BATCH = 256 consecutive tuples at a time; wave w the 64 tuples 64 w ..
// 64 w + 63 as four tiles, their indices staged one tuple per lane as in tt_gather.hip.  The core goes through LDS in
// chunks of TKG_KC rows p, one residency shared by the four waves and their 16 tiles.  Beside it every wave forms the same
// rows of its own A operand in LDS, lane = tuple: the lane walks p upwards, keeps the product over the slow row modes
// 0 .. m - 2 in a register and forms it anew only when their index changes (every s_{m-1} rows; p is the same in all lanes,
// so the index arithmetic is scalar), and multiplies by U_{m-1}[a, i_e], read with stride n_k straight from the (s_k, n_k)
// factor.  The k-loop then carries LDS reads and matrix instructions only: per k-block one A fragment per tile, one B
// fragment per column tile, 4 x CT instructions (fp64 matrix instructions do not hide vector work).  Both
// pitches are 16 modulo 32 doubles: the two rows a half-wave reads fall on disjoint banks.  Rows past P and columns past Q
// are zeros on both operands.
//
// Order of sums: fixed, the same bits on every call.  An entry: p in ascending k-blocks of four inside the matrix
// instruction; then per lane the column tiles in ascending order (fma), then the xor butterfly 8, 4, 2, 1 over the 16
// lanes of a row.  The products: the slow row modes from m - 2 down to 0, times the fast one; the column modes from d - 1
// down to m.  The statistics: a thread adds its tuples in ascending batches (the workgroup's batches b, b + G, ...),
// block_total (wave.h), the library's closing sum over the G partials (reduce.hip).  G depends on N and the CU count
// alone, and nothing in the sums on dev_out.  No atomics.
#include "gather_common.h"
#include "prof.h"
#include "tucker_gather_plan.h"

namespace ttsk {

namespace {

template <int CT>
__global__ __launch_bounds__(256, CT == 4 ? 1 : 2) void tucker_gather_kernel(TuckerGatherArgs g, GatherIdx ix, size_t N, const double *__restrict__ val,
                                                            double *__restrict__ out, double *__restrict__ part)
{
    extern __shared__ double tkg_sm[];
    constexpr int BP = CT == 1 ? 16 : 16 * CT + 16, AP = TKG_A_PITCH, KC = TKG_KC, QP = 16 * CT;
    const int tid = threadIdx.x, lane = tid & 63, x16 = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double *const Bs = tkg_sm;
    double *const Aw = tkg_sm + KC * BP + wave * (KC * AP);
    double *const res = tkg_sm + KC * BP + 4 * KC * AP + wave * 64;
    int *const sidx = (int *)(tkg_sm + KC * BP + 4 * KC * AP + 256) + wave * ix.d * 64;
    const int d = g.d, m = g.m, P = g.P, Q = g.Q, sf = g.s[m - 1];
    const int64_t nf = g.n[m - 1];
    const int nch = (P + KC - 1) / KC;
    const size_t nbatch = (N + TKG_BATCH - 1) / TKG_BATCH;
    double sums[3] = {0.0, 0.0, 0.0};           // x.t, t.t, |t - x|^2

    for (size_t bt = blockIdx.x; bt < nbatch; bt += gridDim.x) {
        const size_t e_own = bt * TKG_BATCH + (size_t)wave * 64 + lane;
        stage_indices(ix, e_own, true, N, lane, sidx);
        wave_lds_sync();
        const double *const ufast = g.fac[m - 1] + sidx[(m - 1) * 64 + lane];

        v4d acc[TKG_TILES][CT];
#pragma unroll
        for (int t = 0; t < TKG_TILES; ++t)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) acc[t][ct] = v4d{0.0, 0.0, 0.0, 0.0};
        int last_slow = -1;
        double sp = 1.0;                        // the product over the slow row modes at `last_slow`

        for (int c = 0; c < nch; ++c) {
            const int p0 = c * KC;
            // ---- the chunk of the core (rows p0 .. p0 + KC - 1, columns 0 .. 16 CT - 1: CT elements per thread) and the fast
            // factor's entries of the same rows (lane = tuple): every load is in flight before the first is used
            double cv[CT], fv[KC];
#pragma unroll
            for (int u = 0; u < CT; ++u) {
                const int i = tid + 256 * u, r = i / QP, q = i - r * QP, p = p0 + r;
                cv[u] = p < P && q < Q ? g.core[(int64_t)p * Q + q] : 0.0;
            }
#pragma unroll
            for (int r = 0; r < KC; ++r) {
                const int p = p0 + r;           // the same in every lane
                fv[r] = p < P ? ufast[(int64_t)(p % sf) * nf] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < CT; ++u) {
                const int i = tid + 256 * u, r = i / QP, q = i - r * QP;
                Bs[r * BP + q] = cv[u];
            }
            // ---- the same rows of this wave's A operand
#pragma unroll
            for (int r = 0; r < KC; ++r) {
                const int p = p0 + r;
                if (p < P) {
                    const int slow = p / sf;
                    if (slow != last_slow) {
                        sp = 1.0;
                        int rem = slow;
                        for (int k = m - 2; k >= 0; --k) {
                            const int ak = rem % g.s[k];
                            rem /= g.s[k];
                            sp *= g.fac[k][(int64_t)ak * g.n[k] + sidx[k * 64 + lane]];
                        }
                        last_slow = slow;
                    }
                }
                Aw[r * AP + lane] = p < P ? sp * fv[r] : 0.0;
            }
            __syncthreads();
            // ---- the k-blocks of the chunk
            const int left = P - p0, kbn = left >= KC ? KC / 4 : (left + 3) >> 2;
            const double *af = Aw + kq * AP + x16, *bf = Bs + kq * BP + x16;
            // the fragments of k-block kb + 1 are read under the matrix instructions of kb (past the last: kb again)
            double a[TKG_TILES], b[CT];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) b[ct] = LDS_UNPAIRED(bf[16 * ct]);
#pragma unroll
            for (int t = 0; t < TKG_TILES; ++t) a[t] = LDS_UNPAIRED(af[16 * t]);
            for (int kb = 0; kb < kbn; ++kb) {
                if (kb + 1 < kbn) { af += 4 * AP; bf += 4 * BP; }
                double na[TKG_TILES], nb[CT];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) nb[ct] = LDS_UNPAIRED(bf[16 * ct]);
#pragma unroll
                for (int t = 0; t < TKG_TILES; ++t) na[t] = LDS_UNPAIRED(af[16 * t]);
#pragma unroll
                for (int t = 0; t < TKG_TILES; ++t)
#pragma unroll
                    for (int ct = 0; ct < CT; ++ct) acc[t][ct] = mfma16(a[t], b[ct], acc[t][ct]);
#pragma unroll
                for (int t = 0; t < TKG_TILES; ++t) a[t] = na[t];
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) b[ct] = nb[ct];
            }
            __syncthreads();                    // the chunk is read before the next one is written
        }

        // ---- the epilogue: register j of tile t is tuple 16 t + kq + 4 j of the wave at column 16 ct + x16
        double s[TKG_TILES][4];
#pragma unroll
        for (int t = 0; t < TKG_TILES; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) s[t][j] = 0.0;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            const int q = 16 * ct + x16;
            const bool qok = q < Q;
            double w[TKG_TILES][4];
#pragma unroll
            for (int t = 0; t < TKG_TILES; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) w[t][j] = qok ? 1.0 : 0.0;
            int rem = qok ? q : 0;
            for (int k = d - 1; k >= m; --k) {
                const int bk = rem % g.s[k];
                rem /= g.s[k];
                const double *const u = g.fac[k] + (int64_t)bk * g.n[k];
                const int *const si = sidx + k * 64 + kq;
#pragma unroll
                for (int t = 0; t < TKG_TILES; ++t)
#pragma unroll
                    for (int j = 0; j < 4; ++j) w[t][j] *= u[si[16 * t + 4 * j]];
            }
#pragma unroll
            for (int t = 0; t < TKG_TILES; ++t)
#pragma unroll
                for (int j = 0; j < 4; ++j) s[t][j] = fma(acc[t][ct][j], w[t][j], s[t][j]);
        }
#pragma unroll
        for (int t = 0; t < TKG_TILES; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double v = s[t][j];
#pragma unroll
                for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
                if (x16 == 0) res[16 * t + kq + 4 * j] = v;
            }
        wave_lds_sync();
        const double mine = res[lane];
        wave_lds_sync();                        // res and sidx are read before the next batch writes them
        emit(mine, e_own, true, N, val, out, part != nullptr, sums[0], sums[1], sums[2]);
    }
    if (part) store_block_stats(sums, part);
}

}  // namespace

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_tucker_gather(const double *dev_core, const double *const *dev_factors, const int64_t *ranks, const int64_t *shape, int d,
                       const int64_t *dev_idx, int64_t row_stride, const int *row_order, size_t N, const double *dev_val,
                       double *dev_out, double *dev_stats, int stream)
{
    TTSK_STREAM(st, stream);
    const int n_cu = device_num_cu();
    if (n_cu < 1) return TTSK_ERR_HIP;
    TuckerGatherPlan p;
    if (int rc = tucker_gather_plan(dev_core, (const void *const *)dev_factors, ranks, shape, d, dev_idx, row_stride, row_order, N, dev_val,
                                    dev_out, dev_stats, n_cu, &p)) {
        set_error("%s", p.msg);
        return rc;
    }
    GatherIdx ix;
    ix.idx = dev_idx;
    ix.row_stride = row_stride;
    ix.d = d;
    for (int k = 0; k < d; ++k) ix.row[k] = p.row[k];
    auto kern = p.ct == 1 ? tucker_gather_kernel<1> : p.ct == 2 ? tucker_gather_kernel<2> : tucker_gather_kernel<4>;
    return gather_run(p.grid, dev_stats, stream, st, [&](double *part) {
        ProfBracket prof(st, PROF_EVAL, p.flops, "tucker_gather_kernel");
        return launch(kern, dim3(p.grid), dim3(256), p.lds, st, p.a, ix, N, dev_val, dev_out, part);
    });
}

}  // extern "C"
