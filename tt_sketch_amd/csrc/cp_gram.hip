// Inner product of two CP tensors: <a, b> = sum_{j < N, j' < M} prod_k (A_k^T B_k)[j, j'] for factor matrices A_k (n_k x N)
// and B_k (n_k x M) (Tensor.dot / norm / error(fast=True) with a CPTensor on either side, reference tensor.py:53-88, which
// densifies both).  2 N M sum_k n_k flops and no array of size N x M: the product over the modes stays in registers.
//
// A workgroup of four waves owns a tile of 64 x 64 pairs (j, j') (cp_gram_plan.h); wave w the rows 16 w .. 16 w + 15 as four
// 16 x 16 accumulator tiles.  For each mode the accumulators are A_k^T B_k over i in k-blocks of four (v_mfma_f64_16x16x4):
// both fragments have the same shape, lane l holds row i0 + (l >> 4), column j0 + (l & 15).  The accumulator layout is the
// same for every mode, so the running product `prod *= acc` is lane-local: no LDS, no cross-lane move.  After the last mode
// the tile is summed: the 16 registers of a lane one by one, then block_total (wave.h).
//
// Operand traffic.  The slabs (n_k x 64) of A and of B of a mode are needed by all four waves, or four times over: they come
// once per workgroup, CPG_KC rows at a time, through LDS.  The steps (mode, chunk of rows) of a tile are one stream: the
// loads of step s + 2 are in flight under the matrix instructions of steps s and s + 1, across the mode boundaries, so the
// load latency is paid once per tile and not once per mode (n_k = 12 is ONE step of three k-blocks: 12 matrix
// instructions per wave, less than one trip to L2).  Two LDS buffers, one barrier per step.  Thread t loads column t & 63 of rows (t >> 6) + 4 u: a wave reads one 512-byte run per row; the loader steps
// pointers and forms its 64-bit products once per mode (fp64 matrix instructions do not hide vector
// address work).  Rows past n_k and columns past N / M are selected to zero after a load from a valid address, so a padded
// pair contributes exactly 0 and nothing is read out of bounds.
//
// Order of sums.  Workgroup g owns the tiles g, g + G, ... in ascending order, adds their totals (times the tile's weight:
// with `sym` only tiles with tile(j) <= tile(j') are formed, those above the diagonal count twice) in that order and writes
// one partial; the library's closing sum (reduce.hip) adds the partials.  No atomics; G depends on the shapes, `sym` and the
// CU count alone: the same bits on every call.
#include "common.h"
#include "prof.h"
#include "cp_gram_plan.h"

namespace ttsk {

namespace {

__global__ __launch_bounds__(256, CPG_WG_PER_CU) void cp_gram_kernel(CpGramArgs g)
{
    __shared__ double slab[2][2][CPG_KC * CPG_PITCH];              // [buffer][A, B][row i][column]
    const int tid = threadIdx.x, lane = tid & 63, x16 = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = tid >> 6, lc = tid & 63;                        // the loader: rows lr + 4 u, column lc of the slabs
    const int d = g.d;
    double total = 0.0;

    for (int64_t t = blockIdx.x; t < g.tiles; t += gridDim.x) {
        const CpGramTile T = cp_gram_tile(g.tn, g.tm, g.sym, t);
        const int ja = T.ti * CPG_TILE + lc, jb = T.tj * CPG_TILE + lc;
        const bool aok = ja < g.N, bok = jb < g.M;
        const int ca = aok ? ja : g.N - 1, cb = bok ? jb : g.M - 1;

        // ---- the loader: step (lk, li0) of the tile's stream, two ahead of the matrix instructions
        int lk = 0;
        int64_t li0 = 0, ln = g.n[0], sa = 4 * g.lda[0], sb = 4 * g.ldb[0];
        const double *pa = g.a[0] + ca, *pb = g.b[0] + cb;        // row 0 of the lane's column: always valid
        const double *ra = pa + lr * g.lda[0], *rb = pb + lr * g.ldb[0];
        // Raw values and the row tests only: the select to zero happens where the step is written to LDS, two steps later.
        // (With the select beside the load the compiler branches around each pair of loads and waits for it there.)  Past
        // the stream's end ln = 0: every row fails its test and the loads repeat a valid address.
        struct Staged { double a[4], b[4]; unsigned rows; };
        auto fetch = [&](Staged &x) {
            x.rows = 0;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool rok = li0 + lr + 4 * u < ln;
                x.a[u] = *(rok ? ra : pa);
                x.b[u] = *(rok ? rb : pb);
                x.rows |= (unsigned)rok << u;
                ra += sa; rb += sb;
            }
            li0 += CPG_KC;
            if (li0 >= ln) {
                li0 = 0; ln = 0;
                if (++lk < d) {                                    // the next mode: its 64-bit products, once
                    ln = g.n[lk]; sa = 4 * g.lda[lk]; sb = 4 * g.ldb[lk];
                    pa = g.a[lk] + ca; pb = g.b[lk] + cb;
                    ra = pa + lr * g.lda[lk]; rb = pb + lr * g.ldb[lk];
                }
            }
        };

        // ---- the matrix instructions: step (k, i0), its operands staged in x and written to LDS buffer `buf`
        v4d prod[4], acc[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) { prod[c] = v4d{1.0, 1.0, 1.0, 1.0}; acc[c] = v4d{0.0, 0.0, 0.0, 0.0}; }
        int k = 0;
        int64_t i0 = 0, n = g.n[0];
        auto step = [&](Staged &x, double *As, double *Bs) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool rok = (x.rows >> u) & 1;
                As[(lr + 4 * u) * CPG_PITCH + lc] = rok && aok ? x.a[u] : 0.0;
                Bs[(lr + 4 * u) * CPG_PITCH + lc] = rok && bok ? x.b[u] : 0.0;
            }
            // the buffer written now was last read two steps ago, before the barrier of the step between
            __syncthreads();
            fetch(x);
            const int kbs = n - i0 < CPG_KC ? (int)((n - i0 + 3) >> 2) : CPG_KC / 4;
            const double *af = As + kq * CPG_PITCH + 16 * wave + x16, *bf = Bs + kq * CPG_PITCH + x16;
            // the fragments of k-block kb + 1 are read under the matrix instructions of kb (past the last: kb again)
            double a = LDS_UNPAIRED(af[0]), b[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = LDS_UNPAIRED(bf[16 * c]);
            for (int kb = 0; kb < kbs; ++kb) {
                const int fwd = kb + 1 < kbs ? 4 * CPG_PITCH : 0;
                af += fwd; bf += fwd;
                const double na = LDS_UNPAIRED(af[0]);
                double nb[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) nb[c] = LDS_UNPAIRED(bf[16 * c]);
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] = mfma16(a, b[c], acc[c]);
                a = na;
#pragma unroll
                for (int c = 0; c < 4; ++c) b[c] = nb[c];
            }
            i0 += CPG_KC;
            if (i0 >= n) {                                         // the mode is complete
#pragma unroll
                for (int c = 0; c < 4; ++c) { prod[c] *= acc[c]; acc[c] = v4d{0.0, 0.0, 0.0, 0.0}; }
                i0 = 0;
                if (++k < d) n = g.n[k];
            }
        };
        Staged x0, x1;
        fetch(x0);
        fetch(x1);
        for (int64_t s = 0; s < g.steps; s += 2) {
            step(x0, slab[0][0], slab[0][1]);
            if (s + 1 < g.steps) step(x1, slab[1][0], slab[1][1]);
        }
        // ---- the tile's total: the lane's 16 pairs one by one, then the workgroup (the same value in every thread)
        double s[1] = {0.0};
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) s[0] += prod[c][r];
        total += (double)T.weight * block_total(s);
        __syncthreads();                                           // block_total's LDS, and the slabs, before the next tile
    }
    if (tid == 0) g.part[blockIdx.x] = total;
}

}  // namespace

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_cp_gram(const double *const *dev_a, const int64_t *lda, int64_t N, const double *const *dev_b, const int64_t *ldb, int64_t M,
                 const int64_t *shape, int d, int sym, double *dev_out, int stream)
{
    TTSK_STREAM(st, stream);
    const int n_cu = device_num_cu();
    if (n_cu < 1) return TTSK_ERR_HIP;
    CpGramPlan p;
    if (int rc = cp_gram_plan(dev_a, lda, N, dev_b, ldb, M, shape, d, sym, dev_out, n_cu, &p)) {
        set_error("%s", p.msg);
        return rc;
    }
    p.a.part = (double *)scratch(stream, SCRATCH_MISC, p.scratch);
    if (!p.a.part) return TTSK_ERR_HIP;
    {
        ProfBracket prof(st, PROF_EVAL, p.flops, "cp_gram_kernel");      // closed before the reduce below
        if (int rc = launch(cp_gram_kernel, dim3(p.grid), dim3(256), 0, st, p.a)) return rc;
    }
    return sum_partials(p.a.part, p.grid, 1, dev_out, 0, st);
}

}  // extern "C"
