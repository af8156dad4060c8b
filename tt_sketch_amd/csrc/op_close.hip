// The closing half of one mode of <M x, N y>, the inner product of two operator-times-train products, neither of which is
// formed (ttsk_op_close).  With the chain so far carried through the cores of M and x by ttsk_op_apply,
// Wl ((c gamma), i, p) for the ranks c of y, gamma of N and p = (beta' a') of M x:
//   T1[j][c][p, gamma']      = sum_{gamma, i} Wl[(c S + gamma), i, p] N[gamma, j, i, gamma']     stage 1, into LDS
//   out[p, c' S' + gamma']  += sum_c Y[c, j, c'] T1[j][c][p, gamma']                             stage 2, in registers, over j as well
// The (P x s' S') x n_in array that a composition from ttsk_gemm calls writes only to add it up never exists.
//
// The stages are those of hadamard_stages.h with A = Wl, B = N, C = Y, m = p, n = gamma', kappa = c, col = c', and the inner
// index of stage 1 the pair (gamma, i), one run of N (op_close_plan.h refuses an N where it is not).  Against
// hadamard_close_kernel the loop is over j, the in-index of N and the mode index of y, and the chain operand does not
// depend on it: workgroup (j chunk, p tile, gamma' tile, c' block) of four waves runs hd_mode for each j of its chunk on the
// same accumulators, N and Y stepped per j, and writes its tile of the partial sum to work (jchunks, P, s' S').
// ttsk_sum_slices then adds the slices in ascending order into out: one workgroup forms each element of a slice in a fixed
// order and the slices are added in a fixed order, no atomics.
//
// ttsk_op_close_batch does this for many independent pairs in two launches (plan in op_close_batch_plan.h): the table of
// pairs is the kernel's argument, a workgroup finds its pair from blockIdx.x and runs the same body with that pair's plan
// and the row pitch ldw of its Wl, a column slice of the W that ttsk_op_apply wrote for all pairs; a second kernel adds
// every pair's slices in the order of ttsk_sum_slices.  A pair gets the bits of its ttsk_op_close call.
#include "common.h"
#include "prof.h"
#include "op_close_plan.h"
#include "op_close_batch_plan.h"
#include "hadamard_stages.h"

namespace ttsk {

namespace {

// What a workgroup of either kernel does: workgroup b of the pair whose plan is g, with rows of Wl `arow` elements apart.
__device__ __forceinline__ void op_close_body(const OpCloseArgs &g, const int b, const int64_t arow, double *const oc_sm)
{
    const int tid = threadIdx.x, lane = tid & 63, x16 = lane & 15;
    const OpCloseTile w = op_close_tile_of(g, b);
    const int S1 = g.S1, s1 = g.s1, P = g.P;
    const int p0 = w.pt * 16, a0 = w.gt * 16, c0 = w.cb * HD_COLS;
    const int j_begin = w.jc * g.jper, j_end = j_begin + g.jper < g.n_in ? j_begin + g.jper : g.n_in;
    const HdLane ln = {__builtin_amdgcn_readfirstlane(tid >> 6), lane >> 4, x16, p0 + x16 < P, a0 + x16 < S1};

    // stage 1 operands: this lane's column of Wl (over p) and of N (over gamma')
    const double *const Wp = g.Wl + (ln.mok ? p0 + x16 : P - 1);
    const double *const Np = g.N + (int64_t)(ln.nok ? a0 + x16 : S1 - 1) * g.sN[3];
    int64_t coff[HD_COL_TILES];
    hd_coff(coff, c0, x16, s1, g.sY[2]);
    const int k = g.S * g.n_out;                                        // the inner index (gamma, i)
    HdAcc acc;
    hd_zero(acc);
    for (int j = j_begin; j < j_end; ++j)                               // in-index j of N, mode index j of Y
        hd_mode(acc, oc_sm, Wp, Np + (int64_t)j * g.sN[1], g.Y + (int64_t)j * g.sY[1], arow, g.sNk, g.sY[0], coff, g.s, s1, k, c0, ln);
    // ---- the slice of this j chunk: register rr of a lane is c' = c0 + 16 ct + (lane >> 4) + 4 rr at gamma' = a0 + (lane & 15)
    const int64_t cols = (int64_t)s1 * S1;
    hd_store(acc, g.work + (int64_t)w.jc * P * cols + a0 + x16, cols, S1, c0, s1, p0, P, ln);
}

__global__ __launch_bounds__(256, 2) void op_close_kernel(OpCloseArgs g)
{
    extern __shared__ double oc_sm[];
    op_close_body(g, (int)blockIdx.x, (int64_t)g.P, oc_sm);
}

// Many pairs in one launch: the pair of a workgroup comes from blockIdx.x and the block0 of the table, uniform over the
// workgroup, so the lookup and the pair's plan stay in scalar registers (as the term lookup of op_apply_kernel does).
__global__ __launch_bounds__(256, 2) void op_close_batch_kernel(OpCloseBatchArgs g)
{
    extern __shared__ double oc_sm[];
    const OpClosePair &t = g.t[op_close_pair_of(g, (int)blockIdx.x)];
    op_close_body(t.a, (int)blockIdx.x - t.block0, t.ldw, oc_sm);
}

// out (+)= the jchunks slices of every pair, in the order and the association of sum_slices_kernel (vector_ops.hip): from out or
// from zero, the slices added one after the other in ascending order, eight loads in flight.
__global__ __launch_bounds__(256) void op_close_batch_sum_kernel(OpCloseBatchArgs g)
{
    const int p = op_close_sum_pair_of(g, (int)blockIdx.x);
    const OpClosePair &t = g.t[p];
    const size_t n = (size_t)t.slice, nb = t.a.jchunks;
    const int last = p + 1 < g.npairs ? g.t[p + 1].sum0 : (int)gridDim.x;
    const size_t step = (size_t)(last - t.sum0) * 256;
    for (size_t i = (size_t)((int)blockIdx.x - t.sum0) * 256 + threadIdx.x; i < n; i += step) {
        double acc = g.accumulate ? t.out[i] : 0.0;
        const double *q = t.a.work + i;
        size_t b = 0;
        for (; b + 8 <= nb; b += 8, q += 8 * n) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = q[(size_t)u * n];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += v[u];
        }
        for (; b < nb; ++b, q += n) acc += *q;
        t.out[i] = acc;
    }
}

}  // namespace

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_op_close(const double *Wl, const double *N, const double *Y, const int64_t *dims, const int64_t *strides, double *out,
                  int accumulate, double *work, int64_t work_doubles, int stream)
{
    TTSK_STREAM(st, stream);
    OpClosePlan p;
    const int rc = op_close_plan(Wl, N, Y, dims, strides, out, accumulate, work, work_doubles, &p);
    if (rc) { set_error("%s", p.msg); return rc; }
    {
        ProfBracket prof(st, PROF_EVAL, p.flops, "op_close_kernel");
        if (const int lrc = launch(op_close_kernel, dim3((unsigned)p.blocks), dim3(256), HD_LDS, st, p.a)) return lrc;
    }
    const size_t slice = (size_t)(p.slab / p.a.jchunks);
    return ttsk_sum_slices(out, work, p.a.jchunks, slice, slice, accumulate, stream);
}

int ttsk_op_close_layout(const int64_t *dims, int64_t *out)
{
    OpClosePlan p;
    if (!out) { set_error("ttsk_op_close_layout: NULL argument"); return TTSK_ERR_ARG; }
    const int rc = op_close_layout(dims, &p);
    if (rc) { set_error("%s", p.msg); return rc; }
    out[0] = p.a.jchunks;
    out[1] = p.slab;
    return TTSK_OK;
}

int ttsk_op_close_batch(int npairs, const double *const *Wl, const double *const *N, const double *const *Y, const int64_t *dims,
                        const int64_t *strides, const int64_t *ldw, double *const *out, int accumulate, double *work,
                        int64_t work_doubles, int stream)
{
    TTSK_STREAM(st, stream);
    OpCloseBatchPlan p;
    const int rc = op_close_batch_plan(npairs, Wl, N, Y, dims, strides, ldw, out, accumulate, work, work_doubles, &p);
    if (rc) { set_error("%s", p.msg); return rc; }
    {
        ProfBracket prof(st, PROF_EVAL, p.flops, "op_close_batch_kernel");
        if (const int lrc = launch(op_close_batch_kernel, dim3((unsigned)p.blocks), dim3(256), HD_LDS, st, p.a)) return lrc;
    }
    return launch(op_close_batch_sum_kernel, dim3((unsigned)p.sum_blocks), dim3(256), 0, st, p.a);
}

int ttsk_op_close_batch_layout(int npairs, const int64_t *dims, int64_t *out)
{
    OpCloseBatchPlan p;
    const int rc = op_close_batch_layout(npairs, dims, out, &p);
    if (rc) set_error("%s", p.msg);
    return rc;
}

}  // extern "C"
