// The closing half of one mode of <x o y, u o v>, the inner product of two entrywise products of tensor trains, neither
// of which is formed (ttsk_hadamard_close).  With the chain so far carried through the cores of x and y by
// ttsk_hadamard_apply, Wl ((gamma c), i, p) for the ranks gamma of u, c of v and p = (beta' a') of x o y:
//   T1[i][gamma][p, c']     = sum_c Wl[(gamma s + c), i, p] V[c, i, c']              stage 1, into LDS
//   out[p, gamma' s' + c'] += sum_gamma U[gamma, i, gamma'] T1[i][gamma][p, c']      stage 2, in registers, over i as well
// The (P x S' s') x n array that a composition from ttsk_gemm calls writes only to add it up never exists.
//
// The stages are those of hadamard_stages.h with A = Wl, B = V, C = U, m = p, n = c', kappa = gamma, col = gamma'.  Against
// hadamard_apply_kernel the chain operand depends on the mode index (its row (gamma, c) of mode i starts at
// ((gamma s + c) n + i) P, rows n P apart), and the result is summed over i instead of indexed by it: workgroup (i chunk,
// p tile, c' tile, gamma' block) of four waves runs hd_mode for each i of its chunk on the same accumulators and writes its
// tile of the partial sum to work (ichunks, P, S' s').  ttsk_sum_slices then adds the slices in ascending order into out:
// one workgroup forms each element of a slice in a fixed order and the slices are added in a fixed order, no atomics.
#include "common.h"
#include "prof.h"
#include "hadamard_close_plan.h"
#include "hadamard_stages.h"

namespace ttsk {

namespace {

__global__ __launch_bounds__(256, 2) void hadamard_close_kernel(HadamardCloseArgs g)
{
    extern __shared__ double hc_sm[];
    const int tid = threadIdx.x, lane = tid & 63, x16 = lane & 15;
    int b = (int)blockIdx.x;
    const int gb = b % g.gblocks;
    b /= g.gblocks;
    const int ct0 = b % g.ctiles;
    b /= g.ctiles;
    const int pt = b % g.ptiles, ic = b / g.ptiles;
    const int S1 = g.S1, s1 = g.s1, P = g.P;
    const int p0 = pt * 16, a0 = ct0 * 16, c0 = gb * HD_COLS;
    const int i_begin = ic * g.iper, i_end = i_begin + g.iper < g.n ? i_begin + g.iper : g.n;
    const HdLane ln = {__builtin_amdgcn_readfirstlane(tid >> 6), lane >> 4, x16, p0 + x16 < P, a0 + x16 < s1};

    // stage 1 operands: this lane's column of Wl (over p) and of V (over c')
    const int64_t nP = (int64_t)g.n * P;                                // one row (gamma, c) of Wl
    const double *const Wp = g.Wl + (ln.mok ? p0 + x16 : P - 1);
    const double *const Vp = g.V + (int64_t)(ln.nok ? a0 + x16 : s1 - 1) * g.sV[2];
    int64_t coff[HD_COL_TILES];
    hd_coff(coff, c0, x16, S1, g.sU[2]);
    HdAcc acc;
    hd_zero(acc);
    for (int i = i_begin; i < i_end; ++i)                               // mode i of Wl, of V and of U
        hd_mode(acc, hc_sm, Wp + (int64_t)i * P, Vp + (int64_t)i * g.sV[1], g.U + (int64_t)i * g.sU[1], nP, g.sV[0], g.sU[0], coff,
                g.S, S1, g.s, c0, ln);
    // ---- the slice of this i chunk: register rr of a lane is gamma' = c0 + 16 ct + (lane >> 4) + 4 rr at c' = a0 + (lane & 15)
    const int64_t cols = (int64_t)S1 * s1;
    hd_store(acc, g.work + (int64_t)ic * P * cols + a0 + x16, cols, s1, c0, S1, p0, P, ln);
}

}  // namespace

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_hadamard_close(const double *Wl, const double *U, const double *V, const int64_t *dims, const int64_t *strides, double *out,
                        int accumulate, double *work, int64_t work_doubles, int stream)
{
    TTSK_STREAM(st, stream);
    HadamardClosePlan p;
    const int rc = hadamard_close_plan(Wl, U, V, dims, strides, out, accumulate, work, work_doubles, &p);
    if (rc) { set_error("%s", p.msg); return rc; }
    {
        ProfBracket prof(st, PROF_EVAL, p.flops, "hadamard_close_kernel");
        if (const int lrc = launch(hadamard_close_kernel, dim3((unsigned)p.blocks), dim3(256), HD_LDS, st, p.a)) return lrc;
    }
    const size_t slice = (size_t)(p.slab / p.a.ichunks);
    return ttsk_sum_slices(out, work, p.a.ichunks, slice, slice, accumulate, stream);
}

int ttsk_hadamard_close_layout(const int64_t *dims, int64_t *out)
{
    HadamardClosePlan p;
    if (!out) { set_error("ttsk_hadamard_close_layout: NULL argument"); return TTSK_ERR_ARG; }
    const int rc = hadamard_close_layout(dims, &p);
    if (rc) { set_error("%s", p.msg); return rc; }
    out[0] = p.a.ichunks;
    out[1] = p.slab;
    return TTSK_OK;
}

}  // extern "C"
