// One sketch step of the entrywise product of two tensor trains that is never formed (ttsk_hadamard_apply).  The product
// core is P[(beta a), i, (beta' a')] = X[beta, i, beta'] Y[a, i, a'], (R r) x n x (R' r'); with the chain so far L (R, r, l):
//   T1[i][beta][l, a']             = sum_a L[beta, a, l] Y[a, i, a']               stage 1, into LDS
//   W[l, i, w_off + beta' r' + a'] = sum_beta X[beta, i, beta'] T1[i][beta][l, a']   stage 2, in registers
// Nothing is summed over the mode: i is a batch index and sits in the grid.  The chain step, Psi and Omega are then one
// ttsk_gemm each on W (l x n x R' r').
//
// The stages are those of hadamard_stages.h with A = L (rows l apart, the same for every i), B = Y, C = X, m = l, n = a',
// kappa = beta, col = beta'.  Workgroup (i, l tile, a' tile, beta' block) of four waves runs hd_mode once, at its i, and
// stores its tile of W, rows n w_cols apart.  R' > HD_COLS takes further beta' blocks, each of which forms stage 1 again
// (DESIGN section 15).  Two workgroups per CU: 237 VGPRs, 69 632 bytes of LDS.
#include "common.h"
#include "prof.h"
#include "hadamard_plan.h"
#include "hadamard_stages.h"

namespace ttsk {

namespace {

__global__ __launch_bounds__(256, 2) void hadamard_apply_kernel(HadamardArgs g)
{
    extern __shared__ double hd_sm[];
    const int tid = threadIdx.x, lane = tid & 63, x16 = lane & 15;
    int b = (int)blockIdx.x;
    const int cb = b % g.cblocks;
    b /= g.cblocks;
    const int at = b % g.atiles;
    b /= g.atiles;
    const int lt = b % g.ltiles, i = b / g.ltiles;
    const int R1 = g.R1, r1 = g.r1, l = g.l;
    const int l0 = lt * 16, a0 = at * 16, c0 = cb * HD_COLS;
    const HdLane ln = {__builtin_amdgcn_readfirstlane(tid >> 6), lane >> 4, x16, l0 + x16 < l, a0 + x16 < r1};

    // stage 1 operands: this lane's column of L (over l) and of Y (over a'); stage 2: mode i of X
    const double *const Lp = g.L + (ln.mok ? l0 + x16 : l - 1);
    const double *const Yp = g.Y + (int64_t)i * g.sY[1] + (int64_t)(ln.nok ? a0 + x16 : r1 - 1) * g.sY[2];
    const double *const Xp = g.X + (int64_t)i * g.sX[1];
    int64_t coff[HD_COL_TILES];
    hd_coff(coff, c0, x16, R1, g.sX[2]);
    HdAcc acc;
    hd_zero(acc);
    hd_mode(acc, hd_sm, Lp, Yp, Xp, l, g.sY[0], g.sX[0], coff, g.R, R1, g.r, c0, ln);
    // ---- W: register rr of a lane is beta' = c0 + 16 ct + (lane >> 4) + 4 rr at a' = a0 + (lane & 15)
    hd_store(acc, g.W + (int64_t)i * g.w_cols + g.w_off + a0 + x16, (int64_t)g.n * g.w_cols, r1, c0, R1, l0, l, ln);
}

}  // namespace

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_hadamard_apply(const double *L, const double *X, const double *Y, const int64_t *dims, const int64_t *strides,
                        double *W, int64_t w_cols, int64_t w_off, int stream)
{
    TTSK_STREAM(st, stream);
    HadamardPlan p;
    const int rc = hadamard_apply_plan(L, X, Y, dims, strides, W, w_cols, w_off, &p);
    if (rc) { set_error("%s", p.msg); return rc; }
    ProfBracket prof(st, PROF_EVAL, p.flops, "hadamard_apply_kernel");
    return launch(hadamard_apply_kernel, dim3((unsigned)p.blocks), dim3(256), HD_LDS, st, p.a);
}

}  // extern "C"
