// One sketch step of the entrywise product of two tensor trains that is never formed (ttsk_hadamard_apply).  The product
// core is P[(beta a), i, (beta' a')] = X[beta, i, beta'] Y[a, i, a'], (R r) x n x (R' r'); with the chain so far L (R, r, l):
//   T1[i][beta][l, a']             = sum_a L[beta, a, l] Y[a, i, a']               stage 1, into LDS
//   W[l, i, w_off + beta' r' + a'] = sum_beta X[beta, i, beta'] T1[i][beta][l, a']   stage 2, in registers
// Nothing is summed over the mode: i is a batch index and sits in the grid.  The chain step, Psi and Omega are then one
// ttsk_gemm each on W (l x n x R' r').
//
// Workgroup (i, l tile, a' tile, beta' block) of four waves: a 16 x 16 tile of (l, a') and HD_COLS values of beta'.  It walks
// beta in chunks of HD_KC with persistent accumulators, so no R is too long (hadamard_plan.h).
//   stage 1   wave w forms the tiles w, w + 4, ... of the chunk with v_mfma_f64_16x16x4 over a: the A operand [m = l][k = a] is
//             L[beta][a][l0 + lane & 15], 16 lanes one 128-byte run; the B operand [k = a][n = a'] is Y[a, i, a0 + lane & 15],
//             the same for every beta (it stays in cache).  Register r of lane (row (lane >> 4) + 4 r, column lane & 15)
//             goes to T1s[beta of the chunk][l][a'].  The wave's tiles are one stream of fragments with HD_S1_DEPTH loads
//             of each operand in flight across the tile boundaries.  Rows past R inside the last k-block of four are
//             written as zeros, rows beyond it neither formed nor read.
//   stage 2   wave w owns l = 4 w .. 4 w + 3 of the tile and all beta' tiles: out[beta'][a'] += X^T[beta'][kk] T1s[kk][l][a'],
//             the A operand [m = beta'][k = kk] from X through L2 (contiguous over beta' in the stored orientation), the B
//             operand [k = kk][n = a'] from LDS at the conflict-free pitch.  One A fragment serves four matrix instructions,
//             one B fragment up to HD_COL_TILES of them; the X fragments of the next k-block are in flight under this one's.
//             a' sits on the accumulator's lane column, so 16 lanes store one 128-byte run of W.
// The k-block loops step pointers (L and Y by four a, X by four beta); a 64-bit product is formed once per tile or chunk.
// Two workgroups per CU: 237 VGPRs, 69 632 bytes of LDS.
// Operands beyond an extent are zeros selected after a load from a valid address.  R' > HD_COLS takes further beta' blocks,
// each of which forms stage 1 again.  One workgroup forms each element in a fixed order, no atomics: the
// same bits on every call.
#include "common.h"
#include "prof.h"
#include "hadamard_plan.h"

namespace ttsk {

namespace {

constexpr int HD_S1_DEPTH = 8;           // fragments of stage 1 in flight

__global__ __launch_bounds__(256, 2) void hadamard_apply_kernel(HadamardArgs g)
{
    extern __shared__ double hd_sm[];
    double *const T1s = hd_sm;
    const int tid = threadIdx.x, lane = tid & 63, x16 = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int b = (int)blockIdx.x;
    const int cb = b % g.cblocks;
    b /= g.cblocks;
    const int at = b % g.atiles;
    b /= g.atiles;
    const int lt = b % g.ltiles, i = b / g.ltiles;
    const int R = g.R, R1 = g.R1, r = g.r, r1 = g.r1, l = g.l;
    const int l0 = lt * 16, a0 = at * 16, c0 = cb * HD_COLS;
    const int k1 = (r + 3) >> 2;

    // stage 1 operands: this lane's column of L (over l) and of Y (over a'), at a = lane >> 4
    const bool lok = l0 + x16 < l, aok = a0 + x16 < r1;
    const double *const Lp = g.L + (lok ? l0 + x16 : l - 1);
    const double *const Yp = g.Y + (int64_t)i * g.sY[1] + (int64_t)(aok ? a0 + x16 : r1 - 1) * g.sY[2];
    const int64_t lstep = 4 * (int64_t)l, ystep = 4 * g.sY[0];
    // stage 2 operands: this lane's columns beta' of X
    const double *const Xp = g.X + (int64_t)i * g.sX[1];
    const int64_t xstep = 4 * g.sX[0];
    int64_t coff[HD_COL_TILES];
#pragma unroll
    for (int ct = 0; ct < HD_COL_TILES; ++ct) {
        const int col = c0 + ct * 16 + x16;
        coff[ct] = (int64_t)(col < R1 ? col : R1 - 1) * g.sX[2];
    }
    v4d acc[4][HD_COL_TILES];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int ct = 0; ct < HD_COL_TILES; ++ct) acc[u][ct] = v4d{0.0, 0.0, 0.0, 0.0};

    const int nch = (R + HD_KC - 1) / HD_KC;
    for (int ch = 0; ch < nch; ++ch) {
        const int beta0 = ch * HD_KC;
        const int rows = R - beta0 < HD_KC ? R - beta0 : HD_KC;         // beta of this chunk
        const int nkb = (rows + 3) >> 2;                                // its k-blocks of stage 2
        // the X fragments of this lane's next beta; the first k-block's are in flight under stage 1
        const double *xr = Xp + (int64_t)(beta0 + kq) * g.sX[0];
        int beta = beta0 + kq;
        auto rows_of = [&](double *dst) {
            const bool rowok = beta < R;
            const double *const p = rowok ? xr : Xp;
#pragma unroll
            for (int ct = 0; ct < HD_COL_TILES; ++ct) {
                double v = 0.0;
                if (c0 + ct * 16 < R1) v = p[coff[ct]];
                dst[ct] = rowok && c0 + ct * 16 + x16 < R1 ? v : 0.0;
            }
            xr += xstep; beta += 4;
        };
        double mv[HD_COL_TILES], mn[HD_COL_TILES];
        rows_of(mv);
        // ---- stage 1: T1 of the chunk's rows into LDS.  The wave's tiles q = wave, wave + 4, ... (nkb of them, k1 fragments
        // each) are one stream of fragments: HD_S1_DEPTH loads stay in flight across the tile boundaries, so the load
        // latency is paid once per chunk and not once per tile.
        {
            const int total = nkb * k1;
            int lq = wave, lks = 0, la = kq;                            // the loader: tile, k-block, this lane's a
            const double *pl = Lp + ((int64_t)(beta0 + lq) * r + kq) * l, *py = Yp + (int64_t)kq * g.sY[0];
            auto frag = [&](double &lv, double &yv) {
                const bool ok = lq < rows && la < r;                    // past the stream's end lq >= rows: nothing is read
                const double x = *(ok ? pl : Lp), y = *(ok ? py : Yp);
                lv = ok && lok ? x : 0.0;
                yv = ok && aok ? y : 0.0;
                pl += lstep; py += ystep; la += 4;
                if (++lks == k1) {
                    lks = 0; lq += 4; la = kq;
                    pl = Lp + ((int64_t)(beta0 + lq) * r + kq) * l;
                    py = Yp + (int64_t)kq * g.sY[0];
                }
            };
            double cl[HD_S1_DEPTH], cy[HD_S1_DEPTH], nl[HD_S1_DEPTH], ny[HD_S1_DEPTH];
#pragma unroll
            for (int u = 0; u < HD_S1_DEPTH; ++u) frag(cl[u], cy[u]);
            v4d tt = v4d{0.0, 0.0, 0.0, 0.0};
            int cq = wave, cks = 0;                                     // the consumer: tile, k-block
            for (int f = 0; f < total; f += HD_S1_DEPTH) {
#pragma unroll
                for (int u = 0; u < HD_S1_DEPTH; ++u) frag(nl[u], ny[u]);
#pragma unroll
                for (int u = 0; u < HD_S1_DEPTH; ++u) {
                    if (f + u < total) {
                        tt = mfma16(cl[u], cy[u], tt);
                        if (++cks == k1) {                              // a tile is complete (rows past R: zeros)
                            double *const To = T1s + cq * HD_PITCH + kq * 16 + x16;
#pragma unroll
                            for (int rr = 0; rr < 4; ++rr) To[64 * rr] = tt[rr];
                            tt = v4d{0.0, 0.0, 0.0, 0.0};
                            cks = 0; cq += 4;
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < HD_S1_DEPTH; ++u) { cl[u] = nl[u]; cy[u] = ny[u]; }
            }
        }
        lds_barrier();
        // ---- stage 2: the wave's four l against every beta' tile
        const double *const Tf = T1s + kq * HD_PITCH + wave * 64 + x16;
        for (int ks = 0; ks < nkb; ++ks) {
#pragma unroll
            for (int ct = 0; ct < HD_COL_TILES; ++ct) mn[ct] = 0.0;
            if (ks + 1 < nkb) rows_of(mn);
            double tf[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) tf[u] = LDS_UNPAIRED(Tf[4 * ks * HD_PITCH + 16 * u]);
#pragma unroll
            for (int ct = 0; ct < HD_COL_TILES; ++ct) {
                if (c0 + ct * 16 < R1) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[u][ct] = mfma16(mv[ct], tf[u], acc[u][ct]);
                }
            }
#pragma unroll
            for (int ct = 0; ct < HD_COL_TILES; ++ct) mv[ct] = mn[ct];
        }
        lds_barrier();
    }
    // ---- W: register rr of a lane is beta' = c0 + 16 ct + (lane >> 4) + 4 rr at a' = a0 + (lane & 15)
    if (!aok) return;
    double *const Wp = g.W + (int64_t)i * g.w_cols + g.w_off + a0 + x16;
    const int64_t lrow = (int64_t)g.n * g.w_cols;
#pragma unroll
    for (int ct = 0; ct < HD_COL_TILES; ++ct)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int col = c0 + ct * 16 + kq + 4 * rr;
            if (col < R1) {
                double *const Wc = Wp + (int64_t)col * r1;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int lr = l0 + wave * 4 + u;
                    if (lr < l) Wc[lr * lrow] = acc[u][ct][rr];
                }
            }
        }
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
