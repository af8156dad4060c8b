// The closing half of one mode of <x o y, u o v>, the inner product of two entrywise products of tensor trains, neither
// of which is formed (ttsk_hadamard_close).  With the chain so far carried through the cores of x and y by
// ttsk_hadamard_apply, Wl ((gamma c), i, p) for the ranks gamma of u, c of v and p = (beta' a') of x o y:
//   T1[i][gamma][p, c']     = sum_c Wl[(gamma s + c), i, p] V[c, i, c']              stage 1, into LDS
//   out[p, gamma' s' + c'] += sum_gamma U[gamma, i, gamma'] T1[i][gamma][p, c']      stage 2, in registers, over i as well
// This is hadamard_apply_kernel with two differences: the chain operand depends on the mode index (its row (gamma, c) of mode
// i starts at ((gamma s + c) n + i) P, rows n P apart), and the result is summed over i instead of indexed by it: the
// (P x S' s') x n array that a composition from ttsk_gemm calls writes only to add it up never exists.
//
// Workgroup (i chunk, p tile, c' tile, gamma' block) of four waves: a 16 x 16 tile of (p, c') and HD_COLS values of gamma'.
// For each i of its chunk it walks gamma in chunks of HD_KC; the accumulators stay in registers across both loops.
//   stage 1   wave w forms the tiles w, w + 4, ... of the gamma chunk with v_mfma_f64_16x16x4 over c: the A operand
//             [m = p][k = c] is Wl[(gamma s + c), i, p0 + lane & 15], 16 lanes one 128-byte run; the B operand [k = c][n = c'] is
//             V[c, i, c0 + lane & 15], the same for every gamma.  One stream of fragments with HD_S1_DEPTH loads of each
//             operand in flight across the tile boundaries; rows past S inside the last k-block are written as zeros.
//   stage 2   wave w owns p = 4 w .. 4 w + 3 of the tile and all gamma' tiles: acc[gamma'][c'] += U^T[gamma'][kk] T1s[kk][p][c'],
//             the A operand from U through L2, the B operand from LDS at the conflict-free pitch.
// The workgroup writes its tile of the partial sum over its i to work (ichunks, P, S' s'), c' on the accumulator's lane
// column: 16 lanes store one 128-byte run.  ttsk_sum_slices then adds the slices in ascending order into out.
// Operands beyond an extent are zeros selected after a load from a valid address.  One workgroup forms each element of a
// slice in a fixed order and the slices are added in a fixed order, no atomics: the same bits on every call.
#include "common.h"
#include "prof.h"
#include "hadamard_close_plan.h"

namespace ttsk {

namespace {

constexpr int HC_S1_DEPTH = 8;           // fragments of stage 1 in flight

__global__ __launch_bounds__(256, 2) void hadamard_close_kernel(HadamardCloseArgs g)
{
    extern __shared__ double hc_sm[];
    double *const T1s = hc_sm;
    const int tid = threadIdx.x, lane = tid & 63, x16 = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int b = (int)blockIdx.x;
    const int gb = b % g.gblocks;
    b /= g.gblocks;
    const int ct0 = b % g.ctiles;
    b /= g.ctiles;
    const int pt = b % g.ptiles, ic = b / g.ptiles;
    const int S = g.S, S1 = g.S1, s = g.s, s1 = g.s1, P = g.P;
    const int p0 = pt * 16, a0 = ct0 * 16, c0 = gb * HD_COLS;
    const int k1 = (s + 3) >> 2;
    const int i_begin = ic * g.iper, i_end = i_begin + g.iper < g.n ? i_begin + g.iper : g.n;

    // stage 1 operands: this lane's column of Wl (over p) and of V (over c'), at c = lane >> 4
    const bool pok = p0 + x16 < P, aok = a0 + x16 < s1;
    const int64_t nP = (int64_t)g.n * P;                                // one row (gamma, c) of Wl
    const double *const Wp = g.Wl + (pok ? p0 + x16 : P - 1);
    const double *const Vp = g.V + (int64_t)(aok ? a0 + x16 : s1 - 1) * g.sV[2];
    const int64_t wstep = 4 * nP, vstep = 4 * g.sV[0];
    // stage 2 operands: this lane's columns gamma' of U
    const int64_t ustep = 4 * g.sU[0];
    int64_t coff[HD_COL_TILES];
#pragma unroll
    for (int ct = 0; ct < HD_COL_TILES; ++ct) {
        const int col = c0 + ct * 16 + x16;
        coff[ct] = (int64_t)(col < S1 ? col : S1 - 1) * g.sU[2];
    }
    v4d acc[4][HD_COL_TILES];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int ct = 0; ct < HD_COL_TILES; ++ct) acc[u][ct] = v4d{0.0, 0.0, 0.0, 0.0};

    const int nch = (S + HD_KC - 1) / HD_KC;
    for (int i = i_begin; i < i_end; ++i) {
        const double *const Lp = Wp + (int64_t)i * P;                   // mode i of Wl, of V and of U
        const double *const Yp = Vp + (int64_t)i * g.sV[1];
        const double *const Xp = g.U + (int64_t)i * g.sU[1];
        for (int ch = 0; ch < nch; ++ch) {
            const int beta0 = ch * HD_KC;
            const int rows = S - beta0 < HD_KC ? S - beta0 : HD_KC;     // gamma of this chunk
            const int nkb = (rows + 3) >> 2;                            // its k-blocks of stage 2
            // the U fragments of this lane's next gamma; the first k-block's are in flight under stage 1
            const double *xr = Xp + (int64_t)(beta0 + kq) * g.sU[0];
            int beta = beta0 + kq;
            auto rows_of = [&](double *dst) {
                const bool rowok = beta < S;
                const double *const p = rowok ? xr : Xp;
#pragma unroll
                for (int ct = 0; ct < HD_COL_TILES; ++ct) {
                    double v = 0.0;
                    if (c0 + ct * 16 < S1) v = p[coff[ct]];
                    dst[ct] = rowok && c0 + ct * 16 + x16 < S1 ? v : 0.0;
                }
                xr += ustep; beta += 4;
            };
            double mv[HD_COL_TILES], mn[HD_COL_TILES];
            rows_of(mv);
            // ---- stage 1: T1 of the chunk's rows into LDS, the wave's tiles q = wave, wave + 4, ... as one stream of fragments
            {
                const int total = nkb * k1;
                int lq = wave, lks = 0, la = kq;                        // the loader: tile, k-block, this lane's c
                const double *pl = Lp + ((int64_t)(beta0 + lq) * s + kq) * nP, *py = Yp + (int64_t)kq * g.sV[0];
                auto frag = [&](double &lv, double &yv) {
                    const bool ok = lq < rows && la < s;                // past the stream's end lq >= rows: nothing is read
                    const double x = *(ok ? pl : Lp), y = *(ok ? py : Yp);
                    lv = ok && pok ? x : 0.0;
                    yv = ok && aok ? y : 0.0;
                    pl += wstep; py += vstep; la += 4;
                    if (++lks == k1) {
                        lks = 0; lq += 4; la = kq;
                        pl = Lp + ((int64_t)(beta0 + lq) * s + kq) * nP;
                        py = Yp + (int64_t)kq * g.sV[0];
                    }
                };
                double cl[HC_S1_DEPTH], cy[HC_S1_DEPTH], nl[HC_S1_DEPTH], ny[HC_S1_DEPTH];
#pragma unroll
                for (int u = 0; u < HC_S1_DEPTH; ++u) frag(cl[u], cy[u]);
                v4d tt = v4d{0.0, 0.0, 0.0, 0.0};
                int cq = wave, cks = 0;                                 // the consumer: tile, k-block
                for (int f = 0; f < total; f += HC_S1_DEPTH) {
#pragma unroll
                    for (int u = 0; u < HC_S1_DEPTH; ++u) frag(nl[u], ny[u]);
#pragma unroll
                    for (int u = 0; u < HC_S1_DEPTH; ++u) {
                        if (f + u < total) {
                            tt = mfma16(cl[u], cy[u], tt);
                            if (++cks == k1) {                          // a tile is complete (rows past S: zeros)
                                double *const To = T1s + cq * HD_PITCH + kq * 16 + x16;
#pragma unroll
                                for (int rr = 0; rr < 4; ++rr) To[64 * rr] = tt[rr];
                                tt = v4d{0.0, 0.0, 0.0, 0.0};
                                cks = 0; cq += 4;
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < HC_S1_DEPTH; ++u) { cl[u] = nl[u]; cy[u] = ny[u]; }
                }
            }
            lds_barrier();
            // ---- stage 2: the wave's four p against every gamma' tile
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
                    if (c0 + ct * 16 < S1) {
#pragma unroll
                        for (int u = 0; u < 4; ++u) acc[u][ct] = mfma16(mv[ct], tf[u], acc[u][ct]);
                    }
                }
#pragma unroll
                for (int ct = 0; ct < HD_COL_TILES; ++ct) mv[ct] = mn[ct];
            }
            lds_barrier();
        }
    }
    // ---- the slice of this i chunk: register rr of a lane is gamma' = c0 + 16 ct + (lane >> 4) + 4 rr at c' = a0 + (lane & 15)
    if (!aok) return;
    const int64_t cols = (int64_t)S1 * s1;
    double *const Op = g.work + (int64_t)ic * P * cols + a0 + x16;
#pragma unroll
    for (int ct = 0; ct < HD_COL_TILES; ++ct)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int col = c0 + ct * 16 + kq + 4 * rr;
            if (col < S1) {
                double *const Oc = Op + (int64_t)col * s1;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int pr = p0 + wave * 4 + u;
                    if (pr < P) Oc[pr * cols] = acc[u][ct][rr];
                }
            }
        }
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
