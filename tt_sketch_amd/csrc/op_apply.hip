// One sketch step of operator-times-train products that are never formed (ttsk_op_apply; MPO.__call__, reference
// tt_gmres.py:91-101, builds the (R r) x n x (R' r') product core only to have it sketched away).  Per term p of a sum, with
// operator core M (R, n_in, n_out, R'), train core C (r, n_in, r') and the chain so far L (R, r, l):
//   T1[beta, j][l, a']            = sum_a L[beta, a, l] C[a, j, a']                       stage 1, into LDS
//   W[l, i, w_off + beta' r' + a'] = sum_{beta, j} M[beta, j, i, beta'] T1[beta, j][l, a']   stage 2, in registers
// The chain step, Psi and Omega of the whole sum are then one ttsk_gemm each on W (l x n_out x sum_p R' r').
//
// Workgroup (term, l tile, a' tile, column block) of four waves: a 16 x 16 tile of (l, a') and OP_COLS columns (i, beta').  It
// walks the rows (beta, j) of the operator's (R n_in) x (n_out R') matrix in chunks of OP_KC with persistent accumulators, so
// no R n_in is too long (op_apply_plan.h).
//   stage 1   wave w forms the tiles w, w + 4, ... of the chunk with v_mfma_f64_16x16x4 over a: the A operand [m = l][k = a] is
//             L[beta][a][l0 + lane & 15], 16 lanes one 128-byte run; the B operand [k = a][n = a'] is C[a, j, a0 + lane & 15].
//             Register r of lane (row (lane >> 4) + 4 r, column lane & 15) goes to T1s[row of the chunk][l][a']: 64
//             consecutive doubles per register.
//   stage 2   wave w owns l = 4 w .. 4 w + 3 of the tile and all column tiles: out[(i beta')][a'] += M^T[(i beta')][kk] T1s[kk][l][a'],
//             the A operand [m = column][k = kk] from the operator through L2 (rows of the stored orientation are contiguous
//             over the columns), the B operand [k = kk][n = a'] from LDS -- the two rows a half-wave reads lie OP_PITCH =
//             16 modulo 32 doubles apart, 64 different banks.  One A fragment serves four matrix instructions, one B fragment
//             OP_COL_TILES of them.  a' sits on the accumulator's lane column, so 16 lanes store one 128-byte run of W.
// What is hoisted out of the k-block loops are the divisions: a lane's column offsets are fixed, and the row offsets of a chunk
// come from a table in LDS (one division per row and chunk).  Left inside, per k-block and lane: stage 2 reads its row offset
// from that table and adds it to eight column offsets (64-bit adds), stage 1 forms two 64-bit products for its operand
// addresses -- vector work that an fp64 matrix instruction does not hide.  Operands beyond an extent are zeros selected after a
// clamped load.  A term without operator runs the same stream with the identity selected in place of M, over the chunks
// its columns meet only.  Stage 1 is formed once per column block: r / OP_COLS of the work of stage 2 on top.
// One workgroup forms each element in a fixed order, no atomics: the same bits on every call.
#include "common.h"
#include "prof.h"
#include "op_apply_plan.h"

namespace ttsk {

namespace {

__global__ __launch_bounds__(256) void op_apply_kernel(OpApplyArgs g)
{
    extern __shared__ double op_sm[];
    double *const T1s = op_sm;
    int64_t *const moffs = (int64_t *)(op_sm + OP_KC * OP_PITCH);
    const int tid = threadIdx.x, lane = tid & 63, x16 = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int p = 0;
    while (p + 1 < g.K && (int)blockIdx.x >= g.t[p + 1].block0) ++p;
    const OpTerm &t = g.t[p];
    int b = (int)blockIdx.x - t.block0;
    const int cb = b % t.cblocks;
    b /= t.cblocks;
    const int at = b % t.atiles, lt = b / t.atiles;
    const int R1 = t.R1, r = t.r, r1 = t.r1, n_in = t.n_in, l = g.l;
    const int RK = t.R * n_in, NC = g.n_out * R1;
    const int l0 = lt * 16, a0 = at * 16, c0 = cb * OP_COLS;
    const int k1 = (r + 3) >> 2;
    const bool plain = t.plain != 0;

    // stage 1 operands: this lane's column of L (over l) and of C (over a')
    const bool lok = l0 + x16 < l, aok = a0 + x16 < r1;
    const double *const Lp = t.L + (lok ? l0 + x16 : l - 1);
    const double *const Cp = t.C + (int64_t)(aok ? a0 + x16 : r1 - 1) * t.sC[2];
    // stage 2 operands: this lane's columns (i, beta') of the operator
    const double *const Mp = t.M;
    int64_t coff[OP_COL_TILES];
    int colv[OP_COL_TILES];
#pragma unroll
    for (int ct = 0; ct < OP_COL_TILES; ++ct) {
        const int col = c0 + ct * 16 + x16;
        const int cc = col < NC ? col : NC - 1, i = cc / R1;
        coff[ct] = (int64_t)i * t.sM[2] + (int64_t)(cc - i * R1) * t.sM[3];
        colv[ct] = col < NC ? col : -1;
    }
    v4d acc[4][OP_COL_TILES];
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int ct = 0; ct < OP_COL_TILES; ++ct) acc[u][ct] = v4d{0.0, 0.0, 0.0, 0.0};

    const int nch = (RK + OP_KC - 1) / OP_KC;
    int ch0 = 0, ch1 = nch;
    if (plain) {                                      // the identity: only the rows that are columns of this block
        ch0 = c0 / OP_KC;
        const int e = (c0 + OP_COLS + OP_KC - 1) / OP_KC;
        ch1 = e < nch ? e : nch;
    }
    for (int ch = ch0; ch < ch1; ++ch) {
        // ---- stage 1: T1 of the chunk's rows into LDS
        if (tid < OP_KC) {
            const int kg = ch * OP_KC + tid, kc = kg < RK ? kg : RK - 1, beta = kc / n_in;
            moffs[tid] = (int64_t)beta * t.sM[0] + (int64_t)(kc - beta * n_in) * t.sM[1];
        }
        for (int q = wave; q < OP_KC; q += 4) {
            const int kg = ch * OP_KC + q;
            const bool rowok = kg < RK;
            const int kc = rowok ? kg : RK - 1, beta = kc / n_in, j = kc - beta * n_in;
            const double *const Lq = Lp + (int64_t)beta * r * l;
            const double *const Cq = Cp + (int64_t)j * t.sC[1];
            v4d tt = v4d{0.0, 0.0, 0.0, 0.0};
            // four k-blocks in flight under the four matrix instructions before them
            auto frag = [&](int ks, double &lv, double &cv) {
                const int a = 4 * (ks < k1 ? ks : k1 - 1) + kq;
                const bool ok = a < r;
                const int ac = ok ? a : r - 1;
                const double x = Lq[(int64_t)ac * l], y = Cq[(int64_t)ac * t.sC[0]];
                lv = ok && lok ? x : 0.0;
                cv = ok && aok && rowok ? y : 0.0;
            };
            double cl[4], cc[4], nl[4], nc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) frag(u, cl[u], cc[u]);
            for (int ks = 0; ks < k1; ks += 4) {
#pragma unroll
                for (int u = 0; u < 4; ++u) frag(ks + 4 + u, nl[u], nc[u]);
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (ks + u < k1) tt = mfma16(cl[u], cc[u], tt);
#pragma unroll
                for (int u = 0; u < 4; ++u) { cl[u] = nl[u]; cc[u] = nc[u]; }
            }
            double *const To = T1s + q * OP_PITCH + kq * 16 + x16;
#pragma unroll
            for (int rr = 0; rr < 4; ++rr) To[64 * rr] = tt[rr];
        }
        __syncthreads();
        // ---- stage 2: the wave's four l against every column tile
        const double *const Tf = T1s + kq * OP_PITCH + wave * 64 + x16;
        // the operator fragments of the next k-block in flight under this one's matrix instructions
        auto rows_of = [&](int ks, double *dst) {
            const double *const Mr = Mp + moffs[4 * ks + kq];
#pragma unroll
            for (int ct = 0; ct < OP_COL_TILES; ++ct) dst[ct] = c0 + ct * 16 < NC ? Mr[coff[ct]] : 0.0;
        };
        double mv[OP_COL_TILES], mn[OP_COL_TILES];
        rows_of(0, mv);
#pragma unroll
        for (int ks = 0; ks < OP_KC / 4; ++ks) {
            if (ks + 1 < OP_KC / 4) rows_of(ks + 1, mn);
            const int kg = ch * OP_KC + 4 * ks + kq;
            const bool rowok = kg < RK;
            double tf[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) tf[u] = LDS_UNPAIRED(Tf[4 * ks * OP_PITCH + 16 * u]);
#pragma unroll
            for (int ct = 0; ct < OP_COL_TILES; ++ct) {
                if (c0 + ct * 16 < NC) {
                    const double m = plain ? (kg == colv[ct] ? 1.0 : 0.0) : (rowok && colv[ct] >= 0 ? mv[ct] : 0.0);
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[u][ct] = mfma16(m, tf[u], acc[u][ct]);
                }
            }
#pragma unroll
            for (int ct = 0; ct < OP_COL_TILES; ++ct) mv[ct] = mn[ct];
        }
        __syncthreads();
    }
    // ---- W: register rr of a lane is column c0 + 16 ct + (lane >> 4) + 4 rr at a' = a0 + (lane & 15)
    if (!aok) return;
    double *const Wp = g.W + t.w_off + a0 + x16;
    const int64_t lrow = (int64_t)g.n_out * g.w_cols;
#pragma unroll
    for (int ct = 0; ct < OP_COL_TILES; ++ct)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int col = c0 + ct * 16 + kq + 4 * rr;
            if (col < NC) {
                const int i = col / R1;
                double *const Wc = Wp + (int64_t)i * g.w_cols + (int64_t)(col - i * R1) * r1;
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

int ttsk_op_apply(int K, const double *const *L, const double *const *M, const double *const *C, const int64_t *dims,
                  const int64_t *strides, int64_t l, double *W, int64_t w_cols, int stream)
{
    TTSK_STREAM(st, stream);
    OpPlan p;
    const int rc = op_apply_plan(K, L, M, C, dims, strides, l, W, w_cols, &p);
    if (rc) { set_error("%s", p.msg); return rc; }
    ProfBracket prof(st, PROF_EVAL, p.flops, "op_apply_kernel");
    return launch(op_apply_kernel, dim3((unsigned)p.blocks), dim3(256), OP_LDS, st, p.a);
}

}  // extern "C"
