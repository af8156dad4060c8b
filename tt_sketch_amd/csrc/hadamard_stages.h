// The stages that hadamard_apply_kernel and hadamard_close_kernel share, each defined once.  Both contract a chain operand
// A, rows (kappa, c) `arow` elements apart and columns m, with two cores B (c, i, n) and C (kappa, i, col) at one mode index i:
//   T1[kappa][m, n]              = sum_c A[(kappa k + c), m] B[c, i, n]             stage 1, into LDS
//   acc[m, col k1 + n]          += sum_kappa C[kappa, i, col] T1[kappa][m, n]       stage 2, in registers
// with extents kappa < K, col < K1, c < k, n < k1 (hadamard_apply.hip and hadamard_close.hip say what these are there).
//
// A workgroup of four waves holds a 16 x 16 tile of (m, n) and HD_COLS values of col from c0.  hd_mode walks kappa in chunks
// of HD_KC with the accumulators of its caller, so no K is too long (hadamard_plan.h).
//   stage 1   wave w forms the tiles w, w + 4, ... of the chunk with v_mfma_f64_16x16x4 over c: the A operand [m][k = c] is
//             A[(kappa k + c), m0 + lane & 15], 16 lanes one 128-byte run; the B operand [k = c][n] is B[c, i, n0 + lane & 15],
//             the same for every kappa (it stays in cache).  Register r of lane (row (lane >> 4) + 4 r, column lane & 15)
//             goes to T1s[kappa of the chunk][m][n].  The wave's tiles are one stream of fragments with HD_S1_DEPTH loads
//             of each operand in flight across the tile boundaries, so the load latency is paid once per chunk and not
//             once per tile.  Rows past K inside the last k-block of four are written as zeros, rows beyond it neither
//             formed nor read.
//   stage 2   wave w owns m = 4 w .. 4 w + 3 of the tile and all col tiles: acc[col][n] += C^T[col][kk] T1s[kk][m][n], the A
//             operand [col][k = kk] from C through L2 (contiguous over col in the stored orientation), the B operand
//             [k = kk][n] from LDS at the conflict-free pitch.  One A fragment serves four matrix instructions, one B
//             fragment up to HD_COL_TILES of them; the C fragments of the next k-block are in flight under this one's, the
//             first k-block's under stage 1.  n sits on the accumulator's lane column, so 16 lanes store one 128-byte run.
// The k-block loops step pointers (A and B by four c, C by four kappa); a 64-bit product is formed once per tile or chunk.
// Operands beyond an extent are zeros selected after a load from a valid address: a lane past an extent reads the last
// column, a fragment past the stream's end the base of its operand.  One workgroup forms each element in a fixed order
// (kappa ascending within i, c ascending within kappa), no atomics: the same bits on every call.
//
// op_close_kernel (op_close.hip) runs the same stages with A = Wl, B = an operator core whose inner index is the pair
// (gamma, i), C = a train core, looping over the operator's in-index.
//
// The functions are inlined into three kernels at 237, 241 and 239 VGPRs, two workgroups per CU.  The stage-2 fragments of C are
// held as one 4-vector: written as four doubles the compiler made that vector in the kernels' own bodies and not in
// these functions, and the k-block loop of stage 2 came out four waits longer ("Hadamard stages").
#pragma once
#include "common.h"
#include "hadamard_plan.h"

namespace ttsk {

constexpr int HD_S1_DEPTH = 8;           // fragments of stage 1 in flight

// what a lane is in its workgroup: mok, nok say whether its column lane & 15 of the (m, n) tile lies inside the extents
struct HdLane {
    int wave, kq, x16;                   // wave of the four (uniform), lane >> 4, lane & 15
    bool mok, nok;
};

typedef v4d HdAcc[4][HD_COL_TILES];      // [u][ct][rr]: m = 4 wave + u, col = c0 + 16 ct + (lane >> 4) + 4 rr, n = lane & 15

__device__ __forceinline__ void hd_zero(HdAcc &acc)
{
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int ct = 0; ct < HD_COL_TILES; ++ct) acc[u][ct] = v4d{0.0, 0.0, 0.0, 0.0};
}

// this lane's columns col of C, in elements, clamped to the last column
__device__ __forceinline__ void hd_coff(int64_t (&coff)[HD_COL_TILES], int c0, int x16, int K1, int64_t stride)
{
#pragma unroll
    for (int ct = 0; ct < HD_COL_TILES; ++ct) {
        const int col = c0 + ct * 16 + x16;
        coff[ct] = (int64_t)(col < K1 ? col : K1 - 1) * stride;
    }
}

// One mode index: both stages over every chunk of kappa.  Ap, Bp are this lane's column of A and of B at mode i and
// c = 0, Cp is C at mode i; arow the row stride of A, sB0 that of B over c, sC0 that of C over kappa.
__device__ __forceinline__ void hd_mode(HdAcc &acc, double *const T1s, const double *const Ap, const double *const Bp,
                                        const double *const Cp, const int64_t arow, const int64_t sB0, const int64_t sC0,
                                        const int64_t (&coff)[HD_COL_TILES], const int K, const int K1, const int k, const int c0,
                                        const HdLane &ln)
{
    const int wave = ln.wave, kq = ln.kq, x16 = ln.x16;
    const int kb1 = (k + 3) >> 2;                                       // k-blocks of a stage-1 tile
    const int64_t astep = 4 * arow, bstep = 4 * sB0, cstep = 4 * sC0;
    const int nch = (K + HD_KC - 1) / HD_KC;
    for (int ch = 0; ch < nch; ++ch) {
        const int kap0 = ch * HD_KC;
        const int rows = K - kap0 < HD_KC ? K - kap0 : HD_KC;           // kappa of this chunk
        const int nkb = (rows + 3) >> 2;                                // its k-blocks of stage 2
        // the C fragments of this lane's next kappa; the first k-block's are in flight under stage 1
        const double *cr = Cp + (int64_t)(kap0 + kq) * sC0;
        int kap = kap0 + kq;
        auto rows_of = [&](v4d &dst) {
            const bool rowok = kap < K;
            const double *const p = rowok ? cr : Cp;
#pragma unroll
            for (int ct = 0; ct < HD_COL_TILES; ++ct) {
                double v = 0.0;
                if (c0 + ct * 16 < K1) v = p[coff[ct]];
                dst[ct] = rowok && c0 + ct * 16 + x16 < K1 ? v : 0.0;
            }
            cr += cstep; kap += 4;
        };
        static_assert(HD_COL_TILES == 4, "the fragments of the column tiles are held as one v4d");
        v4d mv, mn;                                                     // [ct]: this k-block's and the next one's
        rows_of(mv);
        // ---- stage 1: T1 of the chunk's rows into LDS, the wave's tiles q = wave, wave + 4, ... (nkb of them, kb1 fragments
        // each) as one stream of fragments
        {
            const int total = nkb * kb1;
            int lq = wave, lks = 0, lc = kq;                            // the loader: tile, k-block, this lane's c
            const double *pa = Ap + ((int64_t)(kap0 + lq) * k + kq) * arow, *pb = Bp + (int64_t)kq * sB0;
            auto frag = [&](double &av, double &bv) {
                const bool ok = lq < rows && lc < k;                    // past the stream's end lq >= rows: nothing is read
                const double x = *(ok ? pa : Ap), y = *(ok ? pb : Bp);
                av = ok && ln.mok ? x : 0.0;
                bv = ok && ln.nok ? y : 0.0;
                pa += astep; pb += bstep; lc += 4;
                if (++lks == kb1) {
                    lks = 0; lq += 4; lc = kq;
                    pa = Ap + ((int64_t)(kap0 + lq) * k + kq) * arow;
                    pb = Bp + (int64_t)kq * sB0;
                }
            };
            double ca[HD_S1_DEPTH], cb[HD_S1_DEPTH], na[HD_S1_DEPTH], nb[HD_S1_DEPTH];
#pragma unroll
            for (int u = 0; u < HD_S1_DEPTH; ++u) frag(ca[u], cb[u]);
            v4d tt = v4d{0.0, 0.0, 0.0, 0.0};
            int cq = wave, cks = 0;                                     // the consumer: tile, k-block
            for (int f = 0; f < total; f += HD_S1_DEPTH) {
#pragma unroll
                for (int u = 0; u < HD_S1_DEPTH; ++u) frag(na[u], nb[u]);
#pragma unroll
                for (int u = 0; u < HD_S1_DEPTH; ++u) {
                    if (f + u < total) {
                        tt = mfma16(ca[u], cb[u], tt);
                        if (++cks == kb1) {                             // a tile is complete (rows past K: zeros)
                            double *const To = T1s + cq * HD_PITCH + kq * 16 + x16;
#pragma unroll
                            for (int rr = 0; rr < 4; ++rr) To[64 * rr] = tt[rr];
                            tt = v4d{0.0, 0.0, 0.0, 0.0};
                            cks = 0; cq += 4;
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < HD_S1_DEPTH; ++u) { ca[u] = na[u]; cb[u] = nb[u]; }
            }
        }
        lds_barrier();
        // ---- stage 2: the wave's four m against every col tile
        const double *const Tf = T1s + kq * HD_PITCH + wave * 64 + x16;
        for (int ks = 0; ks < nkb; ++ks) {
            mn = v4d{0.0, 0.0, 0.0, 0.0};
            if (ks + 1 < nkb) rows_of(mn);
            double tf[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) tf[u] = LDS_UNPAIRED(Tf[4 * ks * HD_PITCH + 16 * u]);
#pragma unroll
            for (int ct = 0; ct < HD_COL_TILES; ++ct) {
                if (c0 + ct * 16 < K1) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc[u][ct] = mfma16(mv[ct], tf[u], acc[u][ct]);
                }
            }
            mv = mn;
        }
        lds_barrier();
    }
}

// The accumulators to out[m, col k1 + n], rows `orow` apart: Op is the element (m = 0, col = 0, this lane's n); the wave's
// rows are m0 + 4 wave + u, those below M are stored.
__device__ __forceinline__ void hd_store(const HdAcc &acc, double *const Op, const int64_t orow, const int k1, const int c0, const int K1,
                                         const int m0, const int M, const HdLane &ln)
{
    if (!ln.nok) return;
#pragma unroll
    for (int ct = 0; ct < HD_COL_TILES; ++ct)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            const int col = c0 + ct * 16 + ln.kq + 4 * rr;
            if (col < K1) {
                double *const Oc = Op + (int64_t)col * k1;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int mr = m0 + ln.wave * 4 + u;
                    if (mr < M) Oc[mr * orow] = acc[u][ct][rr];
                }
            }
        }
}

}  // namespace ttsk
