// The sketch of a CP tensor (factor matrices V_mu (n x N), CP rank N) with tensor-train DRMs as two GEMMs whose Khatri-Rao
// operand is formed in registers (ttsk_cp_chain_step, ttsk_cp_psi_omega; reference tensor_train_drm.py:90-107 and
// cp_sketch.py:6-36 store an N x n x rank panel per product only to contract it away):
//   chain step   out[j, m]      = sum_{(a, k)} (L[j, a] V[k, j]) D[(a, k), m]        rows N, contracted rho n, columns rho'
//   Psi          psi[i, (k, m)] = sum_j L[j, i] (V[k, j] R[j, m])                    rows l, contracted N, columns n r
//   Omega        om[i, m]       = sum_j L[j, i] Ro[j, m]                              more columns of the Psi product, V == 1
// Both run on v_mfma_f64_16x16x4 (common.h: A lane holds [m = lane & 15][k = lane >> 4], B lane [k = lane >> 4][n = lane & 15]).
//
// cp_chain_kernel<RT>   workgroup of four waves, wave w carries RT 16-row tiles of j and every column tile of rho'.  D, the
//             one streamed operand, goes through LDS in chunks of CP_KC rows (a, k) shared by the waves: two stages, the
//             next chunk is loaded into registers before the matrix instructions of this one and written after them, one
//             barrier per chunk.  Rows of a stage lie CP_D_PITCH doubles apart (cp_pass_plan.h: the two rows of a half-wave's
//             read on 64 different banks).  The A fragment of a k-block is L[j, a] V[k, j] at the lane's (a, k) = divmod(4 kb
//             + lane >> 4, n): one product per row tile, its operands loaded a group of CP_A_AHEAD k-blocks ahead.  Per k-block a lane steps k by 4 mod n
//             and a by 4 / n with one compare for the wrap -- no division in the loop, one offset per operand (DESIGN
//             section 9: vector address arithmetic is not hidden behind fp64 matrix instructions).  Rows past N are clamped
//             loads whose results are not stored, (a, k) past rho n zeros on both operands, columns past rho' zeros in LDS.
// cp_psi_kernel         workgroup (column block of CP_PSI_COLS, chunk of CP_N_CHUNK terms of j), wave w owns CP_PSI_COL_TILES
//             column tiles and every row tile of l: its B fragment V[k, j] R[j, m] (the lane's (k, m) = divmod(column, r) is
//             fixed, found once) is one product per column tile and k-block and serves l / 16 matrix instructions.  Operands
//             come through L2 a group of CP_PSI_AHEAD k-blocks ahead, one pointer increment each.  With one chunk the workgroup writes psi and
//             omega itself; otherwise its partial goes to the workspace and cp_psi_reduce_kernel sums the chunks in
//             ascending order.  No atomics anywhere: the same bits on every call.
#include "common.h"
#include "prof.h"
#include "cp_pass_plan.h"

namespace ttsk {

namespace {

template <int RT>
__global__ __launch_bounds__(64 * CP_WAVES) void cp_chain_kernel(CpChainArgs g)
{
    extern __shared__ double cp_sm[];
    const int tid = threadIdx.x, lane = tid & 63, x16 = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = g.N, K = g.K, n = g.n, rho1 = g.rho1;
    const int64_t row0 = (int64_t)blockIdx.x * (16 * RT * CP_WAVES) + wave * (16 * RT);
    const bool active = row0 < N;                              // a wave past N still stages D and meets the barriers
    const int ctn = (rho1 + 15) >> 4;

    // this lane's rows of L and V, one per row tile
    const double *Lrow[RT], *Vrow[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int64_t j = row0 + rt * 16 + x16, jc = j < N ? j : N - 1;
        Lrow[rt] = g.L ? g.L + jc * g.ldl : nullptr;
        Vrow[rt] = g.V + jc * g.v_j;
    }
    // its (a, k) of the k-block at hand, kk = 4 kb + kq = a n + k
    int kk = kq, a = kq / n, k = kq - a * n;
    int64_t koff = (int64_t)k * g.v_k;
    const int q4 = g.q4, r4 = g.r4;
    const int64_t kstep = (int64_t)r4 * g.v_k, kwrap = (int64_t)n * g.v_k;
    // The operands of the A fragments of one k-block at (a, k), then on to the next k-block.  They are multiplied where the
    // matrix instruction takes them, a group of k-blocks later: a product formed here would wait for its loads here.
    auto frag = [&](double *ldst, double *vdst) {
        const bool ok = kk < K;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            double lv = 1.0, vv = 0.0;
            if (ok) {
                vv = Vrow[rt][koff];
                if (Lrow[rt]) lv = Lrow[rt][a];
            }
            ldst[rt] = lv;
            vdst[rt] = vv;
        }
        kk += 4; a += q4; k += r4; koff += kstep;
        if (k >= n) { k -= n; koff -= kwrap; ++a; }
    };

    // staging of D: thread (row pair, column) of a chunk, 16 rows each
    constexpr int ST = CP_KC * 16 * CP_COL_TILES / (64 * CP_WAVES);
    const int scol = tid & 127, srow = tid >> 7;
    const bool scol_ok = scol < rho1;
    const double *const Dcol = g.D + (scol_ok ? scol : 0);
    auto stage_load = [&](int c, double *st) {
#pragma unroll
        for (int i = 0; i < ST; ++i) {
            const int gk = c * CP_KC + 2 * i + srow;
            st[i] = scol_ok && gk < K ? Dcol[(int64_t)gk * rho1] : 0.0;
        }
    };
    auto stage_store = [&](int c, const double *st) {
        double *const dst = cp_sm + (c & 1) * (CP_KC * CP_D_PITCH) + srow * CP_D_PITCH + scol;
#pragma unroll
        for (int i = 0; i < ST; ++i) dst[2 * i * CP_D_PITCH] = st[i];
    };

    v4d acc[RT][CP_COL_TILES];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CP_COL_TILES; ++ct) acc[rt][ct] = v4d{0.0, 0.0, 0.0, 0.0};

    const int nch = (K + CP_KC - 1) / CP_KC;
    // A chunk is two groups of CP_A_AHEAD k-blocks.  The operands of one group are loaded while the matrix instructions of
    // the group before it run, into the buffer that group has left: a wave alone on its SIMD spends 64 cycles per matrix
    // instruction, one k-block of a narrow rho' is far shorter than a load from L2.
    static_assert(CP_KC / 4 == 2 * CP_A_AHEAD, "a chunk is two groups of k-blocks");
    double st[ST], la[2][CP_A_AHEAD][RT], va[2][CP_A_AHEAD][RT];
    auto load_group = [&](int b) {
#pragma unroll
        for (int u = 0; u < CP_A_AHEAD; ++u) frag(la[b][u], va[b][u]);
    };
    auto run_group = [&](int b, int kb0, int kbn, const double *Bs) {
#pragma unroll
        for (int u = 0; u < CP_A_AHEAD; ++u) {
            if (kb0 + u < kbn) {
                double bf[CP_COL_TILES], af[RT];
#pragma unroll
                for (int ct = 0; ct < CP_COL_TILES; ++ct)
                    if (ct < ctn) bf[ct] = LDS_UNPAIRED(Bs[4 * (kb0 + u) * CP_D_PITCH + 16 * ct]);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) af[rt] = la[b][u][rt] * va[b][u][rt];
#pragma unroll
                for (int ct = 0; ct < CP_COL_TILES; ++ct)
                    if (ct < ctn) {
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt) acc[rt][ct] = mfma16(af[rt], bf[ct], acc[rt][ct]);
                    }
            }
        }
    };
    stage_load(0, st);
    stage_store(0, st);
    if (active) load_group(0);
    __syncthreads();
    for (int c = 0; c < nch; ++c) {
        if (c + 1 < nch) stage_load(c + 1, st);
        if (active) {
            const int left = K - c * CP_KC, kbn = left >= CP_KC ? CP_KC / 4 : (left + 3) >> 2;
            const double *const Bs = cp_sm + (c & 1) * (CP_KC * CP_D_PITCH) + kq * CP_D_PITCH + x16;
            load_group(1);
            run_group(0, 0, kbn, Bs);
            load_group(0);                                     // the first group of the next chunk; zeros past rho n
            run_group(1, CP_A_AHEAD, kbn, Bs);
        }
        if (c + 1 < nch) stage_store(c + 1, st);
        __syncthreads();
    }
    if (!active) return;
    // register jj of a lane is row (lane >> 4) + 4 jj of the tile at column lane & 15: 16 lanes store one 128-byte run
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CP_COL_TILES; ++ct) {
            const int col = ct * 16 + x16;
            if (ct < ctn && col < rho1) {
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int64_t row = row0 + rt * 16 + kq + 4 * jj;
                    if (row < N) g.out[row * g.ldo + col] = acc[rt][ct][jj];
                }
            }
        }
}

__global__ __launch_bounds__(64 * CP_WAVES) void cp_psi_kernel(CpPsiArgs g)
{
    const int tid = threadIdx.x, lane = tid & 63, x16 = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cb = (int)(blockIdx.x % (unsigned)g.cblocks), ch = (int)(blockIdx.x / (unsigned)g.cblocks);
    const int N = g.N, l = g.l, r = g.r, r_om = g.r_om;
    const int64_t cols = g.cols, psi_cols = g.psi_cols;
    const int64_t cw = (int64_t)cb * CP_PSI_COLS + wave * (16 * CP_PSI_COL_TILES);        // the wave's first column
    if (cw >= cols) return;
    const int j0 = ch * CP_N_CHUNK, j1 = N - j0 > CP_N_CHUNK ? j0 + CP_N_CHUNK : N;
    const int rtn = (l + 15) >> 4;

    // B operand: the lane's columns (k, m), fixed over the reduction
    const double *Rp[CP_PSI_COL_TILES], *Vp[CP_PSI_COL_TILES];
    int64_t rstep[CP_PSI_COL_TILES];
    bool cok[CP_PSI_COL_TILES];
    int64_t j = j0 + kq;
#pragma unroll
    for (int ct = 0; ct < CP_PSI_COL_TILES; ++ct) {
        const int64_t col = cw + ct * 16 + x16;
        cok[ct] = col < cols;
        const int64_t cc = cok[ct] ? col : 0;
        if (cc < psi_cols) {
            const int64_t kc = cc / r, m = cc - kc * r;
            Vp[ct] = g.V + kc * g.v_k + j * g.v_j;
            Rp[ct] = g.R ? g.R + j * g.ldr + m : nullptr;
            rstep[ct] = 4 * g.ldr;
        } else {                                               // a column of Omega: V == 1, its own right operand
            Vp[ct] = nullptr;
            Rp[ct] = g.Ro ? g.Ro + j * g.ldro + (cc - psi_cols) : nullptr;
            rstep[ct] = 4 * g.ldro;
        }
    }
    // A operand: L[j, i] at i = 16 rt + (lane & 15)
    const double *Lp = g.L ? g.L + j * g.ldl : nullptr;
    const int64_t lstep = 4 * g.ldl, vstep = 4 * g.v_j;
    // The operands of the fragments of one k-block at row j, then on to the next k-block.  V and R are multiplied where the
    // matrix instruction takes them, a group of k-blocks later: a product formed here would wait for its loads here.
    auto frag = [&](double *adst, double *rdst, double *vdst) {
        const bool jok = j < j1;
#pragma unroll
        for (int rt = 0; rt < CP_PSI_ROW_TILES; ++rt)
            if (rt < rtn) {
                const int i = rt * 16 + x16;
                const bool ok = jok && i < l;
                double v = 0.0;
                if (ok) v = Lp ? Lp[i] : 1.0;
                adst[rt] = v;
            }
#pragma unroll
        for (int ct = 0; ct < CP_PSI_COL_TILES; ++ct) {
            double rv = 0.0, vv = 1.0;
            if (jok && cok[ct]) {
                rv = Rp[ct] ? *Rp[ct] : 1.0;
                if (Vp[ct]) vv = *Vp[ct];
            }
            rdst[ct] = rv;
            vdst[ct] = vv;
            if (Rp[ct]) Rp[ct] += rstep[ct];
            if (Vp[ct]) Vp[ct] += vstep;
        }
        if (Lp) Lp += lstep;
        j += 4;
    };

    v4d acc[CP_PSI_ROW_TILES][CP_PSI_COL_TILES];
#pragma unroll
    for (int rt = 0; rt < CP_PSI_ROW_TILES; ++rt)
#pragma unroll
        for (int ct = 0; ct < CP_PSI_COL_TILES; ++ct) acc[rt][ct] = v4d{0.0, 0.0, 0.0, 0.0};
    // Groups of CP_PSI_AHEAD k-blocks: the operands of one group are loaded while the matrix instructions of the group
    // before it run, into the buffer that group has left.
    double ab[2][CP_PSI_AHEAD][CP_PSI_ROW_TILES], rb[2][CP_PSI_AHEAD][CP_PSI_COL_TILES], vb[2][CP_PSI_AHEAD][CP_PSI_COL_TILES];
    auto load_group = [&](int b) {
#pragma unroll
        for (int u = 0; u < CP_PSI_AHEAD; ++u) frag(ab[b][u], rb[b][u], vb[b][u]);
    };
    auto run_group = [&](int b, int jb) {
#pragma unroll
        for (int u = 0; u < CP_PSI_AHEAD; ++u) {
            if (jb + 4 * u < j1) {
#pragma unroll
                for (int ct = 0; ct < CP_PSI_COL_TILES; ++ct)
                    if (cw + ct * 16 < cols) {
                        const double bf = rb[b][u][ct] * vb[b][u][ct];
#pragma unroll
                        for (int rt = 0; rt < CP_PSI_ROW_TILES; ++rt)
                            if (rt < rtn) acc[rt][ct] = mfma16(ab[b][u][rt], bf, acc[rt][ct]);
                    }
            }
        }
    };
    load_group(0);
    for (int jb = j0; jb < j1; jb += 8 * CP_PSI_AHEAD) {
        load_group(1);
        run_group(0, jb);
        load_group(0);                                         // zeros past the chunk
        run_group(1, jb + 4 * CP_PSI_AHEAD);
    }
    // register jj of a lane is row i = 16 rt + (lane >> 4) + 4 jj at the lane's column: 16 lanes store one 128-byte run
    const bool direct = g.chunks == 1;
    double *const part = direct ? nullptr : g.ws + (int64_t)ch * l * cols;
#pragma unroll
    for (int ct = 0; ct < CP_PSI_COL_TILES; ++ct) {
        if (!cok[ct]) continue;
        const int64_t col = cw + ct * 16 + x16;
        const bool om = col >= psi_cols;
#pragma unroll
        for (int rt = 0; rt < CP_PSI_ROW_TILES; ++rt)
            if (rt < rtn) {
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int i = rt * 16 + kq + 4 * jj;
                    if (i >= l) continue;
                    double *const dst = !direct ? part + (int64_t)i * cols + col
                                        : om    ? g.omega + (int64_t)i * r_om + (col - psi_cols)
                                                : g.psi + (int64_t)i * psi_cols + col;
                    *dst = acc[rt][ct][jj];
                }
            }
    }
}

// out element (i, column) = the chunks' partials, summed in ascending chunk order
__global__ __launch_bounds__(CP_REDUCE_THREADS) void cp_psi_reduce_kernel(CpPsiArgs g)
{
    const int64_t cols = g.cols, elems = (int64_t)g.l * cols;
    const int64_t e = (int64_t)blockIdx.x * CP_REDUCE_THREADS + threadIdx.x;
    if (e >= elems) return;
    double s = g.ws[e];
    for (int ch = 1; ch < g.chunks; ++ch) s += g.ws[(int64_t)ch * elems + e];
    const int64_t i = e / cols, col = e - i * cols;
    if (col < g.psi_cols) g.psi[i * g.psi_cols + col] = s;
    else g.omega[i * g.r_om + (col - g.psi_cols)] = s;
}

}  // namespace

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_cp_chain_step(const double *L, int64_t ldl, const double *V, int64_t v_k, int64_t v_j, const double *D, double *out, int64_t ldo,
                       int64_t N, int64_t rho, int64_t n, int64_t rho1, int stream)
{
    TTSK_STREAM(st, stream);
    CpChainPlan p;
    const int rc = cp_chain_plan(L, ldl, V, v_k, v_j, D, out, ldo, N, rho, n, rho1, &p);
    if (rc) { set_error("%s", p.msg); return rc; }
    ProfBracket prof(st, PROF_EVAL, p.flops, "cp_chain_kernel<%d>", p.row_tiles);
    if (p.row_tiles == 1) return launch(cp_chain_kernel<1>, dim3((unsigned)p.blocks), dim3(64 * CP_WAVES), p.lds, st, p.a);
    return launch(cp_chain_kernel<CP_ROW_TILES>, dim3((unsigned)p.blocks), dim3(64 * CP_WAVES), p.lds, st, p.a);
}

int ttsk_cp_psi_omega(const double *L, int64_t ldl, const double *R, int64_t ldr, const double *V, int64_t v_k, int64_t v_j, double *psi,
                      const double *R_om, int64_t ld_om, int64_t r_om, double *omega, int64_t N, int64_t l, int64_t n, int64_t r, int stream)
{
    TTSK_STREAM(st, stream);
    CpPsiPlan p;
    const int rc = cp_psi_plan(L, ldl, R, ldr, V, v_k, v_j, psi, R_om, ld_om, r_om, omega, N, l, n, r, &p);
    if (rc) { set_error("%s", p.msg); return rc; }
    if (p.ws_bytes) {
        p.a.ws = (double *)scratch(stream, SCRATCH_MISC, p.ws_bytes);
        if (!p.a.ws) return TTSK_ERR_HIP;
    }
    {
        ProfBracket prof(st, PROF_EVAL, p.flops, "cp_psi_kernel");
        const int lrc = launch(cp_psi_kernel, dim3((unsigned)p.blocks), dim3(64 * CP_WAVES), 0, st, p.a);
        if (lrc) return lrc;
    }
    if (!p.reduce_blocks) return TTSK_OK;
    ProfBracket prof(st, PROF_EVAL, (double)p.a.chunks * (double)p.a.l * (double)p.a.cols, "cp_psi_reduce_kernel");
    return launch(cp_psi_reduce_kernel, dim3((unsigned)p.reduce_blocks), dim3(CP_REDUCE_THREADS), 0, st, p.a);
}

}  // extern "C"
