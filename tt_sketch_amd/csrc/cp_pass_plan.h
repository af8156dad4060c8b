// What the two CP sketch kernels (cp_pass.hip) are launched with, decided on the host: the argument checks and the cover
// of ttsk_cp_chain_step and ttsk_cp_psi_omega, their kernel arguments, grids, LDS, the split of the reduction of the
// Psi / Omega product into chunks, its workspace and the flops and algorithmic bytes of a call.
//
// Plain C++: no HIP types, so that the plan is compiled and checked by the host compiler alone
// (tests/test_cp_pass_host.py) before any kernel reads it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "ttsk.h"
#include "plan_common.h"

namespace ttsk {

constexpr int CP_MAX_RANK = 128;                 // rho, rho', l, r of the cover
constexpr int64_t CP_MAX_BLOCKS = (1ll << 31) - 1;

// ---- chain step: out (N x rho') = A (N x rho n) D (rho n x rho'), A[j, (a, k)] = L[j, a] V[k, j] formed in registers
constexpr int CP_WAVES = 4;                      // waves of a workgroup, each with its own row tiles
constexpr int CP_ROW_TILES = 2;                  // 16-row tiles a wave carries where N is past one workgroup of single tiles
constexpr int CP_SMALL_N = 16 * CP_WAVES;        // up to here one tile per wave: one workgroup covers N
constexpr int CP_COL_TILES = CP_MAX_RANK / 16;   // every column of rho' sits in one workgroup
constexpr int CP_KC = 32;                        // rows (a, k) of D per LDS stage
constexpr int CP_A_AHEAD = 4;                    // k-blocks of a group: its A operands are loaded under the matrix instructions of the group before
// a staged row of D holds up to 128 columns; the two rows that a half-wave's 64-bit LDS read touches (lanes 0-15 row
// 4 kb + 0, lanes 16-31 row 4 kb + 1) lie CP_D_PITCH = 16 modulo 32 doubles apart: 2 x 32 dwords on 64 different banks
constexpr int CP_D_PITCH = 16 * CP_COL_TILES + 16;
constexpr size_t CP_CHAIN_LDS = (size_t)2 * CP_KC * CP_D_PITCH * 8;      // two stages: one read while the next is written

struct CpChainArgs {
    const double *L, *V, *D;     // L NULL: rho = 1, L == 1
    double *out;
    int64_t ldl, v_k, v_j, ldo;
    int N, rho, n, rho1;
    int K;                       // rho n, the contracted length
    int q4, r4;                  // 4 = q4 n + r4: the step of a lane's (a, k) from one k-block to the next
};

struct CpChainPlan {
    CpChainArgs a;
    int row_tiles;               // per wave: the kernel instantiation
    int rows_per_block;          // 16 row_tiles CP_WAVES
    int64_t blocks;
    size_t lds;
    double flops, bytes;         // 2 N rho n rho'; L, V, D read once and out written once
    char msg[200];               // why not, when the status is not TTSK_OK
};

inline int cp_chain_plan(const double *L, int64_t ldl, const double *V, int64_t v_k, int64_t v_j, const double *D, double *out, int64_t ldo,
                         int64_t N, int64_t rho, int64_t n, int64_t rho1, CpChainPlan *p)
{
    *p = CpChainPlan{};
    if (!V || !D || !out) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_chain_step: NULL argument");
    if (N < 1 || rho < 1 || n < 1 || rho1 < 1)
        PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_chain_step: N = %lld, rho = %lld, n = %lld, rho' = %lld must be positive", (long long)N, (long long)rho,
                  (long long)n, (long long)rho1);
    if (!L && rho != 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_chain_step: no L stands for rho = 1, not %lld", (long long)rho);
    if (L && ldl < rho) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_chain_step: leading dimension %lld of L below rho = %lld", (long long)ldl, (long long)rho);
    if (ldo < rho1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_chain_step: leading dimension %lld of out below rho' = %lld", (long long)ldo, (long long)rho1);
    // ---- the cover
    if (rho > CP_MAX_RANK || rho1 > CP_MAX_RANK)
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_cp_chain_step: rank %lld; up to %d is covered", (long long)(rho > CP_MAX_RANK ? rho : rho1), CP_MAX_RANK);
    if (N > PLAN_MAX_EXTENT || n > PLAN_MAX_EXTENT) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_cp_chain_step: N or n of 2^31 or more; below 2^31 is covered");
    // the kernel's 32-bit row counters of D run up to two stages past rho n
    if (rho * n > PLAN_MAX_EXTENT - 2 * CP_KC)
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_cp_chain_step: rho n = %lld; up to 2^31 - %d is covered", (long long)(rho * n), 2 * CP_KC + 1);
    CpChainArgs &a = p->a;
    a.L = L; a.V = V; a.D = D; a.out = out;
    a.ldl = L ? ldl : 0; a.v_k = v_k; a.v_j = v_j; a.ldo = ldo;
    a.N = (int)N; a.rho = (int)rho; a.n = (int)n; a.rho1 = (int)rho1;
    a.K = (int)(rho * n);
    a.q4 = (int)(4 / n); a.r4 = (int)(4 % n);
    p->row_tiles = N > CP_SMALL_N ? CP_ROW_TILES : 1;
    p->rows_per_block = 16 * p->row_tiles * CP_WAVES;
    p->blocks = (N + p->rows_per_block - 1) / p->rows_per_block;
    p->lds = CP_CHAIN_LDS;
    p->flops = 2.0 * (double)N * (double)a.K * (double)rho1;
    p->bytes = 8.0 * ((double)N * (L ? rho : 0) + (double)N * n + (double)a.K * rho1 + (double)N * rho1);
    return TTSK_OK;
}

// ---- Psi / Omega: out (l x cols) = L^T (l x N) B (N x cols); the columns are (k, m) of Psi, B[j, (k, m)] = V[k, j] R[j, m],
// then the columns of Omega, B[j, m] = Ro[j, m]: in a sketch Psi_mu and Omega_{mu-1} share L_{mu-1}, but Omega pairs it with the
// right contraction of its own bond, so its right operand is an argument of its own (NULL: R itself)
constexpr int CP_PSI_COL_TILES = 2;                           // 16-column tiles per wave: its B fragments serve every row tile
constexpr int CP_PSI_COLS = 16 * CP_PSI_COL_TILES * CP_WAVES; // columns of a workgroup
constexpr int CP_PSI_ROW_TILES = CP_MAX_RANK / 16;
constexpr int CP_PSI_AHEAD = 2;                               // k-blocks of a group of the Psi kernel, as CP_A_AHEAD
constexpr int CP_N_CHUNK = 512;                               // terms of the reduction over N one workgroup sums

struct CpPsiArgs {
    const double *L, *R, *V;     // L NULL: l = 1, L == 1; R NULL: r = 1, R == 1; V may be NULL when psi is
    const double *Ro;            // Omega's right operand (N x r_om); NULL: r_om = 1, Ro == 1
    double *psi, *omega;         // either may be NULL
    double *ws;                  // (chunks, l, cols) partials when chunks > 1
    int64_t ldl, ldr, ldro, v_k, v_j;
    int64_t psi_cols, cols;      // n r (0 without psi), and with Omega's r_om behind them
    int N, l, r, r_om;
    int cblocks, chunks;
};

struct CpPsiPlan {
    CpPsiArgs a;
    int64_t blocks;              // cblocks chunks, the column block fastest
    int64_t reduce_blocks;       // of the closing launch that sums the chunks in ascending order; 0 when chunks = 1
    size_t ws_bytes;
    double flops, bytes;         // 2 l N cols; L, R, V read once, the outputs written once, the partials written and read
    char msg[200];
};

constexpr int CP_REDUCE_THREADS = 256;

// R_om NULL: Omega is formed with R (and r) itself, ld_om and r_om are not read
inline int cp_psi_plan(const double *L, int64_t ldl, const double *R, int64_t ldr, const double *V, int64_t v_k, int64_t v_j, double *psi,
                       const double *R_om, int64_t ld_om, int64_t r_om, double *omega, int64_t N, int64_t l, int64_t n, int64_t r, CpPsiPlan *p)
{
    *p = CpPsiPlan{};
    if (!psi && !omega) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_psi_omega: NULL output: neither psi nor omega");
    if (psi && !V) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_psi_omega: NULL factor matrix V");
    if (N < 1 || l < 1 || r < 1 || (psi && n < 1))
        PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_psi_omega: N = %lld, l = %lld, n = %lld, r = %lld must be positive", (long long)N, (long long)l,
                  (long long)n, (long long)r);
    if (!L && l != 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_psi_omega: no L stands for l = 1, not %lld", (long long)l);
    if (!R && r != 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_psi_omega: no R stands for r = 1, not %lld", (long long)r);
    if (L && ldl < l) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_psi_omega: leading dimension %lld of L below l = %lld", (long long)ldl, (long long)l);
    if (R && ldr < r) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_psi_omega: leading dimension %lld of R below r = %lld", (long long)ldr, (long long)r);
    if (!R_om) { R_om = R; ld_om = ldr; r_om = r; }
    if (!omega) r_om = 0;
    if (omega && (r_om < 1 || ld_om < r_om))
        PLAN_FAIL(TTSK_ERR_ARG, "ttsk_cp_psi_omega: Omega's right operand has r = %lld, leading dimension %lld", (long long)r_om, (long long)ld_om);
    // ---- the cover
    if (l > CP_MAX_RANK || r > CP_MAX_RANK || r_om > CP_MAX_RANK)
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_cp_psi_omega: rank %lld; up to %d is covered", (long long)(l > CP_MAX_RANK ? l : r > CP_MAX_RANK ? r : r_om),
                  CP_MAX_RANK);
    if (N > PLAN_MAX_EXTENT || (psi && n > PLAN_MAX_EXTENT)) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_cp_psi_omega: N or n of 2^31 or more; below 2^31 is covered");
    CpPsiArgs &a = p->a;
    a.L = L; a.R = R; a.V = V; a.Ro = omega ? R_om : nullptr; a.psi = psi; a.omega = omega;
    a.ldl = L ? ldl : 0; a.ldr = R ? ldr : 0; a.ldro = a.Ro ? ld_om : 0; a.v_k = v_k; a.v_j = v_j;
    a.psi_cols = psi ? n * r : 0;                                        // below 2^38
    a.cols = a.psi_cols + r_om;
    a.N = (int)N; a.l = (int)l; a.r = (int)r; a.r_om = (int)r_om;
    const int64_t cblocks = (a.cols + CP_PSI_COLS - 1) / CP_PSI_COLS;    // below 2^32
    const int64_t chunks = (N + CP_N_CHUNK - 1) / CP_N_CHUNK;            // below 2^22
    if (cblocks > CP_MAX_BLOCKS || cblocks * chunks > CP_MAX_BLOCKS)
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_cp_psi_omega: %lld column blocks x %lld chunks of N; up to 2^31 - 1 workgroups are covered",
                  (long long)cblocks, (long long)chunks);
    a.cblocks = (int)cblocks; a.chunks = (int)chunks;
    p->blocks = cblocks * chunks;
    const int64_t out_elems = l * a.cols;                                // below 2^46
    if (chunks > 1) {
        if (out_elems > (int64_t)(((size_t)-1 >> 1) / 8) / chunks)
            PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_cp_psi_omega: the partials of %lld chunks are not addressable", (long long)chunks);
        p->ws_bytes = (size_t)chunks * (size_t)out_elems * 8;
        p->reduce_blocks = (out_elems + CP_REDUCE_THREADS - 1) / CP_REDUCE_THREADS;
        if (p->reduce_blocks > CP_MAX_BLOCKS) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_cp_psi_omega: more than 2^31 workgroups in the closing sum");
    }
    p->flops = 2.0 * (double)l * (double)N * (double)a.cols;
    p->bytes = 8.0 * ((double)N * (L ? l : 0) + (double)N * (R && psi ? r : 0) + (double)N * (a.Ro && a.Ro != R ? r_om : 0) + (psi ? (double)N * n : 0.0) +
                      (double)out_elems) + 2.0 * (double)p->ws_bytes;
    return TTSK_OK;
}

}  // namespace ttsk
