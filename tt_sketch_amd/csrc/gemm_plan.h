// What the kernel families behind ttsk_gemm are launched with, decided on the host: the order of attempts (gemm_route) and,
// per family, the cover, the argument struct, the instantiation, the grid, the LDS, the scratch and the slab sum that follows
// (rows_longk_plan, skinny_r_plan, skinny_s_plan, small_gemm_plan, gemm_tile_plan, r_reduce_plan).  The launchers (gemm.hip,
// skinny.hip, small.hip, dense_right_pass.hip) add the scratch, the profiling bracket and the launch, nothing else.
//
// Plain C++: no HIP types, so that the plans are compiled and checked by the host compiler alone (tests/test_gemm_plan.py)
// before any kernel reads them.  Pointers are stored and their alignment is read; none is dereferenced.  A plan function
// returns 1 = covered (the plan is filled), 0 = not covered, < 0 = error (the reason in msg).  `slab` / `partial` of the
// argument structs stay null: the launcher allocates scratch_bytes / partial_bytes and fills them in.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "ttsk.h"
#include "plan_common.h"

#ifdef __HIPCC__
#define GEMM_HD __host__ __device__
#else
#define GEMM_HD
#endif

namespace ttsk {

// ---------------------------------------------------------------------------------------------------------------------------
// constants the plans share with the kernels

constexpr int BK = 32;        // K depth of one staged tile (gemm_kernel.h)
constexpr int LDKF = BK + 2;  // "k-fast" LDS layout tile[x][k], ld == 2 (mod 32)
GEMM_HD constexpr int ldmf(int bx) { return (bx % 32 == 16) ? bx : bx + 16; }  // "m-fast" ld == 16 (mod 32)

constexpr int SKR_KSPLIT_TILES = 12;  // skinny_r outputs of at most that many tiles: kappa split over the 8 waves instead of the tiles
constexpr int RP_BROWS = 48;          // rows of the B tile of rows_longk (N <= 48; rows beyond N repeat the last one, not stored)
// small_gemm_kernel: beyond a few MFLOP the tiled kernels win
constexpr int SG_MAX_K = 1024, SG_MAX_MN = 512;
constexpr double SG_MAX_FLOP = 48e6;
constexpr size_t GEMM_LDS_MAX = 160 * 1024;

// ---------------------------------------------------------------------------------------------------------------------------
// kernel arguments

// skinny_s_kernel (skinny.h): C[m, j] = sum_k W[k, m] S[j, k]
struct SkinnyS {
    const double *W[SK_MAXB], *S[SK_MAXB];
    double *C[SK_MAXB];
    int nb, wpp;        // problems, workgroups per problem: workgroup x serves problem x / wpp
    int64_t w_k, w_m;   // W[k][m]
    int64_t s_j, s_k;   // S[j][k]
    // Two-level streamed index j = u V + v (u < U at stride s_u, v < V at stride s_j; U = 1: plain).
    // A 16-row block is then a (16 >> tvl) (u) x (1 << tvl) (v) tile.  tvl = 4 (16 consecutive v of
    // one u: the right chain's GEMM1 reads X[p'', k, :] for 16 p'' of one k and writes whole 128-byte
    // lines of T[q][k][p'']) measured best; 4 x 4 and 2 x 8 tiles read longer runs but write
    // 32- / 64-byte pieces and were 5-10 % slower end to end.
    int64_t s_u;
    int U, V, nbv, tvl;
    int64_t c_m, c_j;   // C[m][j]
    int64_t c_u;        // two-level streamed index: C[m][u][v] at m c_m + u c_u + v c_j
    int64_t J;
    int P, K, groups;
    int64_t s_extent, w_extent, c_extent;   // elements addressable from each base (all < 2^29)
    double alpha;
    int accumulate;
    int big;            // 1: 64-bit origins per row block / k-block / output tile (operands beyond 4 GB)
    long long *stamps;   // diagnostics (TTSK_SK_STAMPS): s_memtime at phase boundaries, 8 per workgroup
};

// skinny_r_kernel (skinny.h): C[m, n] = sum_kappa A[kappa][m] B[kappa][n], kappa = (ko, ki)
struct SkinnyR {
    const double *A[SK_MAXB], *B[SK_MAXB];
    double *slab;       // [problem][chunk][m][n]
    int nb, chunks;     // workgroup x serves chunk x % chunks of (problem, row tile) x / chunks
    int64_t a_ko, a_ki, b_ko, b_ki;
    int64_t Ki, K, chunk;
    int64_t a_extent, b_extent;
    int M, N;           // rows of one row tile (<= 128), columns (<= 128)
    // A's row dimension may be longer than 128: m_tiles tiles of M rows, Mtot rows in all (the dense
    // unfoldings: 20 x K times K x 4096 ... ).  With a single-level kappa (`rebase`) every workgroup
    // addresses its operands from its own chunk / tile origin, so operands beyond 4 GB are fine.
    int m_tiles, rebase;
    int64_t Mtot;
    // An operand whose rows are not contiguous, or not pairable (odd extent / stride, unaligned base),
    // is "generic": plain 16-row tiles, one 8-byte load per tile and lane at row stride a_m / b_n,
    // each tile through its own descriptor (the rows of a k-contiguous unfolding are 128 MB apart).
    int a_gen, b_gen;
    int64_t a_m, b_n;
    long long *stamps;
};

// small_gemm_kernel (small.hip)
struct SmallG {
    const double *A[SK_MAXB], *B[SK_MAXB];
    double *C[SK_MAXB];
    int nb, M, N, K, tiles_m, tiles_n;   // tiles_n counts 32-column tiles
    int64_t a_m, a_k, b_k, b_n, c_m, c_n;
    int64_t a_extent, b_extent, c_extent;
    double alpha;
    int accumulate;
};

// rows_longk_kernel (dense_right_pass.hip)
struct RightPass {
    const double *S, *B;
    double *slab;                // [row block][K range][64][N]
    int64_t rows, s_row, b_row, K;
    int N, nrb, nkc;
};

// gemm_f64_kernel (gemm_kernel.h), one launcher per staging-layout pair in gemm_inst_*.hip
struct GemmLaunch {
    ttsk_gemm_desc d;
    const double *A, *B, *ks;
    double *C, *partial;
    int family, tiles;      // tiles: 1..4; family 0: 2x2 waves of 2x2 tiles; 1: 1x4 waves of tiles x 1; 2: 4x1 waves of 1 x tiles
    int splits, avec, bvec, fast_ok;
    int64_t kchunk;
    int bm, bn;
    int64_t a_extent, b_extent;   // elements from the (per-batch) operand base to its last element + 1
    unsigned gx, gy, gz;          // the grid: tiles along n, tiles along m, batch x splits
    size_t lds;
};

// where the sum of per-chunk partial results goes
struct ReduceOut { double *C[SK_MAXB]; };

// ---------------------------------------------------------------------------------------------------------------------------
// r_reduce_plan: out[m, n] (+)= alpha sum_c slab[c][m][n] for nprob x m_tiles (problem, row tile) blocks of slabs behind one
// another (skinny.hip launch_r_reduce: the long-K kernels, the fused chain step, the dense left pass)

struct RReduceArgs {
    int chunks, M, N, m_tiles, nprob;
    int64_t Mtot, c_m, c_n;
    double alpha;
    int accumulate;
    ReduceOut out;
};

enum { R_REDUCE_SCALAR = 0, R_REDUCE_PAIRED = 1, R_REDUCE_PAIRED_WIDE = 2 };

struct RReducePlan {
    int variant;         // scalar: skinny_r_reduce; paired / paired-wide: skinny_r_reduce2<16> / <64>, two consecutive n per lane
    unsigned gx, gy;
    int block;
};

inline RReducePlan r_reduce_plan(const double *slab, const RReduceArgs &r)
{
    const int64_t mn = (int64_t)r.M * r.N;
    // 16-byte loads and stores: N, c_m even, c_n = 1, 16-byte aligned bases
    bool vec = r.c_n == 1 && !(r.N & 1) && !(r.c_m & 1) && !((uintptr_t)slab & 15);
    for (int b = 0; b < r.nprob && vec; ++b) vec = !((uintptr_t)r.out.C[b] & 15);
    const unsigned gy = (unsigned)(r.nprob * r.m_tiles);
    // many chunks of one small result: 64 element pairs x 16 chunk groups per block
    if (vec && r.chunks >= 64 && gy * cdiv(mn / 2, 64) >= 64) return {R_REDUCE_PAIRED_WIDE, (unsigned)cdiv(mn / 2, 64), gy, 1024};
    if (vec) return {R_REDUCE_PAIRED, (unsigned)cdiv(mn / 2, 16), gy, 256};
    return {R_REDUCE_SCALAR, (unsigned)cdiv(mn, 16), gy, 256};
}

// ---------------------------------------------------------------------------------------------------------------------------
// gemm_collapse: a single contracted index moves into the inner slot; (ko, ki) that one stride walks become one index

inline ttsk_gemm_desc gemm_collapse(ttsk_gemm_desc n)
{
    if (n.Ki == 1) { n.Ki = n.Ko; n.Ko = 1; n.a_ki = n.a_ko; n.b_ki = n.b_ko; }
    else if (n.Ko > 1 && n.a_ko == n.Ki * n.a_ki && n.b_ko == n.Ki * n.b_ki) { n.Ki *= n.Ko; n.Ko = 1; }
    return n;
}

// ---------------------------------------------------------------------------------------------------------------------------
// rows_longk_plan: rows of an unfolding against a DRM matrix, both contiguous along a long contracted index (the right-hand
// products of a dense sketch with Gaussian matrices): rows_longk_kernel, then the slab sum

struct RowsLongkPlan {
    RightPass a;
    unsigned grid;
    int block;
    size_t lds, scratch_bytes;   // SCRATCH_GEMM: the slabs
    RReduceArgs red;
    const char *name;            // the profiling bracket
    double work;
    char msg[200];
};

// n: collapsed, batch == 1, c_n == 1
inline int rows_longk_plan(const ttsk_gemm_desc &n, const double *A, const double *B, double *C, int n_cu, RowsLongkPlan *p)
{
    *p = RowsLongkPlan{};
    if (!(n.Ko == 1 && n.a_ki == 1 && n.b_ki == 1 && n.N <= RP_BROWS && n.a_m >= n.Ki && n.b_n >= n.Ki)) return 0;
    const int64_t rows = n.M, s_row = n.a_m, b_row = n.b_n, K = n.Ki;
    const int N = (int)n.N;
    if (rows < 1 || N < 1 || N > RP_BROWS || K < 4096 || (K & 63) || (s_row & 1) || (b_row & 1) || s_row < K || b_row < K) return 0;
    if (((uintptr_t)A | (uintptr_t)B) & 15) return 0;
    const int64_t nrb = (rows + 63) / 64;
    // (kept as it was: the slab sum puts the row blocks on the grid's second dimension, so beyond 65535 of them -- 4.2 M rows --
    // its launch is refused with an error instead of the shape going to another kernel)
    if (nrb > (1 << 20)) return 0;
    // K ranges: enough workgroups for two per CU, at least 8 stages each
    const int64_t nst = K >> 6;
    int64_t nkc = (2 * n_cu + nrb - 1) / nrb;
    if (nkc > nst / 8) nkc = nst / 8;
    if (nkc < 1) nkc = 1;
    if (nrb * nkc >= (1ll << 30)) return 0;
    RightPass &a = p->a;
    a.S = A; a.B = B; a.rows = rows; a.s_row = s_row; a.b_row = b_row; a.K = K; a.N = N;
    a.nrb = (int)nrb; a.nkc = (int)nkc;
    p->grid = (unsigned)(nrb * nkc);
    p->block = 512;
    p->lds = (size_t)2 * (64 + RP_BROWS) * 64 * 8;
    p->scratch_bytes = (size_t)nrb * nkc * 64 * N * 8 + 64;
    p->red = RReduceArgs{(int)nkc, 64, N, (int)nrb, 1, rows, n.c_m, 1, n.alpha, n.accumulate, {}};
    p->red.out.C[0] = C;
    p->name = "rows_longk_kernel";
    p->work = 2.0 * rows * (double)N * K;
    return 1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// skinny_r_plan: long-K: one side <= 128, the other <= 128 or cut into row tiles of 128; both operands contiguous along their
// non-contracted index, 16-byte loads possible (even extents / strides, aligned bases); desc not collapsed (two-level kappa ok
// when the operands stay below 4 GB).  skinny_r_kernel<nmt, nnt, 4>, then the slab sum.

struct SkinnyRPlan {
    SkinnyR r;
    int swap;                    // the operand with more 16-row tiles plays "A": B does
    int a_pair, b_pair, gk;      // the descriptor's A / B pairable; generic tiles with kappa contiguous on both sides
    int nmt, nnt, nsub;          // 16-row tiles of a row tile, 16-column tiles, slabs per workgroup (8: one per wave)
    int unit;                    // which of skinny_r0..3.hip holds the instantiation
    int grid, block;             // grid = problems x row tiles x chunks
    size_t scratch_bytes;        // SCRATCH_GEMM: grid x nsub slabs of M x N
    RReduceArgs red;
    double work;                 // the bracket is "skinny_r_kernel<nmt, nnt, 4>"
    char msg[200];
};

inline int skinny_r_plan(const ttsk_gemm_desc &d, int nb, const double *const *A, const double *const *B, double *const *C, int n_cu,
                         SkinnyRPlan *p)
{
    *p = SkinnyRPlan{};
    if (nb < 1 || nb > SK_MAXB || d.batch != 1) return 0;
    const int64_t K = d.Ko * d.Ki;
    if ((d.M > 128 && d.N > 128) || K < 4096) return 0;
    if (d.Ko > 1 && d.Ki < 4) return 0;
    if (d.a_m < 0 || d.b_n < 0 || d.a_ko < 0 || d.a_ki < 0 || d.b_ko < 0 || d.b_ki < 0) return 0;
    // pairable = contiguous rows, even extent / strides, 16-byte aligned base; otherwise generic tiles
    bool a_pair = d.a_m == 1 && !((d.M | d.a_ko | d.a_ki) & 1), b_pair = d.b_n == 1 && !((d.N | d.b_ko | d.b_ki) & 1);
    for (int b = 0; b < nb; ++b) {
        if ((uintptr_t)A[b] & 15) a_pair = false;
        if ((uintptr_t)B[b] & 15) b_pair = false;
    }
    SkinnyR &r = p->r;
    r.nb = nb;
    const bool swap = cdiv(d.N, 16) > cdiv(d.M, 16);
    int64_t big, small_;
    if (!swap) {
        r.a_ko = d.a_ko; r.a_ki = d.a_ki; big = d.M; r.a_m = d.a_m; r.a_gen = !a_pair;
        r.b_ko = d.b_ko; r.b_ki = d.b_ki; small_ = d.N; r.b_n = d.b_n; r.b_gen = !b_pair;
    } else {
        r.a_ko = d.b_ko; r.a_ki = d.b_ki; big = d.N; r.a_m = d.b_n; r.a_gen = !b_pair;
        r.b_ko = d.a_ko; r.b_ki = d.a_ki; small_ = d.M; r.b_n = d.a_m; r.b_gen = !a_pair;
    }
    if (r.a_gen || r.b_gen) r.a_gen = r.b_gen = 1;     // one generic variant: both sides through plain tiles
    // ... or its 16-byte form when kappa is contiguous on both sides (single-level kappa, even strides / K,
    // 16-byte aligned bases)
    bool gk = r.a_gen && d.Ko == 1 && r.a_ki == 1 && r.b_ki == 1 && !(K & 1) && !(r.a_m & 1) && !(r.b_n & 1);
    for (int b = 0; b < nb && gk; ++b)
        if (((uintptr_t)A[b] | (uintptr_t)B[b]) & 15) gk = false;
    // a lane's row offset inside a tile (15 rows) has to fit 32 bits next to the kappa walk
    if (15 * r.a_m * 8 >= (1ll << 31) || 15 * r.b_n * 8 >= (1ll << 31)) return 0;
    r.Mtot = big;
    r.M = (int)(big < 128 ? big : 128);
    r.m_tiles = (int)cdiv(big, 128);
    r.N = (int)small_;
    if ((int64_t)nb * r.m_tiles > 60000) return 0;
    for (int b = 0; b < nb; ++b) {
        r.A[b] = swap ? B[b] : A[b];
        r.B[b] = swap ? A[b] : B[b];
    }
    if (d.Ko == 1) { r.a_ko = 0; r.b_ko = 0; }
    r.Ki = d.Ki;
    r.K = K;
    if (d.Ko > 1 && r.a_ko == d.Ki * r.a_ki && r.b_ko == d.Ki * r.b_ki) r.Ki = K;   // uniform walk
    r.rebase = r.Ki == K ? 1 : 0;
    if (gk && r.rebase) r.a_gen = r.b_gen = 2;
    r.a_extent = (big - 1) * r.a_m + (d.Ko - 1) * r.a_ko + (d.Ki - 1) * r.a_ki + 1;
    r.b_extent = (r.N - 1) * r.b_n + (d.Ko - 1) * r.b_ko + (d.Ki - 1) * r.b_ki + 1;
    // CUs one problem of the batch can count on (more problems than CUs: 1 here, all of them in skinny_s_plan -- as measured)
    const int cus = n_cu / nb > 0 ? n_cu / nb : 1;
    const int64_t want_chunks = cus / r.m_tiles > 0 ? cus / r.m_tiles : 1;
    r.chunk = cdiv(cdiv(K, want_chunks), 8) * 8;
    if (r.chunk < 64) r.chunk = 64;
    if (r.rebase) {
        // per-workgroup origins: 32-bit offsets only have to span one chunk and one row tile; shorter
        // chunks when a kappa row is so long (an unfolding with 2 MB rows) that a chunk would not fit
        auto span = [&](int64_t chunk) {
            const int64_t sa = ((r.a_gen ? 16 * r.a_m : 144) + (chunk + 64) * r.a_ki) * 8;
            const int64_t sb = ((r.b_gen ? 16 * r.b_n : 144) + (chunk + 64) * r.b_ki) * 8;
            return sa > sb ? sa : sb;
        };
        // (kept as it was: the last halving may take a chunk from under 128 to under 64, 104 -> 56; the kernel masks by the
        // chunk's length and takes any multiple of 8)
        while (span(r.chunk) >= (1ll << 32) - 64 && r.chunk > 64) r.chunk = cdiv(r.chunk / 2, 8) * 8;
        if (span(r.chunk) >= (1ll << 32) - 64) return 0;
    }
    const int chunks = (int)cdiv(K, r.chunk);
    r.chunks = chunks;
    if ((int64_t)nb * r.m_tiles * chunks > (1 << 30) / 8) return 0;
    if (!r.rebase) {
        // 32-bit byte offsets including the kappa walk past the end of the last chunk
        const int64_t reach_a = ((r.a_gen ? 16 * r.a_m : big + 144) + (d.Ko + 1) * r.a_ko + (d.Ki + 64) * r.a_ki) * 8;
        const int64_t reach_b = ((r.b_gen ? 16 * r.b_n : 144) + (d.Ko + 1) * r.b_ko + (d.Ki + 64) * r.b_ki) * 8;
        if (reach_a >= (1ll << 32) - 64 || reach_b >= (1ll << 32) - 64) return 0;
    }
    // (one slab per XCD filled with L2-local fp64 atomics was measured 3x slower than slab + reduce)
    const int nmt = (int)cdiv(r.M, 16), nnt = (int)cdiv(r.N, 16);
    const int nsub = nmt * nnt <= SKR_KSPLIT_TILES ? 8 : 1;      // small outputs: one slab per wave
    const int64_t nslab = (int64_t)nb * r.m_tiles * chunks;
    p->swap = swap; p->a_pair = a_pair; p->b_pair = b_pair; p->gk = gk;
    p->nmt = nmt; p->nnt = nnt; p->nsub = nsub;
    p->unit = nmt <= 4 ? 0 : nmt <= 6 ? 1 : nmt == 7 ? 2 : 3;
    p->grid = (int)nslab;
    p->block = 512;
    p->scratch_bytes = (size_t)nslab * nsub * r.M * r.N * 8 + 64;
    p->red = RReduceArgs{chunks * nsub, r.M, r.N, r.m_tiles, nb, r.Mtot, swap ? d.c_n : d.c_m, swap ? d.c_m : d.c_n, d.alpha,
                         d.accumulate, {}};
    for (int b = 0; b < nb; ++b) p->red.out.C[b] = C[b];
    // (a chunk -> XCD mapping that makes all problems of a batch fetch the shared operand into one L2
    // halved the L2-fabric traffic of the batched GEMM2 but not its time)
    p->work = 2.0 * nb * (double)d.M * (double)d.N * (double)K;
    return 1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// skinny_s_plan: streamed x small, K <= 128: skinny_s_kernel<npt, spt, dring, str>.  d: (ko, ki) already collapsed by the
// caller when uniform; nb pointer triples, d.batch the uniformly strided batch of each.

struct SkinnySPlan {
    SkinnyS s;
    int a_small;                 // the descriptor's A plays the small operand W (else B does)
    int npt, spt, dring, str;    // the instantiation: 16-column tiles of W, mode, ring depth, strips of the partial last tile
    int grid, block;
    size_t lds;
    double work;
    char msg[200];
};

inline int skinny_s_plan(const ttsk_gemm_desc &d, int nb, const double *const *A, const double *const *B, double *const *C, int n_cu,
                         SkinnySPlan *p)
{
    *p = SkinnySPlan{};
    if (nb < 1 || nb > SK_MAXB) return 0;
    if (d.Ko != 1) return 0;
    const int64_t K = d.Ki;
    if (K > 128 || K < 1) return 0;
    // which side streams?  A batch index joins the streamed index when the small operand is shared
    // by the batch and the output is contiguous across it (right chain GEMM1: b = k, n = p'').
    // (when both sides could play the small operand the smaller one does; a batched product whose larger side
    // is the shared one -- T[q,k,b,p''] of tt_fused.hip with few p'' -- still goes here, with that side small)
    const bool a_ok = d.M <= 128 && d.batch * d.N >= 2048 && (d.batch == 1 || (d.a_b == 0 && d.c_b >= 0));
    const bool b_ok = d.N <= 128 && d.batch * d.M >= 2048 && (d.batch == 1 || (d.b_b == 0 && d.c_b >= 0));
    const bool a_small = a_ok && (d.M <= d.N || !b_ok);
    const bool b_small = !a_small && b_ok;
    if (!a_small && !b_small) return 0;
    SkinnyS &s = p->s;
    s.nb = nb;
    for (int b = 0; b < nb; ++b) {
        s.W[b] = a_small ? A[b] : B[b];
        s.S[b] = a_small ? B[b] : A[b];
        s.C[b] = C[b];
    }
    if (a_small) {
        s.w_k = d.a_ki; s.w_m = d.a_m; s.P = (int)d.M;
        s.s_j = d.b_n; s.s_k = d.b_ki; s.s_u = d.b_b; s.V = (int)d.N;
        s.c_m = d.c_m; s.c_j = d.c_n;
    } else {
        s.w_k = d.b_ki; s.w_m = d.b_n; s.P = (int)d.N;
        s.s_j = d.a_m; s.s_k = d.a_ki; s.s_u = d.a_b; s.V = (int)d.M;
        s.c_m = d.c_n; s.c_j = d.c_m;
    }
    s.J = d.batch * (int64_t)s.V;
    s.U = (int)d.batch;
    if (d.batch == 1) s.s_u = 0;
    s.tvl = 4;
    s.nbv = (int)cdiv(s.V, 1 << s.tvl);
    if (s.s_j < 0 || s.s_k < 0 || s.s_u < 0 || s.w_k < 0 || s.w_m < 0 || s.c_m < 0 || s.c_j < 0) return 0;
    if (s.J >= (1ll << 31) - 256) return 0;
    s.K = (int)K;
    s.alpha = d.alpha;
    s.accumulate = d.accumulate;
    s.s_extent = (d.batch - 1) * s.s_u + ((int64_t)s.V - 1) * s.s_j + (K - 1) * s.s_k + 1;
    s.w_extent = (K - 1) * s.w_k + (s.P - 1) * s.w_m + 1;
    s.c_u = d.batch == 1 ? 0 : d.c_b;
    s.c_extent = (s.P - 1) * s.c_m + (d.batch - 1) * s.c_u + ((int64_t)(d.batch == 1 ? s.J : s.V) - 1) * s.c_j + 1;
    // per-lane 32-bit byte offsets only span one row block (16 rows, 4 k) and one output tile (16 x 16)
    const int64_t span_s = (16 * s.s_j + 4 * s.s_k) * 8, span_c = (16 * s.c_j + 16 * s.c_m) * 8;
    if (span_s >= (1ll << 32) - 64 || span_c >= (1ll << 32) - 64 || s.w_extent * 8 >= (1ll << 31)) return 0;
    // everything within reach of one descriptor + 32-bit offsets (incl. the last partial group and the
    // padded k-blocks)?  Otherwise the variant with 64-bit origins.
    const int64_t reach = ((d.batch + 4) * s.s_u + ((int64_t)s.V + 96) * s.s_j + (K + 24) * s.s_k) * 8;
    const int64_t reach_c = ((d.batch + 4) * s.c_u + ((int64_t)(d.batch == 1 ? s.J : s.V) + 96) * s.c_j + 144 * s.c_m) * 8;
    s.big = (reach >= (1ll << 32) - 64 || reach_c >= (1ll << 32) - 64) ? 1 : 0;
    const int npt = (int)cdiv(s.P, 16);
    if ((size_t)((cdiv(K, 4) + 4) * 4 * ldmf(16 * npt) + 16) * 8 + 2048 > GEMM_LDS_MAX) return 0;

    // ---- the launch: C[m, j] = alpha sum_k W[k, m] S[j, k]
    const int kb = (s.K + 3) / 4;
    const int64_t nrb = s.U == 1 ? cdiv(s.J, 16) : cdiv(s.U, 16 >> s.tvl) * cdiv(s.V, 1 << s.tvl);
    // CUs one problem of the batch can count on (more problems than CUs: all of them here, 1 in skinny_r_plan -- as measured)
    const int cus = n_cu / s.nb > 0 ? n_cu / s.nb : n_cu;
    // mode (see skinny_s_kernel): rounds of workgroups over the CUs x tile strips per SIMD and round.
    // Mode 2 loads no fragment twice and measured ~10 % faster at equal strip counts, so the others
    // have to beat it by more than that; ties between them go to the one without the shared block.
    const int64_t g4 = cdiv(nrb, 4), g5 = cdiv(nrb, 5), g8 = cdiv(nrb, 8);
    const int64_t t4 = cdiv(g4, cus) * npt, t5 = cdiv(g5, cus) * (npt + (npt > 4 ? 2 : 1)), t8 = cdiv(g8, cus) * 2 * npt;
    int spt = 2;
    int64_t best = t8;
    if (t4 * 112 < best * 100) { best = t4 * 112 / 100; spt = 0; }
    if (t5 * 112 < best * 100 && t5 < t4) { best = t5 * 112 / 100; spt = 1; }
    const int64_t groups = spt == 2 ? g8 : (spt == 1 ? g5 : g4);
    s.groups = (int)groups;
    const int ldw = ldmf(16 * npt);
    // ring depth 5 unless 4 pads K less (k-blocks are processed in multiples of the depth)
    // (a second, register-free prefetch level through `buffer_load ... lds`, a ring as deep as the
    // whole K and opposite k orders for the two waves of a SIMD were all measured slower)
    const int dring = cdiv(kb, 5) * 5 <= cdiv(kb, 4) * 4 ? 5 : 4;
    s.wpp = (int)(groups < cus ? groups : cus);
    // partial last tile of W with <= 8 valid columns: 4-wide strips instead of a padded 16x16x4 tile
    const int rem = (int)(s.P % 16);
    p->a_small = a_small;
    p->npt = npt; p->spt = spt; p->dring = dring;
    p->str = (rem > 0 && rem <= 8) ? (rem + 3) / 4 : 0;
    p->grid = s.wpp * s.nb;
    p->block = 512;
    p->lds = (size_t)cdiv(kb, dring) * dring * 4 * ldw * 8;
    p->work = 2.0 * nb * (double)d.batch * (double)d.M * (double)d.N * (double)K;
    return 1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// small_gemm_plan: a few MFLOP, pure latency: small_gemm_kernel, one wave per 16 x 32 output tile, K cut over ksplit waves.
// d: single contracted index (Ko == 1); nb pointer triples, or one triple with a uniformly strided d.batch

struct SmallGemmPlan {
    SmallG g;
    int ksplit;                  // waves of a workgroup that share K
    unsigned grid;
    int block;
    const char *name;
    double work;
    char msg[200];
};

// whether small_gemm_plan covers the shape: its answer depends on the descriptor and nb alone
inline bool small_batch_covers(const ttsk_gemm_desc &d, int nb)
{
    if (d.Ko != 1) return false;
    const int64_t K = d.Ki;
    int64_t count = nb;
    if (d.batch > 1) {
        if (nb != 1) return false;
        count = d.batch;
    }
    if (count < 1 || count > SK_MAXB) return false;
    if (K < 1 || K > SG_MAX_K || d.M > SG_MAX_MN || d.N > SG_MAX_MN) return false;
    if (2.0 * d.M * d.N * K > SG_MAX_FLOP) return false;
    if (d.a_m < 0 || d.a_ki < 0 || d.b_ki < 0 || d.b_n < 0 || d.c_m < 0 || d.c_n < 0) return false;
    if (d.batch > 1 && (d.a_b < 0 || d.b_b < 0 || d.c_b < 0)) return false;
    // elements from each operand's base to its last element + 1, within 32-bit byte offsets with the look-ahead of the ring
    const int64_t ea = (d.M - 1) * d.a_m + (d.Ki - 1) * d.a_ki + 1, eb = (d.N - 1) * d.b_n + (d.Ki - 1) * d.b_ki + 1;
    const int64_t ec = (d.M - 1) * d.c_m + (d.N - 1) * d.c_n + 1;
    return (ea + 64 * d.a_ki) * 8 < (1ll << 32) - 64 && (eb + 64 * d.b_ki) * 8 < (1ll << 32) - 64 && ec * 8 < (1ll << 32) - 64;
}

inline int small_gemm_plan(const ttsk_gemm_desc &d, int nb, const double *const *A, const double *const *B, double *const *C,
                           SmallGemmPlan *p)
{
    *p = SmallGemmPlan{};
    if (!small_batch_covers(d, nb)) return 0;
    const int64_t K = d.Ki, count = d.batch > 1 ? d.batch : nb;
    SmallG &g = p->g;
    g.nb = (int)count;
    for (int b = 0; b < count; ++b) {
        g.A[b] = d.batch > 1 ? A[0] + b * d.a_b : A[b];
        g.B[b] = d.batch > 1 ? B[0] + b * d.b_b : B[b];
        g.C[b] = d.batch > 1 ? C[0] + b * d.c_b : C[b];
    }
    g.M = (int)d.M; g.N = (int)d.N; g.K = (int)K;
    g.tiles_m = (int)cdiv(d.M, 16);
    g.tiles_n = (int)cdiv(d.N, 32);
    g.a_m = d.a_m; g.a_k = d.a_ki; g.b_k = d.b_ki; g.b_n = d.b_n; g.c_m = d.c_m; g.c_n = d.c_n;
    g.a_extent = (d.M - 1) * d.a_m + (d.Ki - 1) * d.a_ki + 1;
    g.b_extent = (d.N - 1) * d.b_n + (d.Ki - 1) * d.b_ki + 1;
    g.c_extent = (d.M - 1) * d.c_m + (d.N - 1) * d.c_n + 1;
    g.alpha = d.alpha;
    g.accumulate = d.accumulate;
    p->ksplit = K >= 512 ? 8 : (K >= 256 ? 4 : (K >= 128 ? 2 : 1));
    p->grid = (unsigned)(count * g.tiles_m * g.tiles_n);
    p->block = 64 * p->ksplit;
    p->name = "small_gemm_kernel";
    p->work = 2.0 * count * (double)d.M * (double)d.N * (double)K;
    return 1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// gemm_tile_plan: the generic tiles: gemm_f64_kernel<wm, wn, tm, tn, ak, bk>, then splitk_reduce_kernel when K is split

struct GemmTilePlan {
    GemmLaunch g;
    int wm, wn, tm, tn;          // waves along m, n, tiles per wave along m, n
    int ak, bk;                  // A / B staged "k-fast": the contracted index is the contiguous one
    int64_t tiles_m, tiles_n;    // 16 x 16 tiles the grid covers along m, n
    size_t partial_bytes;        // SCRATCH_GEMM: the split-K slabs; 0: one split, no reduce
    int rota;                    // the split-K reduce undoes the rotation of A (family 2) instead of B's
    unsigned red_grid;           // splitk_reduce_kernel, 256 threads
    double work;
    char msg[200];
};

inline int gemm_tile_plan(ttsk_gemm_desc d, const double *A, const double *B, double *C, const double *k_scale, GemmTilePlan *p)
{
    *p = GemmTilePlan{};
    const int64_t K = d.Ko * d.Ki;
    auto even = [](int64_t v) { return (v & 1) == 0; };
    // Tiles per wave in the skinny families are capped at 4: smaller workgroups leave room
    // for 3-4 of them per CU, and co-resident workgroups are what hides the load latency of these
    // short-K products (one wave per SIMD cannot overlap its own loads with its MFMAs).
    constexpr int cap = 4;
    auto split = [&](int64_t X) {            // tiles per wave so that rows*tiles covers ceil(X/16) evenly
        const int need = (int)cdiv(X, 16);
        const int rows = (int)cdiv(need, cap);
        return (int)cdiv(need, rows);
    };
    int family, tiles, bm, bn;
    if (d.M <= 128 && d.M <= d.N) { family = 1; tiles = split(d.M); bm = 16 * tiles; bn = 64; }
    else if (d.N <= 128) { family = 2; tiles = split(d.N); bm = 64; bn = 16 * tiles; }
    else { family = 0; tiles = 2; bm = 64; bn = 64; }
    const int64_t wg = d.batch * cdiv(d.M, bm) * cdiv(d.N, bn);
    int splits = d.split_k;
    if (splits <= 0) {
        splits = 1;
        if (wg < 192 && K >= 4 * BK) {
            int64_t want = cdiv(512, wg);
            int64_t maxs = cdiv(K, K >= 32 * BK ? 4 * BK : BK);
            splits = (int)(want < maxs ? want : maxs);
            if (splits > 1024) splits = 1024;
            if (splits < 1) splits = 1;
        }
    }
    // (the splits as asked for, before the chunk is rounded to whole tiles of K)
    if (!(d.batch * (int64_t)splits <= 65535))
        PLAN_FAIL(TTSK_ERR_ARG, "ttsk_gemm: batch*split_k too large (%lld)", (long long)(d.batch * splits));
    const int64_t kchunk = cdiv(cdiv(K, splits), BK) * BK;
    splits = (int)cdiv(K, kchunk);
    const int64_t tiles_m = cdiv(d.M, bm) * (bm / 16), tiles_n = cdiv(d.N, bn) * (bn / 16);
    p->partial_bytes = splits > 1 ? (size_t)(d.batch * splits * tiles_m * tiles_n * 256) * 8 + 64 : 0;
    // a single contracted index into the inner slot; the strides of the indices of extent 1 (ko, batch) zeroed
    auto k_inward_unit_strides_zeroed = [](ttsk_gemm_desc &n) {
        if (n.Ki == 1) { n.Ki = n.Ko; n.Ko = 1; n.a_ki = n.a_ko; n.b_ki = n.b_ko; }
        if (n.Ko == 1) { n.a_ko = 0; n.b_ko = 0; }
        if (n.batch == 1) { n.a_b = 0; n.b_b = 0; }
    };
    k_inward_unit_strides_zeroed(d);
    // which index is contiguous in memory decides the staging layout; 16-byte loads when the
    // contiguous index pairs up cleanly (even strides, pairs never straddle ko, aligned base)
    const bool ak = d.a_m != 1 && d.a_ki == 1;
    const bool bk = d.b_n != 1 && d.b_ki == 1;
    const bool k_pairs = d.Ko == 1 || even(d.Ki);
    int avec = ak ? (k_pairs && even(d.a_m) && even(d.a_ko) && even(d.a_b))
                  : (d.a_m == 1 && even(d.a_ki) && even(d.a_ko) && even(d.a_b));
    int bvec = bk ? (k_pairs && even(d.b_n) && even(d.b_ko) && even(d.b_b))
                  : (d.b_n == 1 && even(d.b_ki) && even(d.b_ko) && even(d.b_b));
    if (((uintptr_t)A & 15) != 0) avec = 0;
    if (((uintptr_t)B & 15) != 0) bvec = 0;
    // 16-byte loads additionally need whole pairs inside the extents
    if (ak ? (K & 1) : (d.M & 1)) avec = 0;
    if (bk ? (K & 1) : (d.N & 1)) bvec = 0;
    // The fast staging path addresses a tile through a buffer resource: 32-bit byte offsets from the
    // workgroup's first row / column, K offset in a scalar register.
    const int64_t a_extent = (d.M - 1) * d.a_m + (d.Ko - 1) * d.a_ko + (d.Ki - 1) * d.a_ki + 1;
    const int64_t b_extent = (d.N - 1) * d.b_n + (d.Ko - 1) * d.b_ko + (d.Ki - 1) * d.b_ki + 1;
    const int64_t span_a = (int64_t)bm * d.a_m + d.Ko * d.a_ko + (d.Ki + BK) * d.a_ki;
    const int64_t span_b = (int64_t)bn * d.b_n + d.Ko * d.b_ko + (d.Ki + BK) * d.b_ki;
    const int fast_ok = d.a_m >= 0 && d.b_n >= 0 && d.a_ki >= 0 && d.b_ki >= 0 && d.a_ko >= 0 && d.b_ko >= 0 &&
                        span_a * 8 < (1ll << 31) && span_b * 8 < (1ll << 31);
    p->g = GemmLaunch{d, A, B, k_scale, C, nullptr, family, tiles, splits, avec, bvec, fast_ok, kchunk, bm, bn, a_extent, b_extent,
                      (unsigned)cdiv(d.N, bn), (unsigned)cdiv(d.M, bm), (unsigned)(d.batch * splits),
                      8 * (size_t)((ak ? bm * LDKF : BK * ldmf(bm)) + (bk ? bn * LDKF : BK * ldmf(bn)))};
    p->wm = family == 0 ? 2 : (family == 1 ? 1 : 4); p->wn = family == 0 ? 2 : (family == 1 ? 4 : 1);
    p->tm = family == 0 ? 2 : (family == 1 ? tiles : 1); p->tn = family == 0 ? 2 : (family == 1 ? 1 : tiles);
    p->ak = ak; p->bk = bk;
    p->tiles_m = tiles_m; p->tiles_n = tiles_n;
    p->rota = family == 2 ? 1 : 0;
    const int64_t red_blocks = cdiv(d.batch * tiles_m * tiles_n * 256, 64);
    p->red_grid = (unsigned)(red_blocks > 4096 ? 4096 : red_blocks);
    p->work = 2.0 * (double)d.batch * (double)d.M * (double)d.N * (double)K;
    return 1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// gemm_route: the order of attempts of ttsk_gemm.  The plan of the family that takes the call is filled.

enum { GEMM_EMPTY = 0, GEMM_K0, GEMM_ROWS_LONGK, GEMM_SKINNY_R, GEMM_SKINNY_S, GEMM_SMALL, GEMM_LONGK_BATCH, GEMM_TILES };

struct GemmRoute {
    int kind;
    ttsk_gemm_desc n;            // what the plan was made from: d collapsed; LONGK_BATCH: one slice of the batch (batch 1, no batch strides)
    RowsLongkPlan rl;
    SkinnyRPlan sr;              // LONGK_BATCH: the first group of up to SK_MAXB slices
    SkinnySPlan ss;
    SmallGemmPlan sm;
    GemmTilePlan g;
    char msg[200];
};

// TTSK_OK and p->kind, or the error of a bad argument with its reason in p->msg
inline int gemm_route(const ttsk_gemm_desc &d, const double *A, const double *B, double *C, const double *k_scale, int n_cu, GemmRoute *p)
{
    p->kind = GEMM_EMPTY;
    p->msg[0] = 0;
    if (!(d.batch >= 0 && d.M >= 0 && d.N >= 0 && d.Ko >= 0 && d.Ki >= 0)) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_gemm: negative size");
    // every slice of a batch would write the same C (and the tiles of different slices would race): no caller means that
    if (!(d.batch <= 1 || d.c_b != 0)) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_gemm: batch %lld with c_b == 0", (long long)d.batch);
    if (d.batch == 0 || d.M == 0 || d.N == 0) return TTSK_OK;
    const int64_t K = d.Ko * d.Ki;
    if (K == 0) { p->kind = GEMM_K0; return TTSK_OK; }
    p->n = gemm_collapse(d);
    // both operands contiguous along a long contracted index: through LDS by LDS-DMA (dense_right_pass.hip)
    if (d.batch == 1 && !k_scale && d.c_n == 1 && rows_longk_plan(p->n, A, B, C, n_cu, &p->rl) == 1) { p->kind = GEMM_ROWS_LONGK; return TTSK_OK; }
    if (!k_scale) {
        // the chain shapes (tall-skinny, K <= 128, or long-K) have their own barrier-free kernels; then the small products
        if (skinny_r_plan(p->n, 1, &A, &B, &C, n_cu, &p->sr) == 1) { p->kind = GEMM_SKINNY_R; return TTSK_OK; }
        if (skinny_s_plan(p->n, 1, &A, &B, &C, n_cu, &p->ss) == 1) { p->kind = GEMM_SKINNY_S; return TTSK_OK; }
        if (small_gemm_plan(p->n, 1, &A, &B, &C, &p->sm) == 1) { p->kind = GEMM_SMALL; return TTSK_OK; }
    }
    if (d.batch >= 2 && K >= 32768 && !k_scale && d.c_b != 0) {
        // a long contraction batched over an index that only one operand carries (the per-slice right products of
        // dense_sketch.py: P^T X_b for every slice b of the tensor): up to SK_MAXB problems per launch of the long-K
        // chain kernel instead of the generic tiles (C2's Psi_0 pass: 2.76 -> 2.59 ms).  K is beyond skinny_s_plan's 128.
        p->n.batch = 1; p->n.a_b = p->n.b_b = p->n.c_b = 0;
        const int cnt = (int)(d.batch < SK_MAXB ? d.batch : SK_MAXB);
        const double *Ap[SK_MAXB], *Bp[SK_MAXB];
        double *Cp[SK_MAXB];
        for (int b = 0; b < cnt; ++b) { Ap[b] = A + b * d.a_b; Bp[b] = B + b * d.b_b; Cp[b] = C + b * d.c_b; }
        if (skinny_r_plan(p->n, cnt, Ap, Bp, Cp, n_cu, &p->sr) == 1) { p->kind = GEMM_LONGK_BATCH; return TTSK_OK; }
    }
    p->kind = GEMM_TILES;
    const int rc = gemm_tile_plan(d, A, B, C, k_scale, &p->g);
    if (rc < 0) { snprintf(p->msg, sizeof(p->msg), "%s", p->g.msg); return rc; }
    return TTSK_OK;
}

}  // namespace ttsk
