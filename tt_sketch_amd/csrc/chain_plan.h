// What the three chain-step kernels (chain_fused.h, chain_wide.h, chain_sum.h) are launched with, decided on the host:
// the cover tests, the LDS plan, the wave tables, the grid rule, the proofs that every 32-bit byte offset fits, the slab
// of partial results and its closing reduce.  A plan holds the filled kernel-argument struct (all but `slab`, `Epk` and the
// lab-only `diag` / `stamps`), the instantiation the launcher picks and the launch figures; the launchers
// (chain_fused.hip, chain_wide.hip, chain_sum.hip) only carry it out.  What the three plans share -- the common refusals
// with the copy of the pointer tables, the common scalar fields, the launch figures -- is chain_plan_tables,
// chain_plan_scalars and chain_plan_launch; the E image all three kernels read is e_image_*.
//
// Plain C++: no HIP types, so that the plans are compiled and checked by the host compiler alone
// (tests/test_chain_plan.py, tests/test_chain_deal.py) before any kernel reads them.  Pointers are tested for alignment
// and NULL and copied, never dereferenced.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>
#include "chain_deal.h"
#include "plan_common.h"

namespace ttsk {

// ---- the calls ------------------------------------------------------------------------------------------------------
struct ChainStepArgs {
    int nb, n, K1, A, A2, J;
    const double *const *W;      // nb carried matrices (K1 x A), row stride w_c
    int64_t w_c;
    const double *const *X;      // nb cores
    int64_t x_j, x_k, x_c, x_extent;
    const double *E;             // (A, n, A2) contiguous
    double *const *T;            // nullptr, or nb buffers (A, n, J) contiguous
    double *const *Out;          // nb results (J x A2) contiguous
};

// T of the base arguments is ignored: the intermediate goes to Tint[b * t_b + (a * n + k) * t_ld + j] when Tint is given.
struct ChainSumArgs {
    ChainStepArgs s;
    double *Tint;
    int64_t t_b, t_ld, t_extent;
};

// ---- the kernel arguments -------------------------------------------------------------------------------------------
struct ChainStep {
    const double *W[SK_MAXB];
    const double *X[SK_MAXB];
    double *T[SK_MAXB];          // WT: T[a][k][j] (A x n x J contiguous)
    const double *E;
    const double *Epk;           // nullptr, or E packed (chain_pack.hip): slice k is the LDS image of E_k, eunits units; set by the launcher
    double *slab;                // [problem][workgroup of the problem][J][A2]
    int nb, wpp, n;              // problems, workgroups per problem, slices (mode size)
    int K1, A, A2, J;
    int64_t w_c;                 // row stride of W (elements); columns contiguous
    int64_t x_j, x_k, x_c;       // element strides of X
    int64_t x_extent, t_extent;  // elements addressable from the bases
    int AP, A2P;                 // padded extents of the two LDS images
    int ebase;                   // offset (doubles) of the E image in LDS
    int eunits;                  // 16-byte units of the E image the loader fills (multiple of 64)
    int xcd_map;                 // 1: workgroups of the same slice range share an XCD (E_k from one L2)
    unsigned int piece[CD_WAVES];// levelled workgroups (12 waves): wave w runs row tile | first Q << 8 | kind << 16 (chain_deal.h);
                                 // kind CD_NONE: a loader, its index among the nload loaders << 8
    int nload;
    int diag;                    // timing experiments (TTSK_CF_DIAG): 1 = no X loads, 2 = no E loads, 4 = no barriers (results are then wrong); 8 = one loader wave
    long long *stamps;           // diagnostics (TTSK_CF_STAMPS): s_memtime of workgroup 0, [slice][wave of CD_WAVES][8]
};

constexpr int CF_MAX_DMA = 160;  // loader instructions per slice (1 KB each)

// ---- the E image of chain_step_kernel --------------------------------------------------------------------------------
// One slice E_k[a][a'] (A x A2) sits in LDS pair-interleaved, in 16-byte units (two doubles): section sec holds rows
// 2 sec and 2 sec + 1, A2P units long; unit u of a section is columns (2 (u >> 1), + 1) of row 2 sec + (u & 1).  The 32
// lanes (kq in {0, 1}, x) of a phase-B fragment then read 32 consecutive doubles.  Defined here once, for the loader that
// gathers the image from E, for the kernel that packs it (chain_pack.hip) and for the host test of both
// (tests/test_chain_pack_host.py).  constexpr: the device code calls them as they stand.
struct EUnit { int row, col; };

// ceil(2^32 / A2P): U / A2P == (U * inv) >> 32 for U < 2^16
constexpr uint32_t e_image_inv(int A2P) { return (uint32_t)(((1ull << 32) + (uint32_t)A2P - 1) / (uint32_t)A2P); }

// Which two elements E[row][col], E[row][col + 1] unit U of the image holds.  Rows beyond A repeat row A - 1 (they meet
// exact zeros of T), a last unit whose second column would lie beyond A2 holds columns 0, 1 (never read).
constexpr EUnit e_image_unit(uint32_t U, uint32_t inv, int A, int A2, int A2P)
{
    const uint32_t sec = (uint32_t)(((uint64_t)U * inv) >> 32), u = U - sec * (uint32_t)A2P;
    int row = (int)(2 * sec + (u & 1));
    row = row < A ? row : A - 1;
    int col = (int)(2 * (u >> 1));
    col = col + 1 < A2 ? col : 0;
    return EUnit{row, col};
}

// The same for an image that begins at row a0 of E (a chunk of the DRM rank, chain_wide_kernel) and for odd A2, where rows
// are only 8-byte aligned: the unit behind the last column of a row then takes the first element of the next slice along
// (it meets an output column that is never stored) -- except in the last slice (`last`), where it would reach past the
// core: there it holds columns 0, 1 and column A2 - 1 is patched in afterwards, element by element.
constexpr EUnit e_image_unit_from(uint32_t U, uint32_t inv, int a0, int A, int A2, int A2P, bool last)
{
    const EUnit un = e_image_unit(U, inv, A - a0, A2 + (((A2 & 1) && !last) ? 1 : 0), A2P);
    return EUnit{a0 + un.row, un.col};
}

// The inverse view: the offset (doubles) of E[a][a2] in the image ...
constexpr int e_image_at(int a, int a2, int A2P) { return (a >> 1) * 2 * A2P + 4 * (a2 >> 1) + 2 * (a & 1) + (a2 & 1); }
// ... and phase B's fragment reads.  Lane (x16 = lane & 15, kq = lane >> 4) reads E[4 kap + kq][16 nn + x16] of k-block kap,
// column tile nn, at e_frag_lane + kap 4 A2P + 32 nn; of strip q behind NNF full tiles E[4 kap + kq][16 NNF + 4 q + (x16 & 3)]
// at e_strip_lane + e_image_at(0, 16 NNF + (x16 & 3)) + kap 4 A2P + 8 q.
constexpr int e_frag_lane(int x16, int kq, int A2P) { return (kq >> 1) * 2 * A2P + 4 * (x16 >> 1) + 2 * (kq & 1) + (x16 & 1); }
constexpr int e_strip_lane(int kq, int A2P) { return (kq >> 1) * 2 * A2P + 2 * (kq & 1); }

// A packed DRM core (chain_pack.hip): Epk[k][eunits] units, slice k the image of E_k byte for byte.  Its size in bytes --
// at rank 100 as large as the core itself: a packed DRM takes about twice the device memory.
constexpr int64_t e_pack_bytes(int n, int eunits) { return (int64_t)n * eunits * 16; }

struct ChainWide {
    const double *W[SK_MAXB];
    const double *X[SK_MAXB];
    double *T[SK_MAXB];          // WT: T[a][k][j] (A x n x J contiguous)
    const double *E;
    double *slab;                // [problem][unit = slice range x chunk][J][A2]
    int nb, wpp, nac, n;         // problems, slice ranges per problem, chunks of A, slices (mode size)
    int K1, A, A2, J;
    int64_t w_c;                 // row stride of W (elements); columns contiguous
    int64_t x_j, x_k, x_c;       // element strides of X
    int64_t x_extent, t_extent;  // elements addressable from the bases
    int ac;                      // columns of W / rows of E per chunk (<= 16 NQF + 4 STRQ)
    int A2P;                     // A2 rounded up to even: 16-byte units per section of the E image
    int ebase;                   // offset (doubles) of the E image in LDS
    int eunits;                  // 16-byte units of one E image (multiple of 64)
    int ebuf2;                   // 1: two E images (slice k in image k & 1)
    int xcd_map;                 // 1: workgroups of one (slice range, chunk) share an XCD (E_k from one L2)
    int loader;                  // the wave that only feeds E
    signed char tile0[8], tile1[8];   // row tiles of each wave, -1 = none
    // Few rows per tensor (J <= 64: the rank-20 terms of a sum): a workgroup serves `tpw` tensors at once -- one W image
    // each (`wimg` doubles apart), wave w works for tensor slot[w] of the group -- and they share every E_k it loads.
    int tpw, wimg;
    signed char slot[8];
};

// chunk structures that are instantiated: columns = 16 tiles + 4 strips
inline constexpr int CW_NQ[7] = {1, 1, 2, 2, 3, 3, 4}, CW_SQ[7] = {0, 2, 0, 2, 0, 2, 0};

constexpr int CS_NAMAX = 4;       // a-tiles of T a wave computes in phase A (W fragments in registers)
constexpr int CS_SRMAX = 6;       // row tiles of the strip column (one wave owns all of them)
constexpr int CS_NSMAX = 2;       // 4-wide strips behind the full column tiles
constexpr int CS_DMAMAX = 13;     // E loader instructions per wave and slice (1 KB each)

// the phase-B bodies chain_sum_kernel instantiates: rectangles (row tiles, column tiles) of full tiles, and the strip
// column as (row tiles, strips)
#define CS_RECT_BODIES(X) X(1, 1) X(1, 2) X(1, 3) X(2, 1) X(2, 2) X(2, 3) X(3, 1) X(3, 2) X(4, 1) X(5, 1)
#define CS_STRIP_BODIES(X) X(1, 1) X(2, 1) X(3, 1) X(4, 1) X(5, 1) X(6, 1) X(1, 2) X(2, 2) X(3, 2) X(4, 2) X(5, 2) X(6, 2)

struct ChainSumRole {
    unsigned char term, at0, na;  // phase A: local term, first a-tile, a-tiles (0 = none)
    unsigned char body;           // phase-B body: 16 * RT + CT for a rectangle of full tiles, 128 + 16 * SR + NS for the strip column
    unsigned char rt0, ct0;       // origin of the rectangle of full tiles
    unsigned char pad0, pad1;
};

// everything but the pointer tables: what a wave's body reads (no dynamically indexed member -- the kernel picks the
// wave's pointers and role from the tables itself, straight from the kernel-argument segment; handed to the body as one
// struct WITH the tables the compiler copies all of it to scratch)
struct ChainSumS {
    const double *E;
    double *T;                    // nullptr, or T[b * t_b + (a * n + k) * t_ld + j]
    double *slab;                 // [term][slice range][J][A2]
    int nb, n, K1, A, A2, J;
    int tpw, ngroups, nranges;
    int64_t w_c, x_j, x_k, x_c, x_extent;
    int64_t t_b, t_ld, t_extent;
    int RP;                       // row pitch of the T image (>= 16 row tiles; 2 mod 4: the stores of phase A then meet 2-way instead of 4-way bank conflicts)
    int KB2;                      // k-blocks of phase B = ceil(A / 4)
    int A2P;                      // row length of the E image (even, >= 16 NNF + 4 NS)
    int NNF, NS;                  // full column tiles of Out, 4-wide strips behind them
    int ebase, gbase;             // LDS offsets (doubles) of the E and G images; the T image sits at 0
    int eunits;                   // 16-byte units of the E image (multiple of 64)
    int xcd_map;                  // 1: the term groups of a slice range share an XCD (E_k from one L2)
    int c_fast;                   // G loader: 1 = c is the contiguous index of X (right chain), 0 = j
    // What the set-up would otherwise derive with divisions and 64-bit products: it runs once per workgroup, on a cold
    // instruction cache, with nothing else resident on the CU -- its length in INSTRUCTIONS is what it costs (1640 of
    // them took 13 k cycles of a 110 k-cycle launch).
    int kbase, krem;              // slice range rr = [rr kbase + min(rr, krem), + kbase + (rr < krem))
    int inv_ng;                   // (1 << 20) / ngroups + 1: i / ngroups == (i * inv_ng) >> 20 for i * ngroups < 2^20
    int wpt, per, gu;             // G loader: waves per term (8 / tpw), elements per wave, loads per lane and slice
    uint32_t w_c8, x_j8, x_c8;    // byte strides as 32-bit numbers (the host checks that every offset fits)
    uint32_t t_b8, t_a8;          // T: bytes per term, bytes per row a (n t_ld 8)
    uint32_t slab_t8, slab_r8;    // slab: bytes per term (nranges J A2 8) and per slice range (J A2 8)
    uint32_t e_inv;               // ceil(2^32 / A2P): unit U of the E image is in section (U e_inv) >> 32
#ifdef TTSK_LAB                    // timing experiments: only in a lab build (-DTTSK_LAB), never in the shipped code object
    long long *stamps;            // s_memtime of workgroup 0, [slice][wave][8]
    int diag;                     // (results wrong) 1 no E DMA, 2 no phase A, 4 no phase B, 8 no G loads, 16 no barriers, 32 no fragment reads in
                                  // phase B, 64 no priorities, 128 no small rectangles
#endif
};

struct ChainSum {
    ChainSumS s;
    const double *W[SK_MAXB];
    const double *X[SK_MAXB];
    ChainSumRole role[8];
};

// ---- the plans ------------------------------------------------------------------------------------------------------
// What every launcher does around its kernel: the slab of partial results (red_chunks of them per problem, J x A2 each:
// `slab` elements, requested as slab * 8 + 64 bytes), the closing reduce over them, the work of the profiling bracket.
struct ChainLaunch {
    size_t lds;                  // dynamic LDS bytes of a workgroup
    int grid;                    // workgroups
    int64_t slab;
    int red_chunks, red_m, red_n;
    double flops;                // BOTH products of the step (the pair the kernel replaces)
};

struct ChainFusedPlan {
    ChainStep a;
    int nq, sq;                  // tile structure of A (= that of A2): full tiles, strips
    bool wt;
    int ebuf, unr, waves;
    ChainLaunch l;
};

struct ChainWidePlan {
    ChainWide a;
    int ci;                      // chunk structure CW_NQ[ci], CW_SQ[ci]
    int nn, sn;                  // tile structure of A2
    bool wt;
    int unr;
    bool mt2;                    // the instantiation with two row tiles per wave
    ChainLaunch l;
};

struct ChainSumPlan {
    ChainSum ka;
    int na_run;                  // a-tiles per wave in phase A: <= 2 the NA = 2 instantiation, else NA = 4
    bool wt;
    ChainLaunch l;
};

// rank -> full 16-wide tiles + 4-wide strips (a remainder of 9..15 is a zero-padded full tile)
inline void chain_tile_split(int r, int &nf, int &str)
{
    const int rem = r % 16;
    nf = r / 16;
    if (rem == 0) str = 0;
    else if (rem <= 4) str = 1;
    else if (rem <= 8) str = 2;
    else { nf += 1; str = 0; }
}

// The E image of a DRM core of ranks (A, A2) as chain_fused_plan lays it out: row length A2P, and the 16-byte units of a
// slice padded to whole 64-unit (1 KB) loader pieces.  false: chain_step_kernel has no image for these ranks.
inline bool chain_e_image(int A, int A2, int &A2P, int &eunits)
{
    if (A < 4 || A2 < 4 || (A2 & 1)) return false;
    int nq, sq;
    chain_tile_split(A, nq, sq);
    A2P = A2;
    eunits = (int)cdiv((int64_t)2 * (nq * 4 + sq) * A2P, 64) * 64;     // 2 KB2 A2P units
    return eunits / 64 <= CF_MAX_DMA;
}

// k-blocks of phase A are issued in straight-line runs of 25 or of 5 and padded to whole runs (the padded ones
// meet zero rows of the W image): 25 when that pads at most one k-block more than 5 does
inline void chain_phase_a_runs(int K1, int &unr, int &KB1)
{
    const int kb = (K1 + 3) / 4;
    const int pad25 = (kb + 24) / 25 * 25, pad5 = (kb + 4) / 5 * 5;
    unr = pad25 <= pad5 + 1 ? 25 : 5;
    KB1 = unr == 25 ? pad25 : pad5;
}

// ---- what the three plans share ---------------------------------------------------------------------------------------
// The refusals: the batch size, negative strides, rows of W shorter than A, a core that is not 8-byte aligned -- and, as the
// cores are visited for that anyway, the copy of the pointer tables (T: the kernel's table, or nullptr for none).
inline bool chain_plan_tables(const ChainStepArgs &c, const double **W, const double **X, double **T)
{
    if (c.nb < 1 || c.nb > SK_MAXB) return false;
    if (c.x_j < 0 || c.x_k < 0 || c.x_c < 0 || c.w_c < c.A) return false;
    for (int b = 0; b < c.nb; ++b) {
        if ((uintptr_t)c.X[b] & 7) return false;
        W[b] = c.W[b];
        X[b] = c.X[b];
        if (T) T[b] = c.T[b];
    }
    return true;
}

// the extents and strides every kernel-argument struct carries under the same names
template <class KA>
inline void chain_plan_scalars(const ChainStepArgs &c, KA &a)
{
    a.nb = c.nb; a.n = c.n; a.K1 = c.K1; a.A = c.A; a.A2 = c.A2; a.J = c.J;
    a.w_c = c.w_c; a.x_j = c.x_j; a.x_k = c.x_k; a.x_c = c.x_c; a.x_extent = c.x_extent;
    a.E = c.E;
}

// red_chunks partial results per problem
inline ChainLaunch chain_plan_launch(const ChainStepArgs &c, size_t lds, int grid, int red_chunks)
{
    ChainLaunch l{};
    l.lds = lds; l.grid = grid;
    l.slab = (int64_t)c.nb * red_chunks * c.J * c.A2;
    l.red_chunks = red_chunks; l.red_m = c.J; l.red_n = c.A2;
    l.flops = 2.0 * c.nb * (double)c.n * c.J * ((double)c.K1 * c.A + (double)c.A * c.A2);
    return l;
}

// ---- chain_step_kernel: 1 = covered, 0 = not -------------------------------------------------------------------------
inline int chain_fused_plan(const ChainStepArgs &c, int n_cu, bool force, ChainFusedPlan &p)
{
    if (c.J < 1 || c.J > 112 || c.K1 < 1 || c.K1 > 128 || c.A < 4 || c.A2 < 4 || c.n < 1) return 0;
    if ((c.A2 & 1) || ((uintptr_t)c.E & 15)) return 0;                 // 16-byte units of E rows
    int nq, sq, nn, sn;
    chain_tile_split(c.A, nq, sq);
    chain_tile_split(c.A2, nn, sn);
    if (nq != nn || sq != sn || nq + (sq ? 1 : 0) > 7 || nq < 1) return 0;   // one instantiation per (tiles, strips)
    p = ChainFusedPlan{};
    ChainStep &a = p.a;
    const bool wt = c.T != nullptr;
    if (!chain_plan_tables(c, a.W, a.X, wt ? a.T : nullptr)) return 0;
    chain_plan_scalars(c, a);
    int unr, KB1;
    chain_phase_a_runs(c.K1, unr, KB1);
    const int KB2 = nq * 4 + sq;                                         // k-blocks of phase B
    // the loader brings A x A2 doubles per slice while phase A runs K1 deep: a short phase A cannot hide it, and
    // there is little T to keep on chip anyway (the two-launch form is then the faster one: measured on C5)
    if (!force && 2 * c.K1 < c.A) return 0;
    a.AP = 16 * nq + 4 * sq;
    if (a.AP < 4 * KB2) return 0;
    const int64_t wl = (int64_t)4 * KB1 * a.AP;                          // doubles
    a.ebase = (int)((wl + 1) & ~(int64_t)1);
    if (!chain_e_image(c.A, c.A2, a.A2P, a.eunits)) return 0;
    // two E images for the small structures (the load of E_{k+1} then has a whole slice to land: their
    // phases are too short to hide it), one for the large ones (no LDS room; their phases are long)
    const int ebuf = nq <= 4 ? 2 : 1;
    const size_t lds = ((size_t)a.ebase + (size_t)a.eunits * 2 * ebuf) * 8;
    if (lds > 160 * 1024) return 0;
    // 32-bit byte offsets: the X walk (incl. the masked prefetch one slice past the end) and T
    if ((c.x_extent + c.x_k + 132 * c.x_c) * 8 >= (1ll << 32) - 64) return 0;
    if ((int64_t)c.A * c.n * c.A2 * 8 >= (1ll << 32) - 64) return 0;
    a.t_extent = (int64_t)c.A * c.n * c.J;
    if (wt && (a.t_extent + (int64_t)16 * c.n * c.J) * 8 >= (1ll << 32) - 64) return 0;
    // geometry: one workgroup per CU (the LDS images fill it), each a contiguous range of slices
    const int cus = n_cu;
    int wpp = cus / c.nb > 0 ? cus / c.nb : 1;
    if (wpp > c.n) wpp = c.n;
    // (one slice per workgroup -- a single tensor -- still beats the two-launch form: 313 vs 355 us per C3 sketch)
    a.wpp = wpp;
    // the deal of (row tile, range of DRM-rank tiles) pieces over the waves (chain_deal.h): up to 4 row tiles one
    // wave per row tile, beyond that 12 waves that read their piece from the table.  A levelled workgroup pays for the
    // pairing of its cut row tiles (a barrier and a round trip through the slab) once, about 4 us per launch measured on
    // single sketches, and gains about 3 us per slice at rank 100: it is dealt from two slices per workgroup on.
    const ChainDeal deal = chain_deal(c.J, c.A, c.A2, nq, sq, nn, sn, KB1, c.n >= 2 * wpp);
    if (deal.waves == CD_WAVES) {
        bool taken[CD_WAVES] = {};
        for (int i = 0; i < deal.npieces; ++i) taken[deal.piece[i].slot] = true;
        for (int s = 0; s < CD_WAVES; ++s)                               // the last wave and every other one without a piece
            if (!taken[s]) a.piece[s] = (unsigned)a.nload++ << 8 | (unsigned)CD_NONE << 16;
        for (int i = 0; i < deal.npieces; ++i) {
            const ChainPiece &pc = deal.piece[i];
            a.piece[pc.slot] = (unsigned)pc.tile | (unsigned)pc.q0 << 8 | (unsigned)pc.kind << 16;
        }
    }
    a.xcd_map = (wpp % 8 == 0 && wpp >= 8) ? 1 : 0;
    p.nq = nq; p.sq = sq; p.wt = wt; p.ebuf = ebuf; p.unr = unr; p.waves = deal.waves;
    p.l = chain_plan_launch(c, lds, c.nb * wpp, wpp);
    return 1;
}

// ---- chain_wide_kernel ----------------------------------------------------------------------------------------------
// Row tiles -> waves.  Wave w sits on SIMD w & 3 (two waves per SIMD); the tiles are dealt so that the SIMDs
// carry equal shares, SIMD 3 the lightest one: its second wave is the loader.  Returns false if the rows do not fit.
// tpw > 1: `tpw` tensors per workgroup, each with ceil(NT / 2) (or NT) waves of its own, in order.
inline bool cw_wave_table(int NT, bool mt2_ok, int tpw, ChainWide &a, bool &uses_mt2)
{
    memset(a.tile0, -1, sizeof(a.tile0));
    memset(a.tile1, -1, sizeof(a.tile1));
    memset(a.slot, 0, sizeof(a.slot));
    a.loader = 7;
    uses_mt2 = false;
    if (tpw > 1) {
        const int wpt = mt2_ok ? (NT + 1) / 2 : NT;
        if (tpw * wpt > 7) return false;
        int w = 0;
        for (int sl = 0; sl < tpw; ++sl)
            for (int t = 0; t < NT; ++w) {
                a.slot[w] = (signed char)sl;
                a.tile0[w] = (signed char)t++;
                if (mt2_ok && t < NT) { a.tile1[w] = (signed char)t++; uses_mt2 = true; }
            }
        return true;
    }
    if (NT <= 7) {
        for (int w = 0; w < NT; ++w) a.tile0[w] = (signed char)w;
        return true;
    }
    if (!mt2_ok || NT > 11) return false;          // SIMD 3 has one compute wave: at most two tiles there
    int next = 0;
    for (int s = 0; s < 4; ++s) {
        const int t = NT / 4 + (s < NT % 4 ? 1 : 0);
        const int first = s == 3 ? t : (t + 1) / 2;  // tiles of wave s; the rest go to wave s + 4
        if (first > 2 || t - first > 2) return false;
        a.tile0[s] = (signed char)next++;
        if (first == 2) { a.tile1[s] = (signed char)next++; uses_mt2 = true; }
        if (t - first >= 1) a.tile0[s + 4] = (signed char)next++;
        if (t - first == 2) { a.tile1[s + 4] = (signed char)next++; uses_mt2 = true; }
    }
    return next == NT;
}

inline int chain_wide_plan(const ChainStepArgs &c, int n_cu, bool force, ChainWidePlan &p)
{
    if (c.J < 1 || c.K1 < 1 || c.A < 1 || c.A2 < 1 || c.n < 1) return 0;
    if ((uintptr_t)c.E & 7) return 0;
    int nn, sn;
    chain_tile_split(c.A2, nn, sn);
    if (nn + (sn ? 1 : 0) > 10 || (nn == 10 && sn)) return 0;
    const int NT = (c.J + 15) / 16;
    if (NT > 11 || (NT > 7 && nn + (sn ? 1 : 0) > 7)) return 0;     // rows beyond 7 tiles need waves with two tiles
    p = ChainWidePlan{};
    ChainWide &a = p.a;
    const bool wt = c.T != nullptr;
    if (!chain_plan_tables(c, a.W, a.X, wt ? a.T : nullptr)) return 0;
    chain_plan_scalars(c, a);
    a.A2P = c.A2 + (c.A2 & 1);
    int unr, KB1;
    chain_phase_a_runs(c.K1, unr, KB1);
    // ---- chunk plan: the fewest chunks of A whose images fit the LDS; two row tiles per wave only with <= 3 chunk tiles.
    // Few rows per tensor (NT <= 3) and a batch: several tensors per workgroup, as many as have waves and LDS.
    bool uses_mt2 = false;
    int ci = -1, nac = 0, tpw = 1;
    size_t lds = 0;
    const int cus = n_cu;
    const bool out_mt2 = nn + (sn ? 1 : 0) <= 7;
    for (int tryn = 1; tryn <= c.A && tryn <= 64 && ci < 0; ++tryn) {
        const int need = (int)((cdiv(c.A, tryn) + 3) / 4 * 4);
        for (int i = 0; i < 7 && ci < 0; ++i) {
            const int ap = 16 * CW_NQ[i] + 4 * CW_SQ[i];
            if (ap < need) continue;
            const bool mt2_ok = CW_NQ[i] <= 3 && out_mt2;
            int want = 1;
            if (c.nb >= 2 && NT <= 3) {
                want = 7 / (mt2_ok ? (NT + 1) / 2 : NT);
                if (want > c.nb) want = c.nb;
                if (want < 1) want = 1;
            }
            const int64_t wimg = ((int64_t)4 * KB1 * ap + 1) & ~(int64_t)1;
            const int64_t units = (int64_t)2 * (ap / 4) * a.A2P;
            const int eunits = (int)cdiv(units, 64) * 64;
            if (eunits / 64 > CF_MAX_DMA) break;
            // tensors per workgroup: as many as fit beside ONE E image (two images if they fit as well)
            while (want > 1 && ((size_t)want * wimg + (size_t)eunits * 2) * 8 > 160 * 1024) --want;
            if (!cw_wave_table(NT, mt2_ok, want, a, uses_mt2)) { if (ap >= 64) break; continue; }
            const int ebase = (int)((int64_t)want * wimg);
            const size_t one = ((size_t)ebase + (size_t)eunits * 2) * 8, two = ((size_t)ebase + (size_t)eunits * 4) * 8;
            if (one > 160 * 1024) break;               // larger structures only need more: more chunks
            ci = i; nac = tryn; tpw = want;
            a.ac = need; a.ebase = ebase; a.eunits = eunits; a.wimg = (int)wimg;
            a.ebuf2 = two <= 160 * 1024 ? 1 : 0;
            lds = a.ebuf2 ? two : one;
        }
    }
    if (ci < 0) return 0;
    // TT rank much smaller than the DRM rank (C5: 20 against 50 / 100): the two-launch form merges the rows of ALL tensors
    // of the batch into one long-K product (no 20 -> 32 row padding) and wins -- measured per right step: 81 us against 101 us
    // with seven tensors per workgroup here (128 us with one); `force` (ttsk_chain_step_wide) takes this kernel anyway
    if (!force && 2 * c.K1 < c.A) return 0;
    if (!cw_wave_table(NT, CW_NQ[ci] <= 3 && out_mt2, tpw, a, uses_mt2)) return 0;
    a.tpw = tpw;
    a.nac = nac;
    // 32-bit byte offsets: the X walk (incl. the prefetch one slice past the end) and T
    if ((c.x_extent + c.x_k + ((int64_t)KB1 * 4 + 32) * c.x_c) * 8 >= (1ll << 32) - 64) return 0;
    a.t_extent = (int64_t)c.A * c.n * c.J;
    if (wt && (a.t_extent + (int64_t)80 * c.n * c.J) * 8 >= (1ll << 32) - 64) return 0;
    // geometry: one workgroup per CU, each a contiguous range of slices of one chunk
    const int ng = (c.nb + tpw - 1) / tpw;            // workgroup groups of tensors
    int wpp = cus / (ng * nac) > 0 ? cus / (ng * nac) : 1;
    if (wpp > c.n) wpp = c.n;
    a.wpp = wpp;
    const int units = wpp * nac;
    a.xcd_map = (units % 8 == 0) ? 1 : 0;
    p.ci = ci; p.nn = nn; p.sn = sn; p.wt = wt; p.unr = unr;
    p.mt2 = CW_NQ[ci] <= 3 && nn + (sn ? 1 : 0) <= 7;
    p.l = chain_plan_launch(c, lds, ng * units, units);
    return 1;
}

// ---- chain_sum_kernel: the wave table of phase B -----------------------------------------------------------------------
// The (NRT x NNF) full tiles are cut into one or two row bands, each band into rectangles of the bodies the kernel
// instantiates; the strip column (NS 4-wide strips, all row tiles) is a piece of its own or rides on a (1, 1) / (1, 3)
// rectangle.  The pieces (at most 8) are dealt to the wave slots so that the SIMDs -- waves s and s + 4 share SIMD s --
// carry level loads; cost of a piece = its 16x16x4 instructions per k-block (a 4-wide strip tile = 1/4).
struct CsPiece { int rt0, ct0, rt, ct, srt0, sr; double cost; };

inline bool cs_body_ok(int rt, int ct)
{
    static const int ok[][2] = {{1, 1}, {1, 2}, {1, 3}, {2, 1}, {2, 2}, {2, 3}, {3, 1}, {3, 2}, {4, 1}, {5, 1}};
    for (auto &b : ok)
        if (b[0] == rt && b[1] == ct) return true;
    return false;
}

inline void cs_bands(int left, int h, std::vector<int> &cur, std::vector<std::vector<int>> &out)
{
    if (left == 0) { out.push_back(cur); return; }
    for (int wdt = 1; wdt <= 3 && wdt <= left; ++wdt)
        if (cs_body_ok(h, wdt)) { cur.push_back(wdt); cs_bands(left - wdt, h, cur, out); cur.pop_back(); }
}

// best assignment of the pieces to 4 SIMDs x 2 slots: returns the largest SIMD load, slot[i] = wave of piece i
inline double cs_deal(const std::vector<CsPiece> &pc, std::vector<int> &slot)
{
    const int np = (int)pc.size();
    std::vector<int> order(np);
    for (int i = 0; i < np; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return pc[x].cost > pc[y].cost; });
    double best = 1e30;
    std::vector<int> cur(np), bst(np);
    double load[4] = {0, 0, 0, 0};
    int cnt[4] = {0, 0, 0, 0};
    // depth-first over SIMD choices, largest pieces first
    struct Rec {
        static void go(int i, const std::vector<CsPiece> &pc, const std::vector<int> &order, double *load, int *cnt, std::vector<int> &cur,
                       std::vector<int> &bst, double &best)
        {
            const int np = (int)pc.size();
            double mx = 0;
            for (int s = 0; s < 4; ++s) mx = load[s] > mx ? load[s] : mx;
            if (mx >= best) return;
            if (i == np) { best = mx; bst = cur; return; }
            const int p = order[i];
            bool tried_empty = false;
            for (int s = 0; s < 4; ++s) {
                if (cnt[s] >= 2) continue;
                if (cnt[s] == 0) { if (tried_empty) continue; tried_empty = true; }
                cur[p] = s + 4 * cnt[s];
                load[s] += pc[p].cost; cnt[s]++;
                go(i + 1, pc, order, load, cnt, cur, bst, best);
                load[s] -= pc[p].cost; cnt[s]--;
            }
        }
    };
    Rec::go(0, pc, order, load, cnt, cur, bst, best);
    slot = bst;
    return best;
}

inline bool cs_wave_table_search(int NRT, int NNF, int NS, ChainSumRole *role)
{
    if (NRT < 1 || NRT > 10 || (NS && NRT > CS_SRMAX)) return false;
    double best = 1e30;
    int best_reads = 1 << 30;
    std::vector<CsPiece> best_pc;
    std::vector<int> best_slot;
    for (int h1 = (NRT + 1) / 2; h1 <= NRT && h1 <= 5; ++h1) {
        const int h2 = NRT - h1;
        if (h2 > 5) continue;
        std::vector<std::vector<int>> b1, b2;
        std::vector<int> cur;
        if (NNF) cs_bands(NNF, h1, cur, b1); else b1.push_back({});
        if (h2 && NNF) cs_bands(NNF, h2, cur, b2); else b2.push_back({});
        for (auto &x1 : b1)
            for (auto &x2 : b2) {
                std::vector<CsPiece> pc;
                int c0 = 0;
                for (int wdt : x1) { pc.push_back({0, c0, h1, wdt, 0, 0, (double)h1 * wdt}); c0 += wdt; }
                c0 = 0;
                for (int wdt : x2) { pc.push_back({h1, c0, h2, wdt, 0, 0, (double)h2 * wdt}); c0 += wdt; }
                // the strip column (all row tiles): a piece of its own
                {
                    std::vector<CsPiece> q = pc;
                    if (NS) q.push_back({0, 0, 0, 0, 0, NRT, 0.25 * NRT * NS});
                    if (q.empty() || q.size() > 8) continue;
                    std::vector<int> slot;
                    const double mx = cs_deal(q, slot);
                    int reads = 0;
                    for (auto &pq : q) reads += pq.rt + pq.ct + (pq.sr ? pq.sr + NS : 0);
                    if (mx < best - 1e-9 || (mx < best + 1e-9 && reads < best_reads)) {
                        best = mx; best_reads = reads; best_pc = q; best_slot = slot;
                    }
                }
            }
    }
    if (best_pc.empty()) return false;
    for (int wv = 0; wv < 8; ++wv) { role[wv].body = 0; role[wv].rt0 = role[wv].ct0 = role[wv].pad0 = role[wv].pad1 = 0; }
    for (int i = 0; i < (int)best_pc.size(); ++i) {
        const CsPiece &pq = best_pc[i];
        ChainSumRole &r = role[best_slot[i]];
        r.body = (unsigned char)(pq.sr ? 128 + 16 * pq.sr + NS : 16 * pq.rt + pq.ct);
        r.rt0 = (unsigned char)pq.rt0; r.ct0 = (unsigned char)pq.ct0;
    }
    return true;
}

// (the search costs ~0.1 ms of host time: once per structure)
inline bool cs_wave_table(int NRT, int NNF, int NS, ChainSumRole *role)
{
    struct Entry { bool ok; ChainSumRole role[8]; };
    static std::mutex mu;
    static std::map<int, Entry> cache;
    std::lock_guard<std::mutex> lk(mu);
    const int key = (NRT * 64 + NNF) * 8 + NS;
    auto it = cache.find(key);
    if (it == cache.end()) {
        Entry e{};
        e.ok = cs_wave_table_search(NRT, NNF, NS, e.role);
        it = cache.emplace(key, e).first;
    }
    for (int wv = 0; wv < 8; ++wv) role[wv] = it->second.role[wv];
    return it->second.ok;
}

inline int chain_sum_plan(const ChainSumArgs &cc, int n_cu, bool force, ChainSumPlan &p)
{
    const ChainStepArgs &c = cc.s;
    constexpr int JS = 5, KB1 = 5;                      // the instantiated structure: J, K1 <= 20
    if (c.J < 1 || c.J > 4 * JS || c.K1 < 1 || c.K1 > 4 * KB1 || c.A < 4 || c.A > 128 || c.A2 < 4 || c.A2 > 128 || c.n < 1) return 0;
    if ((c.A2 & 1) || ((uintptr_t)c.E & 15)) return 0;                 // 16-byte units of E rows
    if (!force && c.nb < 4) return 0;                   // few terms: the rows of a workgroup would be mostly padding
    p = ChainSumPlan{};
    ChainSum &ka = p.ka;
    ChainSumS &a = ka.s;
    if (!chain_plan_tables(c, ka.W, ka.X, nullptr)) return 0;
    chain_plan_scalars(c, a);
    a.T = cc.Tint; a.t_b = cc.t_b; a.t_ld = cc.t_ld; a.t_extent = cc.t_extent;
    a.c_fast = c.x_c == 1 ? 1 : 0;
    const int JP = 4 * JS, KP = 4 * KB1;
    const int NAT = (c.A + 15) / 16;
    a.KB2 = (c.A + 3) / 4;
    // columns of Out: full tiles + up to two 4-wide strips
    chain_tile_split(c.A2, a.NNF, a.NS);
    a.A2P = std::max(c.A2 + (c.A2 & 1), 16 * a.NNF + 4 * a.NS);
    // terms per workgroup: as many as the LDS, the wave table and the W registers take
    int tpw = 0;
    size_t lds = 0;
    for (int t : {4, 2, 1}) {                           // (at least two waves per term: the G loader's share per lane)
        const int rows = t * JP, NRT = (rows + 15) / 16, RP = 16 * NRT + 2;
        const int64_t tl = (int64_t)4 * a.KB2 * RP;
        const int64_t units = (int64_t)2 * a.KB2 * a.A2P;                // 16-byte units of the E image
        const int64_t eun = cdiv(units, 64) * 64;
        const int64_t el = eun * 2, gl = (int64_t)t * KP * JP;
        const size_t need = (size_t)(tl + el + gl) * 8;
        if (need > 160 * 1024) continue;
        if ((NAT + 8 / t - 1) / (8 / t) > CS_NAMAX) continue;          // a-tiles per wave in phase A
        if (eun / 64 > 8 * CS_DMAMAX) continue;                         // E loader instructions per wave
        ChainSumRole tmp[8];
        if (!cs_wave_table(NRT, a.NNF, a.NS, tmp)) continue;
        tpw = t; lds = need;
        a.RP = RP;
        a.ebase = (int)tl; a.gbase = (int)(tl + el); a.eunits = (int)eun;
        for (int wv = 0; wv < 8; ++wv) ka.role[wv] = tmp[wv];
        break;
    }
    if (!tpw) return 0;
    a.tpw = tpw;
    // phase A: wave w computes the a-tiles [at0, at0 + na) of local term w % tpw
    int na_run = 0;
    {
        const int wpt = 8 / tpw, run = (NAT + wpt - 1) / wpt;
        na_run = run;
        for (int wv = 0; wv < 8; ++wv) {
            const int part = wv / tpw, at0 = part * run;
            ka.role[wv].term = (unsigned char)(wv % tpw);
            ka.role[wv].at0 = (unsigned char)at0;
            ka.role[wv].na = (unsigned char)std::max(0, std::min(run, NAT - at0));
        }
    }
    a.ngroups = (c.nb + tpw - 1) / tpw;
    const int cus = n_cu;
    // Slice ranges per term group = workgroups per group.  A workgroup costs ~20 k cycles before and after its slices
    // (set-up on a cold instruction cache, the switch, the partial results) during which its CU does nothing else -- 157 KB
    // of LDS and 2 x 256 registers per SIMD leave no room for a second one -- so the grid is NOT one workgroup per CU at
    // any price: (i) a workgroup gets at least ~32 k cycles of matrix-pipe time (one and a half times its fixed cost), (ii) a quarter of
    // the CUs is left to the kernel of the other chain, which the sketch drivers always have in flight beside this one.
    // (C5: 24 ranges of 5-6 slices for the right step and 16 of 8 for the left one instead of 32 of 4 each: 0.41 -> 0.39 ms
    // per sketch with two in flight, a single call unchanged.)
    int nr = cus / a.ngroups;
    {
        const int NRT = (tpw * JP + 15) / 16;
        const double slice_cyc = 64.0 * (2.0 * na_run * (JS / 4 + 0.25 * (JS % 4)) * KB1 + NRT * (a.NNF + 0.25 * a.NS) * a.KB2 / 4.0);
        const int min_slices = (int)(32000.0 / slice_cyc) + 1;
        nr = std::min(std::max(1, 3 * cus / 4 / a.ngroups), std::max(1, c.n / min_slices));
    }
    if (nr >= 8) nr = nr / 8 * 8;
    if (nr < 1) nr = 1;
    if (nr > c.n) nr = c.n;
    a.nranges = nr;
    a.xcd_map = (nr % 8 == 0) ? 1 : 0;
    a.kbase = c.n / nr; a.krem = c.n % nr;
    a.inv_ng = (1 << 20) / a.ngroups + 1;
    if ((int64_t)a.ngroups * nr * a.ngroups >= (1 << 20)) return 0;
    a.wpt = 8 / tpw;
    a.e_inv = e_image_inv(a.A2P);
    a.per = (KP * JP + a.wpt - 1) / a.wpt;
    a.gu = (a.per + 63) / 64;
    // 32-bit byte offsets
    const int64_t lim32 = (1ll << 32) - 64;
    if ((c.x_extent + c.x_k) * 8 >= lim32) return 0;
    if ((int64_t)c.A * c.n * c.A2 * 8 >= lim32) return 0;
    if (a.T && a.t_extent * 8 >= lim32) return 0;
    if (((int64_t)(c.K1 - 1) * c.w_c + c.A) * 8 >= lim32) return 0;
    if ((c.J > 1 && c.x_j * 8 >= lim32) || (c.K1 > 1 && c.x_c * 8 >= lim32)) return 0;
    a.w_c8 = (uint32_t)(c.w_c * 8);
    a.x_j8 = c.J > 1 ? (uint32_t)(c.x_j * 8) : 0u;
    a.x_c8 = c.K1 > 1 ? (uint32_t)(c.x_c * 8) : 0u;
    if (a.T) {
        if ((c.nb > 1 && cc.t_b * 8 >= lim32) || (c.A > 1 && (int64_t)c.n * cc.t_ld * 8 >= lim32)) return 0;
        a.t_b8 = c.nb > 1 ? (uint32_t)(cc.t_b * 8) : 0u;
        a.t_a8 = c.A > 1 ? (uint32_t)((int64_t)c.n * cc.t_ld * 8) : 0u;
    }
    if ((int64_t)c.nb * nr * c.J * c.A2 * 8 >= lim32) return 0;
    a.slab_r8 = (uint32_t)((int64_t)c.J * c.A2 * 8);
    a.slab_t8 = (uint32_t)((int64_t)nr * c.J * c.A2 * 8);
    p.na_run = na_run; p.wt = a.T != nullptr;
    p.l = chain_plan_launch(c, lds, a.ngroups * nr, nr);
    return 1;
}

}  // namespace ttsk
