// What a sparse pass (sparse_pass.h) is launched with, decided on the host: where each factor sits in a wave's staged tile,
// the wave's LDS layout, the instantiation (NT, NS, T) of sg_pass_kernel, the grid and the carve-up of the scratch block.
//
// Plain C++: no HIP types, so that the plan is compiled and checked by the host compiler alone (tests/test_sparse_plan.py)
// before any kernel reads it.  What the kernel shares (the LDS layout, the lane mapping of the table DMA) is host and device
// code under the device compiler only.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "ttsk.h"
#include "plan_common.h"

#ifdef __HIPCC__
#define SG_HD __host__ __device__
#else
#define SG_HD
#endif

namespace ttsk {

constexpr int SG_T = 32;                         // nonzeros per staged tile (the stretches of the waves are multiples of it)
constexpr int SG_MIN_TILES = 8;                  // shortest stretch of a wave, in tiles of SG_T
constexpr size_t SG_LDS_BUDGET = 156 * 1024;     // of the 160 KB of a CU, for the workgroups resident on it
// static LDS of a workgroup: the kernel's salt[3][16 NT] and what the compiler may put around it
constexpr size_t sg_salt_bytes(int NT) { return 3 * 16 * (size_t)NT * sizeof(uint64_t); }
constexpr size_t SG_STATIC_SLACK = 64;

// per-wave LDS, offsets in doubles: tile[T][tcols] (the sampled factors) | table blocks [T][2 units] | byte offsets of the
// table rows [3][T] (uint64) | val[T] | j[T] (int) | the tail queue, T * qcols slots (ushort) | with chain factors: the running
// vectors [SG_CHAIN_GROUPS][2][SG_CHAIN_RANK], then the digits [digit rows][T] (int)
struct SgLds { size_t tile, tabs, ro, rv, rj, q, total, cv, cd; };

constexpr int SG_CHAIN_MAX = TTSK_SG_CHAIN_MAX;  // steps of a chain factor
constexpr int SG_CHAIN_RANK = 32;                // widest rank along a chain
constexpr int SG_CHAIN_GROUPS = 4;               // nonzeros whose chains a wave walks at a time: groups of 16 lanes (of 32 beyond rank 16)
constexpr int SG_CHAIN_VECS = SG_CHAIN_GROUPS * 2 * SG_CHAIN_RANK;

// doubles of the chain region of a wave: the running vectors and `digits` rows of T ints; nothing without a chain factor
SG_HD inline int sg_chain_doubles(int digits, int T) { return SG_CHAIN_VECS + (digits * T + 1) / 2; }

SG_HD inline SgLds sg_lds_layout(int tcols, int tab, int qcols, int T, int chain = 0)
{
    SgLds L;
    L.tile = 0;
    L.tabs = L.tile + (size_t)T * tcols;
    L.ro = L.tabs + tab;
    L.rv = L.ro + 3 * T;
    L.rj = L.rv + T;
    L.q = L.rj + T / 2;
    L.total = L.q + ((size_t)T * qcols + 3) / 4;
    L.cv = L.total;                                // (a chain region of 0 doubles: the layout of a pass without chain factors)
    L.cd = L.cv + (chain ? SG_CHAIN_VECS : 0);
    L.total += chain;
    return L;
}

// table DMA: unit i of a block is unit i % units of nonzero i / units; the quotient by multiply and shift, exact for
// i < 32 * units, units <= 16 (checked for every such i by tests/test_sparse_plan.py)
inline int sg_rcp(int units) { return 65536 / units + 1; }
SG_HD inline int sg_div_units(int i, int rcp) { return (i * rcp) >> 16; }

struct SgPlanF {
    int kind, w;         // as SgF of sparse_pass.h (an absent factor: ones, width 1)
    int off;             // sampled, chain: first column the products read in the staged tile; table: offset of its block behind the tile
    int units, rcp;      // table: a row of the block is ceil(w / 2) units of 16 bytes; sg_rcp(units).  chain: of its start row, rank[0] wide
};

// x / d for x < 2^31 and 1 <= d < 2^31 by multiply and shift: with 2^(L-1) < d <= 2^L, mul = ceil(2^(31+L) / d) < 2^32 and
// floor(x mul / 2^(31+L)) = floor(x / d) (the excess x (mul d - 2^(31+L)) / (d 2^(31+L)) is below (d - 1) / (d 2^L) < 1 / d).
// Held against divmod by tests/test_sparse_chain_plan.py.
struct SgDiv { uint32_t mul; int sh; };
inline SgDiv sg_div_make(uint64_t d)
{
    int L = 0;
    while ((1ull << L) < d) ++L;
    return SgDiv{(uint32_t)(((1ull << (31 + L)) + d - 1) / d), 31 + L};
}
SG_HD inline uint32_t sg_div(uint32_t x, SgDiv v) { return (uint32_t)(((uint64_t)x * v.mul) >> v.sh); }

// a chain factor (kinds 4 and 5 of ttsk_sg_factor) as the kernel walks it
struct SgPlanCh {
    int steps, has_table;
    int lo;                           // first column of the last rank the factor keeps
    int toff;                         // offset of the start rows' block in the table region (has_table)
    int doff;                         // first of its rows of digits: one per step
    int gsh;                          // lanes per nonzero: 1 << gsh, 16 or 32
    uint32_t rows, n[SG_CHAIN_MAX];   // divisors of the flat index, in the order they are taken
    SgDiv drows, dn[SG_CHAIN_MAX];
    int rank[SG_CHAIN_MAX + 1];
    int diag;                         // kind 5: the steps are diagonal, core[s] an (n[s], rank) table; everything above as for kind 4
};

// the digits of `flat`: the row of the start table (0 without one), then the index into each core; `j` is the last digit
// where the factor extends the prefix / suffix by the record's own mode (src 2, 3).  Digit s goes to digit[s * stride]; every
// one is below its n[s] whatever `flat` and `j` are (a remainder, or clamped), and the row below `rows`.
SG_HD inline uint32_t sg_chain_digits(const SgPlanCh &c, uint32_t flat, bool j_last, uint32_t j, uint32_t *digit, int stride)
{
    uint32_t rest = flat & 0x7fffffffu, row = 0;       // (the 32-bit streams hold nothing beyond; sg_div is exact below 2^31)
    if (c.has_table) {
        const uint32_t q = sg_div(rest, c.drows);
        row = rest - q * c.rows;
        rest = q;
    }
    for (int s = 0; s < c.steps; ++s) {
        if (j_last && s == c.steps - 1) {
            digit[s * stride] = j < c.n[s] ? j : c.n[s] - 1;
            break;
        }
        const uint32_t q = sg_div(rest, c.dn[s]);
        digit[s * stride] = rest - q * c.n[s];
        rest = q;
    }
    return row;
}

struct SgPlan {
    SgPlanF f[3];
    int tcols, tab, qcols;           // row length of the tile; doubles of all table blocks; columns of the normal factors
    SgPlanCh ch[3];                  // the chain factors
    int has_chain, digits, chain;    // any; rows of digits of all of them; doubles of the chain region (0 without a chain factor)
    int NT, NS, T;
    size_t lds, wg_per_cu;           // dynamic LDS bytes of a workgroup; workgroups resident per CU
    size_t chunk, waves, blocks;     // nonzeros per wave; waves with work; workgroups of 4 waves
    int cellsP, cellsO;
    size_t psi_off, om_off, j_off, scratch;   // bytes: part_psi [4 blocks][2][cellsP], part_om [4 blocks][cellsO], part_j [4 blocks][3]
    char msg[160];                   // why not, when the status is not TTSK_OK
};

// the chain factor at position i: its descriptor checked and restated as p->ch[i]
inline int sg_plan_chain(const ttsk_sg_factor *f, int i, int w32, SgPlan *p)
{
    const SgPlanF &F = p->f[i];
    SgPlanCh &c = p->ch[i];
    const ttsk_sg_chain *ch = f->chain;
    if (!ch) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_sparse_gauss_pass: factor %d: a chain factor without its descriptor", i);
    if (!w32)
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_sparse_gauss_pass: factor %d: a chain factor takes the 32-bit streams only", i);
    if (!(ch->steps >= 0 && ch->steps <= SG_CHAIN_MAX))
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_sparse_gauss_pass: factor %d: chain of %d steps, up to %d are covered", i, ch->steps, SG_CHAIN_MAX);
    if (!ch->rows && ch->steps == 0) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_sparse_gauss_pass: factor %d: chain with neither a table nor a core", i);
    if (ch->rows >= (1ull << 31))
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_sparse_gauss_pass: factor %d: chain table of %llu rows, below 2^31 is covered", i, (unsigned long long)ch->rows);
    c.steps = ch->steps;
    c.has_table = ch->rows > 0;
    c.rows = (uint32_t)ch->rows;
    if (c.has_table) c.drows = sg_div_make(ch->rows);
    int widest = 1;
    for (int s = 0; s <= c.steps; ++s) {
        c.rank[s] = ch->rank[s];
        if (c.rank[s] < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_sparse_gauss_pass: factor %d: chain rank %d is %d", i, s, c.rank[s]);
        if (c.rank[s] > SG_CHAIN_RANK)
            PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_sparse_gauss_pass: factor %d: chain rank %d is %d, up to %d are covered", i, s, c.rank[s], SG_CHAIN_RANK);
        if (c.rank[s] > widest) widest = c.rank[s];
    }
    if (c.diag) {                                  // one rank throughout; without a table the start is that many ones
        for (int s = 1; s <= c.steps; ++s)
            if (c.rank[s] != c.rank[0])
                PLAN_FAIL(TTSK_ERR_ARG, "ttsk_sparse_gauss_pass: factor %d: a diagonal chain of ranks %d and %d, it has one rank throughout", i, c.rank[0], c.rank[s]);
    } else if (!c.has_table && c.rank[0] != 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_sparse_gauss_pass: factor %d: chain from the first core with rank %d in front of it", i, c.rank[0]);
    for (int s = 0; s < c.steps; ++s) {
        if (!ch->core[s]) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_sparse_gauss_pass: factor %d: chain core %d is NULL", i, s);
        if (ch->n[s] < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_sparse_gauss_pass: factor %d: chain mode %d has size %lld", i, s, (long long)ch->n[s]);
        if (ch->n[s] >= (1ll << 31))
            PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_sparse_gauss_pass: factor %d: chain mode %d of size %lld, below 2^31 is covered", i, s, (long long)ch->n[s]);
        c.n[s] = (uint32_t)ch->n[s];
        c.dn[s] = sg_div_make((uint64_t)ch->n[s]);
    }
    c.lo = f->rank_min;
    if (!(c.lo >= 0 && c.lo + F.w <= c.rank[c.steps]))
        PLAN_FAIL(TTSK_ERR_ARG, "ttsk_sparse_gauss_pass: factor %d: columns [%d, %d) of a chain that ends in rank %d", i, c.lo, c.lo + F.w, c.rank[c.steps]);
    c.gsh = widest <= 16 ? 4 : 5;
    return TTSK_OK;
}

// w32: the pass reads the 32-bit streams (what a chain factor needs)
inline int sg_plan(const ttsk_sg_factor *A, const ttsk_sg_factor *B, const ttsk_sg_factor *C, int c_left, size_t N, size_t n_cu, SgPlan *p,
                   int w32 = 0)
{
    *p = SgPlan{};
    const ttsk_sg_factor *fs[3] = {A, B, C};
    int cols = 0, widest = 1, wmax = 1;
    for (int i = 0; i < 3; ++i) {
        SgPlanF &F = p->f[i];
        F.w = 1;
        if (!fs[i]) continue;
        F.kind = fs[i]->kind;
        if (F.kind) F.w = fs[i]->w;
        const int full = fs[i]->full, nnz = fs[i]->nnz, lo = fs[i]->rank_min;
        if (!(F.kind >= 0 && F.kind <= 5 && F.w >= 1 && F.w <= 32))
            PLAN_FAIL(TTSK_ERR_ARG, "ttsk_sparse_gauss_pass: factor %d: kind %d, width %d", i, F.kind, F.w);
        if (F.kind == 5) {                             // a chain with diagonal steps: planned and walked as kind 4, but for the flag
            F.kind = 4;
            p->ch[i].diag = 1;
        }
        if (F.kind == 3 && !(full >= 1 && full <= 32 && nnz >= 0 && nnz <= full && lo >= 0 && lo + F.w <= full))
            PLAN_FAIL(TTSK_ERR_ARG, "ttsk_sparse_gauss_pass: factor %d: sign row of %d entries, %d non-zero, columns [%d, %d)", i, full,
                      nnz, lo, lo + F.w);
        if (F.kind == 3) {                             // the whole row is staged; the products read its slice
            F.off = cols + lo;
            cols += full;
            if (full > widest) widest = full;
        } else if (F.kind == 2) {
            F.off = cols;
            cols += F.w;
            p->qcols += F.w;
        } else if (F.kind == 1) {                      // a block of its own behind the tile
            F.units = (F.w + 1) / 2;
            F.rcp = sg_rcp(F.units);
            F.off = p->tab;                            // in doubles per nonzero of the tile here; times the tile size below
            p->tab += 2 * F.units;
        } else if (F.kind == 4) {                      // its row in the tile; the start rows in a table block, the digits in the chain region
            SgPlanCh &c = p->ch[i];
            if (const int rc = sg_plan_chain(fs[i], i, w32, p)) return rc;
            F.off = cols;
            cols += F.w;
            if (c.has_table) {
                F.units = (c.rank[0] + 1) / 2;
                F.rcp = sg_rcp(F.units);
                c.toff = p->tab;
                p->tab += 2 * F.units;
            }
            c.doff = p->digits;
            p->digits += c.steps;
            p->has_chain = 1;
        }
        if (F.w > widest) widest = F.w;
        if (F.w > wmax) wmax = F.w;
    }
    p->NT = widest > 16 ? 2 : 1;
    p->NS = (p->NT == 2 && wmax > 16 && wmax <= 24) ? (wmax <= 20 ? 1 : 2) : 0;   // strips beyond the first 16 columns
    p->tcols = cols > 0 ? cols : 1;
    // tile of 32 nonzeros; of 16 where 32 would leave LDS for one wide workgroup per CU only
    const size_t fixed = sg_salt_bytes(p->NT) + SG_STATIC_SLACK;
    p->T = SG_T;
    const int chain32 = p->has_chain ? sg_chain_doubles(p->digits, SG_T) : 0;
    if (p->NT == 2 && SG_LDS_BUDGET / (sg_lds_layout(p->tcols, SG_T * p->tab, p->qcols, SG_T, chain32).total * 4 * 8 + fixed) < 2) p->T = 16;
    for (int i = 0; i < 3; ++i) {
        if (p->f[i].kind == 1) p->f[i].off *= p->T;
        if (p->f[i].kind == 4) p->ch[i].toff *= p->T;
    }
    p->tab *= p->T;
    p->chain = p->has_chain ? sg_chain_doubles(p->digits, p->T) : 0;
    p->lds = sg_lds_layout(p->tcols, p->tab, p->qcols, p->T, p->chain).total * 4 * 8;
    // waves: what is resident at once (NT = 1: three workgroups of 4 waves per CU by the registers; NT = 2: two, fewer by the
    // LDS of wide tiles), so that the grid is one even round; stretches of whole tiles
    const size_t by_regs = p->NT == 1 ? 3 : 2;
    p->wg_per_cu = SG_LDS_BUDGET / (p->lds + fixed);
    if (p->wg_per_cu > by_regs) p->wg_per_cu = by_regs;
    if (p->wg_per_cu < 1) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_sparse_gauss_pass: a staged tile of %d columns does not fit the LDS", p->tcols);
    const size_t resident = n_cu * 4 * p->wg_per_cu;
    p->chunk = ((N + resident - 1) / resident + SG_T - 1) / SG_T * SG_T;
    if (p->chunk < (size_t)SG_MIN_TILES * SG_T) p->chunk = (size_t)SG_MIN_TILES * SG_T;
    p->waves = (N + p->chunk - 1) / p->chunk;
    p->blocks = (p->waves + 3) / 4;
    const size_t wtot = p->blocks * 4;
    const int wA = p->f[0].w, wB = p->f[1].w, wC = p->f[2].w;
    p->cellsP = wA * wB;
    p->cellsO = C ? (c_left ? wC * wB : wA * wC) : 0;
    p->psi_off = 0;
    p->om_off = p->psi_off + wtot * 2 * (size_t)p->cellsP * 8;
    p->j_off = p->om_off + wtot * (size_t)p->cellsO * 8;
    p->scratch = p->j_off + wtot * 16 + 256;          // (three ints per wave, rounded up)
    return TTSK_OK;
}

}  // namespace ttsk
