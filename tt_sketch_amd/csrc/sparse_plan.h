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
// table rows [3][T] (uint64) | val[T] | j[T] (int) | the tail queue, T * qcols slots (ushort)
struct SgLds { size_t tile, tabs, ro, rv, rj, q, total; };

SG_HD inline SgLds sg_lds_layout(int tcols, int tab, int qcols, int T)
{
    SgLds L;
    L.tile = 0;
    L.tabs = L.tile + (size_t)T * tcols;
    L.ro = L.tabs + tab;
    L.rv = L.ro + 3 * T;
    L.rj = L.rv + T;
    L.q = L.rj + T / 2;
    L.total = L.q + ((size_t)T * qcols + 3) / 4;
    return L;
}

// table DMA: unit i of a block is unit i % units of nonzero i / units; the quotient by multiply and shift, exact for
// i < 32 * units, units <= 16 (checked for every such i by tests/test_sparse_plan.py)
inline int sg_rcp(int units) { return 65536 / units + 1; }
SG_HD inline int sg_div_units(int i, int rcp) { return (i * rcp) >> 16; }

struct SgPlanF {
    int kind, w;         // as SgF of sparse_pass.h (an absent factor: ones, width 1)
    int off;             // sampled: first column the products read in the staged tile; table: offset of its block behind the tile
    int units, rcp;      // table: a row of the block is ceil(w / 2) units of 16 bytes; sg_rcp(units)
};

struct SgPlan {
    SgPlanF f[3];
    int tcols, tab, qcols;           // row length of the tile; doubles of all table blocks; columns of the normal factors
    int NT, NS, T;
    size_t lds, wg_per_cu;           // dynamic LDS bytes of a workgroup; workgroups resident per CU
    size_t chunk, waves, blocks;     // nonzeros per wave; waves with work; workgroups of 4 waves
    int cellsP, cellsO;
    size_t psi_off, om_off, j_off, scratch;   // bytes: part_psi [4 blocks][2][cellsP], part_om [4 blocks][cellsO], part_j [4 blocks][3]
    char msg[160];                   // why not, when the status is not TTSK_OK
};

#define SG_PLAN_FAIL(status, ...) do { snprintf(p->msg, sizeof(p->msg), __VA_ARGS__); return status; } while (0)

inline int sg_plan(const ttsk_sg_factor *A, const ttsk_sg_factor *B, const ttsk_sg_factor *C, int c_left, size_t N, size_t n_cu, SgPlan *p)
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
        if (!(F.kind >= 0 && F.kind <= 3 && F.w >= 1 && F.w <= 32))
            SG_PLAN_FAIL(TTSK_ERR_ARG, "ttsk_sparse_gauss_pass: factor %d: kind %d, width %d", i, F.kind, F.w);
        if (F.kind == 3 && !(full >= 1 && full <= 32 && nnz >= 0 && nnz <= full && lo >= 0 && lo + F.w <= full))
            SG_PLAN_FAIL(TTSK_ERR_ARG, "ttsk_sparse_gauss_pass: factor %d: sign row of %d entries, %d non-zero, columns [%d, %d)", i, full,
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
    if (p->NT == 2 && SG_LDS_BUDGET / (sg_lds_layout(p->tcols, SG_T * p->tab, p->qcols, SG_T).total * 4 * 8 + fixed) < 2) p->T = 16;
    for (int i = 0; i < 3; ++i)
        if (p->f[i].kind == 1) p->f[i].off *= p->T;
    p->tab *= p->T;
    p->lds = sg_lds_layout(p->tcols, p->tab, p->qcols, p->T).total * 4 * 8;
    // waves: what is resident at once (NT = 1: three workgroups of 4 waves per CU by the registers; NT = 2: two, fewer by the
    // LDS of wide tiles), so that the grid is one even round; stretches of whole tiles
    const size_t by_regs = p->NT == 1 ? 3 : 2;
    p->wg_per_cu = SG_LDS_BUDGET / (p->lds + fixed);
    if (p->wg_per_cu > by_regs) p->wg_per_cu = by_regs;
    if (p->wg_per_cu < 1) SG_PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_sparse_gauss_pass: a staged tile of %d columns does not fit the LDS", p->tcols);
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

#undef SG_PLAN_FAIL

}  // namespace ttsk
