// What the two passes over a dense tensor are launched with, decided on the host: the cover of ttsk_dense_first_pass
// (dense_pass.hip) and of ttsk_dense_left_pass (dense_left_pass.hip), the instantiation, the grid, the LDS and the scratch
// each launch gets, and the arguments of the sums that follow.
//
// Plain C++: no HIP types, so that the plans are compiled and checked by the host compiler alone
// (tests/test_dense_pass_cover.py) before any kernel reads them.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "ttsk.h"
#include "plan_common.h"

namespace ttsk {

// ---------------------------------------------------------------------------------------------------------------------------
// ttsk_dense_first_pass: dense_pass_kernel<NBW, TP, SP, ZT, ZS>, then dense_pass_reduce per kind, then dense_pass_zsum
//
// A workgroup is (block of NB rows bb, t range tr, q chunk qc, kind).  With `total = Q / 8` tiles of eight values of q,
// chunk qc walks the tiles [qc total / nqc, (qc + 1) total / nqc) -- `len` of them, none where there are fewer tiles than
// chunks -- from the rotated start
//     rot = len > 0 ? ((uint32_t)(qc * 2654435761u) >> 8) % len : 0,
// tile `rel` of the walk being it_beg + (rel + rot) mod len.  The id within a block of rows is decoded as
//     tr = (idl >> 3) % nt,   qc = (idl & 7) + 8 (idl / (8 nt)),
// and with two kinds the kinds alternate in groups of 8 consecutive workgroup ids.

// doubles per row of the P image: the columns in use rounded up to 16 mod 32 (rows kq, kq + 1 on disjoint halves of the banks):
// 48 for 2 tiles + 2 strips (40 used) and for 3 tiles, 80 for 4 tiles
constexpr int dp_prow(int TP, int SP) { return (16 * TP + 4 * SP + 15) / 32 * 32 + 16; }

struct DenseFirstPlan {
    bool one_kind, split;        // one kind of workgroup with one strip more of either set; two kinds, each half of the ranks
    int p_half, z_half;          // split: kind k owns the columns [k p_half, ..) of U and the rows [k z_half, ..) of Z
    int NBW, TP, SP, ZT, ZS;     // the instantiation: NB = 8 NBW rows per block, U as TP tiles + SP strips, Z as ZT tiles + ZS strips
    int NB, nbb;                 // rows per block, blocks of rows
    int nt, nqc;                 // t ranges (T / 16), q chunks (a multiple of 8)
    int nqc_want;                // the q chunks the grid asks for, before the tiles there are cap them
    int kinds;
    int64_t grid1, grid;         // workgroups of one kind, of the launch
    int64_t sl64;                // doubles per row of the slab: (4 TP + SP) x 64 lanes
    int64_t pr;                  // row length of P as the kernel reads it (even)
    size_t lds;                  // bytes
    size_t slab_bytes, pad_bytes;// SCRATCH_MISC: the partial U of every workgroup, then the padded copy of P (an odd r)
    int64_t zblock;              // elements of Z = elements between the partial Z of consecutive blocks
    size_t zpart_bytes;          // SCRATCH_GEMM: the blocks' partial Z (nbb > 1), else 0
    int64_t elems;               // threads of one dense_pass_reduce
    int p_off[2], pcount[2];     // per kind: first column and columns of U that its reduce writes (pcount <= 0: no launch)
    int z_off[2], zcount[2];     // per kind: first row and rows of Z that it stores (zcount <= 0: none) -- the kernel derives its
                                 // [z_off, z_end) itself from split, z_half and ll; stated here so that a test can check the ranges
    bool in_cover;               // the extents and the alignment are inside the cover (the 4 GB rule of the partial results comes after)
    char msg[200];              // why not, when the status is not TTSK_OK
};

// `misaligned`: the low four bits of the addresses of X, P and Z, ORed (U and C may lie anywhere)
inline int dense_first_plan(int64_t n0, int64_t Q, int64_t T, int64_t ll, int64_t r, unsigned misaligned, DenseFirstPlan *p)
{
    *p = DenseFirstPlan{};
    if (!(n0 > 0 && Q > 0 && T > 0 && ll > 0 && r > 0)) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_dense_first_pass: empty extent");
    if ((n0 & 31) || n0 > 64 * 64 || (T & 15) || (Q & 7) || ll > 32 || r > 64 || Q * T >= (1ll << 27) || (misaligned & 15))
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_dense_first_pass: shape outside the kernel's cover (first mode a multiple of 32, last mode a multiple "
                                        "of 16, middle extent a multiple of 8, left rank <= 32, right rank <= 64)");
    p->in_cover = true;
    const int nt = (int)(T / 16);
    // accumulator shapes: U as TP tiles + SP strips of columns, Z as ZT tiles + ZS strips of rows.  Up to 40 / 20: one kind of
    // workgroup, blocks of 64 values of b (the C2 shape).  Beyond, with whole blocks of 64: TWO kinds of workgroups, each with
    // half the columns of U and half the rows of Z -- the accumulators of all 64 b fit, Z needs no partial sums over blocks
    // of b, the matrix work stays proportional to the ranks, and the tile is read twice, the kinds of a (t range, q range) one
    // dispatch round apart on one XCD.  Otherwise (first mode a multiple of 32 only): blocks of 32 with wider accumulators.
    // just beyond 20 / 40 (r <= 44, ll <= 24): one more strip of either still fits one kind of workgroup (11 spilled registers, outside the step loop)
    const bool one_kind = !(n0 & 63) && (r > 40 || ll > 20) && r <= 44 && ll <= 24;
    const bool split = !one_kind && !(n0 & 63) && (r > 40 || ll > 20);
    const int p_half = split ? (int)((r + 1) / 2 + 3) / 4 * 4 : 0, z_half = split ? (int)((ll + 1) / 2 + 3) / 4 * 4 : 0;
    const int ushape = split ? (p_half <= 24 ? 3 : 4) : r <= 40 ? 0 : r <= 48 ? 1 : 2;
    const int zshape = split ? (z_half <= 12 ? 2 : 3) : ll <= 20 ? 0 : 1;
    const int TP = one_kind ? 2 : ushape == 0 ? 2 : ushape == 1 ? 3 : ushape == 2 ? 4 : ushape == 3 ? 1 : 2;
    const int SP = one_kind ? 3 : ushape == 0 || ushape == 3 ? 2 : 0;
    const int NB = (one_kind || split || (ushape == 0 && zshape == 0 && !(n0 & 63))) ? 64 : 32, nbb = (int)(n0 / NB);
    const int kinds = split ? 2 : 1;
    // q ranges: about 256 workgroups for one block of b, about 1024 over all blocks otherwise (several rounds over the CUs even
    // out the ranges); a multiple of 8, and not more than there are tiles
    int64_t nqc = 8 * std::max<int64_t>(1, (nbb == 1 ? 32 : (128 + nbb * nt / 2) / (nbb * nt)) / (nbb == 1 ? nt : 1));
    const int64_t nqc_want = nqc;
    nqc = std::min<int64_t>(nqc, 8 * cdiv(Q / 8, 8));          // at least one tile for most chunks
    const int64_t grid1 = (int64_t)nbb * nt * nqc, grid = grid1 * kinds;
    const int64_t sl64 = (4 * TP + SP) * 64;
    // partial results beyond 4 GB (many blocks of a large operand): not this kernel's case -- the caller forms the products separately
    if ((nbb > 1 && (int64_t)nbb * ll * Q * T * 8 > (4ll << 30)) || grid * NB * sl64 * 8 > (4ll << 30))
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_dense_first_pass: %d blocks of rows would need more than 4 GB of partial results", nbb);
    p->one_kind = one_kind;
    p->split = split;
    p->p_half = p_half;
    p->z_half = z_half;
    // one of twelve instantiations (NBW | TP, SP | ZT, ZS): (8 | 2, 2 | 1, 1), (8 | 2, 3 | 1, 2), the four of a split
    // (8 | 1, 2 or 2, 0 | 0, 3 or 1, 0), and with blocks of 32 rows (4 | 2, 2 or 3, 0 or 4, 0 | 1, 1 or 2, 0)
    p->NBW = NB / 8;
    p->TP = TP;
    p->SP = SP;
    if (one_kind) { p->ZT = 1; p->ZS = 2; }
    else if (split) { p->ZT = zshape == 2 ? 0 : 1; p->ZS = zshape == 2 ? 3 : 0; }
    else if (NB == 64) { p->ZT = 1; p->ZS = 1; }
    else { p->ZT = zshape == 0 ? 1 : 2; p->ZS = zshape == 0 ? 1 : 0; }
    p->NB = NB;
    p->nbb = nbb;
    p->nt = nt;
    p->nqc = (int)nqc;
    p->nqc_want = (int)nqc_want;
    p->kinds = kinds;
    p->grid1 = grid1;
    p->grid = grid;
    p->sl64 = sl64;
    p->pr = r + (r & 1);
    p->lds = (size_t)(2 * NB * 128 + 2 * 8 * dp_prow(p->TP, p->SP) + NB * (16 * p->ZT + 4 * p->ZS)) * 8;
    p->slab_bytes = (size_t)grid * NB * sl64 * 8;
    p->pad_bytes = (r & 1) ? (size_t)Q * p->pr * 8 + 64 : 0;
    p->zblock = ll * Q * T;
    p->zpart_bytes = nbb > 1 ? (size_t)nbb * p->zblock * 8 : 0;
    p->elems = (int64_t)NB * sl64 * nt * nbb;
    for (int k = 0; k < 2; ++k) {
        p->p_off[k] = k * p_half;
        p->pcount[k] = k >= kinds ? 0 : split ? (k == 0 ? std::min<int>(p_half, (int)r) : (int)r - p_half) : (int)r;
        // the kernel's z_end: kind 0 of a split stops at z_half where that lies below ll, every other kind at ll
        p->z_off[k] = k * z_half;
        p->zcount[k] = k >= kinds ? 0 : (split && k == 0 && z_half < ll ? z_half : (int)ll) - k * z_half;
    }
    return TTSK_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// ttsk_dense_left_pass: dense_left_pass_kernel<STRIP>, then two slab sums

constexpr int LP_CT = 512;       // columns per workgroup
constexpr int LP_XP = 528;       // row pitch of the X image (16 mod 32: the two k rows a half wave reads hit different banks)
constexpr int LP_MAXI3 = 9;      // i3 values a column tile may span: (3 + that) x 80 gathered A elements <= 1024 = two per thread

struct DenseLeftPlan {
    int ni3;                     // i3 values per column tile = 512 / n4 (>= 1)
    int nct;                     // column tiles = C / 512
    int xcd_map;                 // n2 a multiple of 8: the column tiles of one i2 on one XCD
    int strip;                   // l > 16: rows 16 .. 19 as a 4-row strip
    int nsets, ninstr;           // the A loader: images per k-block (3 + ni3), LDS-DMA instructions that bring their 40 nsets units --
                                 // the kernel derives both itself; wave w >= ninstr repeats the last instruction
    int64_t grid;                // workgroups: n2 nct
    size_t lds;                  // bytes
    int64_t slab;                // elements of each of the two slabs of partial Z_2 / E_3: [i2][l][C]
    size_t scratch_bytes;        // SCRATCH_GEMM
    double flops;
    char msg[200];
};

inline int dense_left_plan(int64_t n0, int64_t n1, int64_t n2, int64_t C, int64_t n4, int l, DenseLeftPlan *p)
{
    *p = DenseLeftPlan{};
    if (!(n0 >= 1 && n1 >= 1 && n2 >= 1 && C >= 1 && n4 >= 1 && l >= 1)) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_dense_left_pass: bad shape");
    const bool ok = n0 % 4 == 0 && C % LP_CT == 0 && C % n4 == 0 && n4 % 16 == 0 && LP_CT % n4 == 0 && LP_CT / n4 <= LP_MAXI3 &&
                    l <= 20 && n0 <= (1 << 20) && n1 <= (1 << 20) && n2 <= (1 << 16) && n2 * (C / LP_CT) < (1ll << 30) &&
                    (double)l * n0 * n1 * n2 * (C / n4) * 8 < 4.0e9 && (double)4 * n1 * n2 * C * 8 < 4.0e9;      // 32-bit lane offsets
    if (!ok)
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_dense_left_pass: shape (%lld, %lld, %lld, C = %lld, n4 = %lld), l = %d is outside the kernel's cover",
                  (long long)n0, (long long)n1, (long long)n2, (long long)C, (long long)n4, l);
    p->ni3 = (int)(LP_CT / n4);
    p->nct = (int)(C / LP_CT);
    p->xcd_map = (n2 % 8 == 0) ? 1 : 0;
    p->strip = l > 16 ? 1 : 0;
    p->nsets = 3 + p->ni3;
    p->ninstr = (p->nsets * 40 + 63) >> 6;
    // the partial Z_2 / E_3 of the n2 workgroup rows: [i2][l][C] each
    p->slab = n2 * l * C;
    p->scratch_bytes = 2 * (size_t)p->slab * 8 + 64;
    p->lds = ((size_t)4 * 4 * LP_XP + (size_t)4 * (((3 + p->ni3) * 80 + 127) / 128 * 128 + 128)) * 8;
    p->grid = n2 * p->nct;
    p->flops = 8.0 * l * (double)n0 * n1 * n2 * C;
    return TTSK_OK;
}

}  // namespace ttsk
