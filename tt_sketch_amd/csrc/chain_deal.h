// The deal of a fused chain step's work over the waves of a workgroup (chain_fused.h), made on the host.
//
// Plain C++: no HIP types, so that the deal is compiled and checked by the host compiler alone
// (tests/test_chain_deal.py) before any kernel reads it.
//
// The unit of work is a piece: (row tile of 16 output rows, range of Q).  Q counts the tiles of the DRM rank a
// that phase A produces: Q < NQF a full 16-wide tile, NQF <= Q < NQF + STRQ a 4-wide strip.  Nothing in either
// phase couples two Q of one row tile, so a row tile may be cut at a tile boundary into
//   FIRST  the first cd_cut(NQF) full tiles              REST  the other full tiles and the strips
// run by two waves on different SIMDs; their results are partial sums of the same output rows.  A last row tile
// with at most 4 valid rows is a piece of its own kind, ROWS4: both products with the four-block 4x4x4 matrix
// instruction, a quarter of a row tile's 16x16x4 cycles.
//
// Up to 4 row tiles (J <= 64) one wave per row tile is level already: the deal is then wave w = row tile w in a
// workgroup of 8 waves, as it is for every shape that cutting does not improve.  Beyond that a workgroup has 12
// waves, three per SIMD (wave s of a workgroup sits on SIMD s & 3), the last one the loader: 11 slots for pieces.
// Row tiles are cut, the last ones first, and the pieces go longest first to the SIMD with the least work that
// still has a slot; of the numbers of cut row tiles the one with the least work on the busiest SIMD is kept,
// the smaller on a tie.  The cost of a piece is its matrix-pipe time per slice: 64 cycles per 16x16x4, 16 per
// 4x4x4 instruction.
#pragma once

namespace ttsk {

constexpr int CD_WAVES = 12;                   // waves of a levelled workgroup, the loader included
constexpr int CD_MAXPIECE = CD_WAVES - 1;
// DRM ranks a levelled workgroup is built for: at least two full tiles (one cannot be cut), at most 25 k-blocks in phase B
// (rank 100: beyond that the whole-range body does not fit the 168 registers of three waves per SIMD without spilling)
constexpr int CD_NQF_MIN = 2, CD_KB2_MAX = 25;
enum ChainPieceKind { CD_NONE = 0, CD_WHOLE = 1, CD_FIRST = 2, CD_REST = 3, CD_ROWS4 = 4 };

// full tiles of a in the FIRST piece of a cut row tile: about two thirds, the REST (with the strips) then pairs
// with a ROWS4 piece on one SIMD
constexpr int cd_cut(int nqf) { return nqf - (nqf + 1) / 3; }

struct ChainPiece {
    int tile;                                  // row tile: output rows 16 tile .. 16 tile + 15
    int q0, nq;                                // first Q and number of Q (strips included)
    int kind;
    int slot;                                  // wave of the workgroup; its SIMD is slot & 3
    long long cycles;                          // modelled matrix-pipe cycles per slice
};

struct ChainDeal {
    int waves;                                 // 8: one wave per row tile (as before); CD_WAVES: levelled
    int npieces;
    ChainPiece piece[CD_MAXPIECE];
    long long simd[4];                         // modelled matrix-pipe cycles per slice of each SIMD
    double useful;                             // the same for the J valid rows alone, all SIMDs together
    double cap() const
    {
        long long m = simd[0];
        for (int s = 1; s < 4; ++s) m = simd[s] > m ? simd[s] : m;
        return m > 0 ? useful / (4.0 * (double)m) : 0.0;
    }
};

// kb1: k-blocks of phase A as the kernel runs them (padded to whole unrolled runs); cut = false: one wave per row tile
// whatever J (the launch asks for that where a workgroup has too few slices to earn back a levelled workgroup's fixed cost)
inline ChainDeal chain_deal(int J, int A, int A2, int NQF, int STRQ, int NNF, int STRN, int kb1, bool cut = true)
{
    (void)A; (void)A2;
    const long long colB = 64ll * NNF + 16ll * STRN;                   // phase B: one k-block over the full width
    auto cost = [&](int nfull, int nstrip) {
        return (long long)kb1 * (64ll * nfull + 16ll * nstrip) + (long long)(4 * nfull + nstrip) * colB;
    };
    const long long cW = cost(NQF, STRQ);
    const long long cR = 16ll * (NQF + STRQ) * (kb1 + 4 * NNF + STRN);
    const int H = cd_cut(NQF);
    const int NW = (J + 15) / 16;
    const bool narrow = J % 16 >= 1 && J % 16 <= 4;

    ChainDeal best{};
    best.waves = 8;
    best.npieces = NW;
    for (int w = 0; w < NW; ++w) {
        best.piece[w] = ChainPiece{w, 0, NQF + STRQ, CD_WHOLE, w, cW};
        best.simd[w & 3] += cW;
    }
    best.useful = (double)J / 16.0 * (double)cW;
    if (!cut || NW <= 4 || NW > 7 || NQF < CD_NQF_MIN || 4 * NQF + STRQ > CD_KB2_MAX) return best;

    long long best_max = 0;
    for (int s = 0; s < 4; ++s) best_max = best.simd[s] > best_max ? best.simd[s] : best_max;
    const int nfull = narrow ? NW - 1 : NW;                            // row tiles run with 16x16x4 instructions
    for (int ncut = 0; ncut <= nfull; ++ncut) {
        if (nfull + ncut + (narrow ? 1 : 0) > CD_MAXPIECE) break;
        if (ncut == 0 && !narrow) continue;                            // that is the deal above
        ChainDeal d{};
        d.waves = CD_WAVES;
        d.useful = best.useful;
        int np = 0;
        for (int t = 0; t < nfull - ncut; ++t) d.piece[np++] = ChainPiece{t, 0, NQF + STRQ, CD_WHOLE, -1, cW};
        for (int t = nfull - ncut; t < nfull; ++t) d.piece[np++] = ChainPiece{t, 0, H, CD_FIRST, -1, cost(H, 0)};
        for (int t = nfull - ncut; t < nfull; ++t)
            d.piece[np++] = ChainPiece{t, H, NQF - H + STRQ, CD_REST, -1, cost(NQF - H, STRQ)};
        if (narrow) d.piece[np++] = ChainPiece{NW - 1, 0, NQF + STRQ, CD_ROWS4, -1, cR};
        d.npieces = np;
        // longest first (stable: equal pieces keep their row-tile order)
        for (int i = 1; i < np; ++i)
            for (int j = i; j > 0 && d.piece[j].cycles > d.piece[j - 1].cycles; --j) {
                const ChainPiece tmp = d.piece[j];
                d.piece[j] = d.piece[j - 1];
                d.piece[j - 1] = tmp;
            }
        int used[4] = {0, 0, 0, 0};
        const int room[4] = {3, 3, 3, 2};                              // the loader is the last wave of SIMD 3
        for (int i = 0; i < np; ++i) {
            int s = -1;
            for (int c = 0; c < 4; ++c)
                if (used[c] < room[c] && (s < 0 || d.simd[c] < d.simd[s])) s = c;
            d.piece[i].slot = s + 4 * used[s];                         // a SIMD's older waves get its longer pieces
            used[s] += 1;
            d.simd[s] += d.piece[i].cycles;
        }
        long long m = 0;
        for (int s = 0; s < 4; ++s) m = d.simd[s] > m ? d.simd[s] : m;
        if (m < best_max) {
            best_max = m;
            best = d;
        }
    }
    return best;
}

}  // namespace ttsk
