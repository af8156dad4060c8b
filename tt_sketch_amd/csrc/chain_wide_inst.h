// Dispatch shared by the chain_wide_i*.hip instantiation units (one unit per chunk structure).
#pragma once
#include "chain_wide.h"

namespace ttsk {

// waves with two row tiles exist only where the registers allow (chain_wide.hip asks cw_has_mt2 first)
constexpr bool cw_has_mt2(int nqf, int nnf, int strn) { return nqf <= 3 && nnf + (strn ? 1 : 0) <= 7; }

template <int NQF, int STRQ, int NNF, int STRN>
static int launch_cw_pick(const ChainWide &a, bool wt, int unr, size_t lds, int grid, hipStream_t st)
{
    constexpr bool MT2 = cw_has_mt2(NQF, NNF, STRN);
    auto kern = unr == 25 ? (wt ? chain_wide_kernel<NQF, STRQ, NNF, STRN, true, 25, MT2> : chain_wide_kernel<NQF, STRQ, NNF, STRN, false, 25, MT2>)
                          : (wt ? chain_wide_kernel<NQF, STRQ, NNF, STRN, true, 5, MT2> : chain_wide_kernel<NQF, STRQ, NNF, STRN, false, 5, MT2>);
    return launch(kern, grid, 512, lds, st, a);
}

#define TTSK_CW_OUT(NNF, STRN) \
    if (nn == NNF && sn == STRN) return launch_cw_pick<TTSK_CW_NQF, TTSK_CW_STRQ, NNF, STRN>(a, wt, unr, lds, grid, st);

// every output structure: up to 10 tiles (+ 0..2 strips of 4 columns behind the full tiles), in two halves so that
// each (chunk structure, half) is one translation unit of the parallel build
#define TTSK_CW_OUT_LO                                                                           \
        TTSK_CW_OUT(0, 1) TTSK_CW_OUT(0, 2)                                                      \
        TTSK_CW_OUT(1, 0) TTSK_CW_OUT(1, 1) TTSK_CW_OUT(1, 2)                                    \
        TTSK_CW_OUT(2, 0) TTSK_CW_OUT(2, 1) TTSK_CW_OUT(2, 2)                                    \
        TTSK_CW_OUT(3, 0) TTSK_CW_OUT(3, 1) TTSK_CW_OUT(3, 2)                                    \
        TTSK_CW_OUT(4, 0) TTSK_CW_OUT(4, 1) TTSK_CW_OUT(4, 2)
#define TTSK_CW_OUT_HI                                                                           \
        TTSK_CW_OUT(5, 0) TTSK_CW_OUT(5, 1) TTSK_CW_OUT(5, 2)                                    \
        TTSK_CW_OUT(6, 0) TTSK_CW_OUT(6, 1) TTSK_CW_OUT(6, 2)                                    \
        TTSK_CW_OUT(7, 0) TTSK_CW_OUT(7, 1) TTSK_CW_OUT(7, 2)                                    \
        TTSK_CW_OUT(8, 0) TTSK_CW_OUT(8, 1) TTSK_CW_OUT(8, 2)                                    \
        TTSK_CW_OUT(9, 0) TTSK_CW_OUT(9, 1) TTSK_CW_OUT(9, 2)                                    \
        TTSK_CW_OUT(10, 0)

}  // namespace ttsk
