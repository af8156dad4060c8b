// Explicit instantiations of skinny_s_kernel for one ring depth (one translation unit per depth
// keeps the parallel build short).
#pragma once
#include "skinny.h"

namespace ttsk {

template <int D, int STR>
int launch_skinny_s_depth(const SkinnyS &a, int npt, int spt, size_t lds_bytes, int grid, hipStream_t st)
{
#define TTSK_S_CASE(N) if (npt == N) return launch(spt == 2 ? skinny_s_kernel<N, 2, D, STR> : (spt == 1 ? skinny_s_kernel<N, 1, D, STR> : skinny_s_kernel<N, 0, D, STR>), grid, 512, lds_bytes, st, a)
    TTSK_S_CASE(1); TTSK_S_CASE(2); TTSK_S_CASE(3); TTSK_S_CASE(4);
    TTSK_S_CASE(5); TTSK_S_CASE(6); TTSK_S_CASE(7); TTSK_S_CASE(8);
#undef TTSK_S_CASE
    set_error("skinny_s: no instantiation for %d/%d tiles", npt, spt);
    return TTSK_ERR_ARG;
}

}  // namespace ttsk
