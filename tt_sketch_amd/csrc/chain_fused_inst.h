// Dispatch shared by the chain_fused_i*.hip instantiation units.
#pragma once
#include "chain_fused.h"

namespace ttsk {

// one E image for the large structures (no LDS room for two), two for the small ones
#define TTSK_CF_KERN(NF, STR, WT, EBUF, UNR) chain_step_kernel<NF, STR, NF, STR, 5, WT, 1, EBUF, UNR>
#define TTSK_CF_CASE(NF, STR, EBUF)                                                                          \
    if (nf == NF && str == STR && ebuf == EBUF)                                                              \
        return launch(unr == 25 ? (wt ? TTSK_CF_KERN(NF, STR, true, EBUF, 25) : TTSK_CF_KERN(NF, STR, false, EBUF, 25)) \
                                : (wt ? TTSK_CF_KERN(NF, STR, true, EBUF, 5) : TTSK_CF_KERN(NF, STR, false, EBUF, 5)),   \
                      grid, 512, lds, st, a);

}  // namespace ttsk
