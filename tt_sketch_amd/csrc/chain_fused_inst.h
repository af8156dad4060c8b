// Dispatch shared by the chain_fused_i*.hip instantiation units.
#pragma once
#include "chain_fused.h"

namespace ttsk {

// one E image for the large structures (no LDS room for two), two for the small ones; a levelled launch (waves == CD_WAVES,
// DRM ranks of two full tiles to 100) has its own instantiation with the pieces' bodies
#define TTSK_CF_KERN(NF, STR, WT, EBUF, UNR, NWV) chain_step_kernel<NF, STR, NF, STR, 5, WT, 1, EBUF, UNR, NWV>
#define TTSK_CF_PICK(NF, STR, EBUF, NWV)                                                                      \
    (unr == 25 ? (wt ? TTSK_CF_KERN(NF, STR, true, EBUF, 25, NWV) : TTSK_CF_KERN(NF, STR, false, EBUF, 25, NWV)) \
               : (wt ? TTSK_CF_KERN(NF, STR, true, EBUF, 5, NWV) : TTSK_CF_KERN(NF, STR, false, EBUF, 5, NWV)))
#define TTSK_CF_CASE(NF, STR, EBUF)                                                                          \
    if (nf == NF && str == STR && ebuf == EBUF) {                                                            \
        if constexpr (NF >= CD_NQF_MIN && 4 * NF + STR <= CD_KB2_MAX)                                        \
            if (waves == CD_WAVES) return launch(TTSK_CF_PICK(NF, STR, EBUF, CD_WAVES), grid, 64 * CD_WAVES, lds, st, a); \
        return launch(TTSK_CF_PICK(NF, STR, EBUF, 8), grid, 512, lds, st, a);                                \
    }

}  // namespace ttsk
