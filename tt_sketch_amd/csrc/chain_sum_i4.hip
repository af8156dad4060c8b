// Explicit instantiations of chain_sum_kernel with 4 a-tiles per wave in the first product (J, K1 <= 20), T written or not.
#include "chain_sum.h"

namespace ttsk {

template __global__ void chain_sum_kernel<5, 5, 4, false>(ChainSum);
template __global__ void chain_sum_kernel<5, 5, 4, true>(ChainSum);

int launch_chain_sum_4(const ChainSum &a, bool wt, size_t lds, int grid, hipStream_t st)
{
    return launch(wt ? chain_sum_kernel<5, 5, 4, true> : chain_sum_kernel<5, 5, 4, false>, dim3(grid), dim3(512), lds, st, a);
}

}  // namespace ttsk
