// The closing sum of the one-pass kernels that leave per-workgroup partial sums (the gather kernels, the dense statistics,
// ttsk_sumsq): one workgroup adds them in the library's stated order (block_total, wave.h).
#include "common.h"

namespace ttsk {

// out[j] (+)= sum_b part[b][j], j < W <= 4: thread t sums b = t, t + 256, ... in ascending order, then block_total.
// nparts = 0: zeros (with `accumulate`: out as it is)
__global__ __launch_bounds__(256) void sum_partials_kernel(const double *__restrict__ part, unsigned nparts, int W,
                                                           double *__restrict__ out, int accumulate)
{
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (unsigned b = threadIdx.x; b < nparts; b += 256)
        for (int j = 0; j < W; ++j) acc[j] += part[(size_t)b * W + j];
    const double v = block_total(acc);
    if ((int)threadIdx.x < W) out[threadIdx.x] = accumulate ? out[threadIdx.x] + v : v;
}

int sum_partials(const double *part, unsigned nparts, int W, double *out, int accumulate, LaunchAt at)
{
    if (W < 1 || W > 4) {
        set_error("sum_partials: W = %d, 1 .. 4 are covered (%s:%d)", W, at.file, at.line);
        return TTSK_ERR_ARG;
    }
    return launch(sum_partials_kernel, dim3(1), dim3(256), 0, at, part, nparts, W, out, accumulate);
}

}  // namespace ttsk
