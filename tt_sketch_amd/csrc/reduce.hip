// The closing sum of the one-pass kernels that leave per-workgroup partial sums (the gather kernels, the dense statistics,
// ttsk_sumsq, ttsk_cp_gram): one workgroup adds them in the library's stated order (block_total, wave.h).  ttsk_sum is that
// sum of a caller's own vector.
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

extern "C" int ttsk_sum(const double *dev_x, size_t n, double *dev_out, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(dev_out && (dev_x || n == 0), "ttsk_sum: NULL argument");
    if (n > 0xffffffffu) {
        ttsk::set_error("ttsk_sum: %zu values, below 2^32 is covered", n);
        return TTSK_ERR_UNSUPPORTED;
    }
    return ttsk::sum_partials(dev_x, (unsigned)n, 1, dev_out, 0, st);
}
