// Small products (Omega_mu = L^T R, the first / last mode of the chains, Psi_0): a few MFLOP each,
// pure latency.  One wave per 16 x 32 output tile, operands straight from memory into MFMA
// registers for the whole K (ring of 8 k-blocks in flight), no LDS and no barrier; up to
// SK_MAXB problems of one shape (the tensors of a batch, or a uniformly strided batch) per launch.
// Long contractions (K >= 128: Omega of a sum of 32 terms has K = 640) are cut over 2, 4 or 8 waves of a
// workgroup, the partial tiles summed in wave order through LDS.
// tensor_train_sketch.py:8-19 (Omega), tensor_train_drm.py:79-88 (first mode) in the reference.
#include <cstdlib>
#include "prof.h"
#include "skinny.h"

#ifndef SMALL_DEPTH
#define SMALL_DEPTH 16       // k-blocks in flight per wave (operands written by the previous kernel come from another XCD's L2: ~2 us a round trip)
#endif

namespace ttsk {

// SmallG, the kernel's arguments: gemm_plan.h
constexpr int SG_D = SMALL_DEPTH;

__global__ __launch_bounds__(512) void small_gemm_kernel(SmallG a)
{
    __shared__ double part[7][64][9];                 // partial tiles of waves 1..7 (padded rows)
    const int lane = threadIdx.x & 63, x16 = lane & 15, kq = lane >> 4;
    const int ws = threadIdx.x >> 6, nws = blockDim.x >> 6;
    int w = blockIdx.x;
    const int nt = w % a.tiles_n;
    w /= a.tiles_n;
    const int mt = w % a.tiles_m, prob = w / a.tiles_m;
    const __amdgpu_buffer_rsrc_t ra = make_rsrc(uniform_ptr(a.A[prob]), a.a_extent * 8);
    const __amdgpu_buffer_rsrc_t rb = make_rsrc(uniform_ptr(a.B[prob]), a.b_extent * 8);
    const __amdgpu_buffer_rsrc_t rc = make_rsrc(uniform_ptr(a.C[prob]), a.c_extent * 8);
    const int row = 16 * mt + x16, col0 = 32 * nt + x16, col1 = col0 + 16;
    const uint32_t oa = row < a.M ? (uint32_t)(((int64_t)row * a.a_m + (int64_t)kq * a.a_k) * 8) : OOB_OFF;
    const uint32_t ob0 = col0 < a.N ? (uint32_t)(((int64_t)col0 * a.b_n + (int64_t)kq * a.b_k) * 8) : OOB_OFF;
    const uint32_t ob1 = col1 < a.N ? (uint32_t)(((int64_t)col1 * a.b_n + (int64_t)kq * a.b_k) * 8) : OOB_OFF;
    const uint32_t sa = (uint32_t)(4 * a.a_k * 8), sb = (uint32_t)(4 * a.b_k * 8);
    const int nkb_lane = (a.K - kq + 3) >> 2, KB = (a.K + 3) >> 2;
    // this wave's stretch of the k-blocks
    const int per = (KB + nws - 1) / nws, kb_beg = ws * per, kb_end = kb_beg + per < KB ? kb_beg + per : KB;
    const int ITER = kb_end > kb_beg ? (kb_end - kb_beg + SG_D - 1) / SG_D : 0;

    double ra_[SG_D], rb0[SG_D], rb1[SG_D];
    int kb_load = kb_beg;
    auto issue = [&](int d) {
        const bool ok = kb_load < nkb_lane && kb_load < kb_end;
        ra_[d] = ld8(ra, (ok && oa != OOB_OFF) ? oa + (uint32_t)kb_load * sa : OOB_OFF, 0);
        rb0[d] = ld8(rb, (ok && ob0 != OOB_OFF) ? ob0 + (uint32_t)kb_load * sb : OOB_OFF, 0);
        rb1[d] = ld8(rb, (ok && ob1 != OOB_OFF) ? ob1 + (uint32_t)kb_load * sb : OOB_OFF, 0);
        ++kb_load;
    };
#pragma unroll
    for (int d = 0; d < SG_D; ++d) issue(d);
    double acc[2][4];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[q][t] = 0.0;
    for (int it = 0; it < ITER; ++it) {
#pragma unroll
        for (int d = 0; d < SG_D; ++d) {
            double rA[4];
            rot4(ra_[d], rA);
            const double b0 = rb0[d], b1 = rb1[d];
            issue(d);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                acc[0][t] = mfma4(rA[t], b0, acc[0][t]);
                acc[1][t] = mfma4(rA[t], b1, acc[1][t]);
            }
        }
    }
    if (nws > 1) {                                     // partial tiles meet in wave 0, summed in wave order
        if (ws > 0) {
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int t = 0; t < 4; ++t) part[ws - 1][lane][4 * q + t] = acc[q][t];
        }
        __syncthreads();
        if (ws > 0) return;
        for (int o = 1; o < nws; ++o)
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[q][t] += part[o - 1][lane][4 * q + t];
    }
    // rotated A: acc[q][t] at lane (i = l>>4, beta = (l>>2)&3, j4 = l&3) is D[4((beta+t)&3) + i][4 beta + j4]
    const int i = lane >> 4, beta = (lane >> 2) & 3, j4 = lane & 3;
    uint32_t off[2][4];
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int m = 16 * mt + 4 * ((beta + t) & 3) + i, n = 32 * nt + 16 * q + 4 * beta + j4;
            off[q][t] = (m < a.M && n < a.N) ? (uint32_t)(((int64_t)m * a.c_m + (int64_t)n * a.c_n) * 8) : OOB_OFF;
            acc[q][t] *= a.alpha;
        }
    if (a.accumulate) {
        double old[2][4];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int t = 0; t < 4; ++t) old[q][t] = ld8(rc, off[q][t], 0);
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[q][t] += old[q][t];
    }
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int t = 0; t < 4; ++t) st8(rc, off[q][t], acc[q][t]);
}

int small_gemm_launch(const SmallGemmPlan &p, hipStream_t st)
{
    ProfBracket prof(st, PROF_CURRENT, p.work, "%s", p.name);
    const int rc = launch(small_gemm_kernel, dim3(p.grid), dim3(p.block), 0, st, p.g);
    return rc == TTSK_OK ? 1 : rc;
}

int small_try_batch(const ttsk_gemm_desc &d, int nb, const double *const *A, const double *const *B, double *const *C,
                    int stream, hipStream_t st)
{
    (void)stream;
    SmallGemmPlan p;
    return small_gemm_plan(d, nb, A, B, C, &p) ? small_gemm_launch(p, st) : 0;
}

int gemm_each(const ttsk_gemm_desc &d, int count, const double *const *A, const double *const *B, double *const *C, int stream,
              hipStream_t st)
{
    int rc = skinny_try_batch(d, count, A, B, C, stream, st);
    if (rc == 0) rc = small_try_batch(d, count, A, B, C, stream, st);
    if (rc != 0) return rc < 0 ? rc : TTSK_OK;
    for (int b = 0; b < count; ++b)
        if ((rc = ttsk_gemm(&d, A[b], B[b], C[b], nullptr, stream))) return rc;
    return TTSK_OK;
}

}  // namespace ttsk
