// Generic strided / batched fp64 contraction on MFMA 16x16x4 (gfx950).
//
//   C[b,m,n] (+)= alpha * sum_{ko,ki} kscale[ko,ki] * A[b,m,ko,ki] * B[b,ko,ki,n]
//
// This is the workhorse behind every einsum of the sketch path that is not served by
// a fused kernel (CP / Tucker / dense inputs, DenseGaussianDRM, Omega products, the
// pinv / QR applications).  Arbitrary element strides make Tensor.T, rank_min:rank_max
// slices and unfoldings zero-copy views.
//
// Tiling: one 256-thread workgroup (4 wave64, 2x2) per BM x BN tile of C, BK = 32 (gemm_kernel.h).
// A and B tiles are staged in LDS in one of two layouts chosen by which index is
// contiguous in global memory, so that both the global read and the LDS write are
// conflict free and the MFMA fragment reads (ds_read_b64) hit 64 distinct banks:
//   "m-fast": tile[k][m], ld = BM+16 (== 16 mod 32)   "k-fast": tile[m][k], ld = 18 (== 2 mod 32)
// Split-K over (ko,ki) through gridDim.z into slabs that splitk_reduce_kernel sums.
// Which kernel family takes a call, and with what, is decided in gemm_plan.h (gemm_route and the plans); this file holds the
// entry point, the tile launcher and the split-K reduce.
#include <cstdlib>
#include "gemm_kernel.h"
#include "prof.h"
#include "skinny.h"   // gemm_plan.h and the launchers of its plans

namespace ttsk {

// C[b,m,n] (+)= alpha * sum_z partial[b*splits+z][tile(m), tile(n)][t][lane]
// 256 threads = 64 consecutive partial elements x 4 interleaved z-lanes, 4 independent loads in
// flight per thread, LDS combine: the sum over ~100 slabs costs ~8 dependent round trips, not 100.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(ttsk_gemm_desc d, const double *__restrict__ partial,
                                                            double *__restrict__ C, int splits, int64_t tiles_m,
                                                            int64_t tiles_n, int rota)
{
    __shared__ double red[4][64];
    const int64_t per_b = tiles_m * tiles_n * 256;
    const int64_t total = d.batch * per_b;
    const int e = threadIdx.x & 63, g = threadIdx.x >> 6;
    for (int64_t g0 = (int64_t)blockIdx.x * 64; g0 < total; g0 += (int64_t)gridDim.x * 64) {
        const int64_t idx = g0 + e;                 // per_b is a multiple of 256: a group never straddles b
        const int64_t b = idx / per_b, rem = idx - b * per_b;
        const double *p = partial + (b * splits) * per_b + rem;
        double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        int z = g;
        for (; z + 12 < splits; z += 16) {
            s0 += p[(int64_t)z * per_b];
            s1 += p[(int64_t)(z + 4) * per_b];
            s2 += p[(int64_t)(z + 8) * per_b];
            s3 += p[(int64_t)(z + 12) * per_b];
        }
        for (; z < splits; z += 4) s0 += p[(int64_t)z * per_b];
        red[g][e] = (s0 + s1) + (s2 + s3);
        __syncthreads();
        if (g == 0) {
            const double s = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
            const int64_t tile = rem >> 8;
            const int t = (int)((rem >> 6) & 3), lane = (int)(rem & 63);
            const int64_t ti = tile / tiles_n, tj = tile - ti * tiles_n;
            const int li = lane >> 4, beta = (lane >> 2) & 3, jj = lane & 3;
            const int rb = rota ? ((beta + t) & 3) : beta, cb = rota ? beta : ((beta + t) & 3);
            const int64_t m = ti * 16 + 4 * rb + li, n = tj * 16 + 4 * cb + jj;
            if (m < d.M && n < d.N) {
                double *c = C + b * d.c_b + m * d.c_m + n * d.c_n;
                *c = d.alpha * s + (d.accumulate ? *c : 0.0);
            }
        }
        __syncthreads();
    }
}

__global__ void fill3_kernel(double *C, int64_t batch, int64_t M, int64_t N, int64_t c_b, int64_t c_m,
                             int64_t c_n, double value)
{
    int64_t tot = batch * M * N;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot;
         i += (int64_t)gridDim.x * blockDim.x) {
        int64_t n = i % N, t = i / N;
        int64_t m = t % M, b = t / M;
        C[b * c_b + m * c_m + n * c_n] = value;
    }
}

static int launch_splitk_reduce(const GemmTilePlan &p, hipStream_t st)
{
    const GemmLaunch &g = p.g;
    return launch(splitk_reduce_kernel, dim3(p.red_grid), dim3(256), 0, st, g.d, g.partial, g.C, g.splits, p.tiles_m, p.tiles_n,
                  p.rota);
}

// gemm_tile_plan gets its split-K slabs, its bracket and its launch, then the sum of the slabs
static int gemm_tile_launch(GemmTilePlan &p, int stream, hipStream_t st)
{
    GemmLaunch &g = p.g;
    if (p.partial_bytes) {
        g.partial = (double *)scratch(stream, SCRATCH_GEMM, p.partial_bytes);
        if (!g.partial) return TTSK_ERR_HIP;
    }
    int rc;
    // the tile kernel alone, not the split-K reduce: <waves along m, n, tiles per wave along m, n, layouts>
    ProfBracket prof(st, PROF_CURRENT, p.work, "gemm_f64_kernel<%d, %d, %d, %d, %s, %s>", p.wm, p.wn, p.tm, p.tn,
                     p.ak ? "true" : "false", p.bk ? "true" : "false");
    if (p.ak && p.bk) rc = launch_gemm_layout<true, true>(g, st);
    else if (p.ak) rc = launch_gemm_layout<true, false>(g, st);
    else if (p.bk) rc = launch_gemm_layout<false, true>(g, st);
    else rc = launch_gemm_layout<false, false>(g, st);
    prof.close();
    if (rc || !g.partial) return rc;
    return launch_splitk_reduce(p, st);
}

static int launched(int rs) { return rs < 0 ? rs : TTSK_OK; }     // of a plan's launcher: 1 = launched, < 0 = error

}  // namespace ttsk

using namespace ttsk;

extern "C" {

// route (gemm_plan.h gemm_route: which family, with its plan), then scratch and launch
int ttsk_gemm(const ttsk_gemm_desc *dp, const double *A, const double *B, double *C,
              const double *k_scale, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(dp && A && B && C, "ttsk_gemm: NULL argument");
    ttsk_gemm_desc d = *dp;
    const int n_cu = device_num_cu();
    if (n_cu < 1) return TTSK_ERR_HIP;
    GemmRoute r;
    if (const int rc = gemm_route(d, A, B, C, k_scale, n_cu, &r)) {
        set_error("%s", r.msg);
        return rc;
    }
    static int trace = [] { const char *e = getenv("TTSK_GEMM_TRACE"); return e ? atoi(e) : 0; }();
    if (trace && r.kind != GEMM_EMPTY)
        fprintf(stderr, "ttsk_gemm b=%lld M=%lld N=%lld Ko=%lld Ki=%lld | a: b%lld m%lld ko%lld ki%lld | b: b%lld ko%lld ki%lld n%lld | c: b%lld m%lld n%lld acc=%d\n",
                (long long)d.batch, (long long)d.M, (long long)d.N, (long long)d.Ko, (long long)d.Ki, (long long)d.a_b,
                (long long)d.a_m, (long long)d.a_ko, (long long)d.a_ki, (long long)d.b_b, (long long)d.b_ko,
                (long long)d.b_ki, (long long)d.b_n, (long long)d.c_b, (long long)d.c_m, (long long)d.c_n, d.accumulate);
    int rs;
    switch (r.kind) {
    case GEMM_EMPTY: return TTSK_OK;
    case GEMM_K0:
        if (d.accumulate) return TTSK_OK;
        return launch(fill3_kernel, dim3(256), dim3(256), 0, st, C, d.batch, d.M, d.N, d.c_b, d.c_m, d.c_n, 0.0);
    case GEMM_ROWS_LONGK: return launched(rows_longk_launch(r.rl, stream, st));
    case GEMM_SKINNY_R: return launched(skinny_r_launch(r.sr, stream, st));
    case GEMM_SKINNY_S: return launched(skinny_s_launch(r.ss, st));
    case GEMM_SMALL: return launched(small_gemm_launch(r.sm, st));
    case GEMM_LONGK_BATCH:
        // up to SK_MAXB slices per launch; the route planned the first group
        for (int64_t b0 = 0; b0 < d.batch; b0 += SK_MAXB) {
            const int cnt = (int)(d.batch - b0 < SK_MAXB ? d.batch - b0 : SK_MAXB);
            const double *Ap[SK_MAXB], *Bp[SK_MAXB];
            double *Cp[SK_MAXB];
            for (int b = 0; b < cnt; ++b) {
                Ap[b] = A + (b0 + b) * d.a_b; Bp[b] = B + (b0 + b) * d.b_b; Cp[b] = C + (b0 + b) * d.c_b;
            }
            rs = b0 == 0 ? skinny_r_launch(r.sr, stream, st) : skinny_try_batch(r.n, cnt, Ap, Bp, Cp, stream, st);
            if (trace) fprintf(stderr, "  long-K batch slice %lld: rs = %d\n", (long long)b0, rs);
            if (rs < 0) return rs;
            if (rs == 0) {
                // rejected (a slice's alignment / extent differs from the first ones'): the slices done so far stand, the
                // rest go through the generic tiles -- same result in both accumulate modes.  No input gets here
                // (tests/test_gemm_plan.py, the sweep of slice groups); kept as the way out should a plan's rules change.
                A += b0 * d.a_b; B += b0 * d.b_b; C += b0 * d.c_b;
                d.batch -= b0;
                if (const int rc = gemm_tile_plan(d, A, B, C, k_scale, &r.g); rc < 0) {
                    set_error("%s", r.g.msg);
                    return rc;
                }
                return gemm_tile_launch(r.g, stream, st);
            }
        }
        return TTSK_OK;
    default: return gemm_tile_launch(r.g, stream, st);
    }
}

}  // extern "C"
