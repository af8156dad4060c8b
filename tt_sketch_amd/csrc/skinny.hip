// Host side of the barrier-free chain kernels (skinny.h): the plans of gemm_plan.h get their scratch, their profiling bracket
// and their launch here; the sums of the per-chunk slabs.
#include <cstdlib>
#include "skinny.h"
#include "prof.h"

namespace ttsk {

template <int D, int STR>
int launch_skinny_s_depth(const SkinnyS &a, int npt, int spt, size_t lds_bytes, int grid, hipStream_t st);
#define TTSK_S_EXT(D, STR) extern template int launch_skinny_s_depth<D, STR>(const SkinnyS &, int, int, size_t, int, hipStream_t)
TTSK_S_EXT(4, 0); TTSK_S_EXT(4, 1); TTSK_S_EXT(4, 2); TTSK_S_EXT(5, 0); TTSK_S_EXT(5, 1); TTSK_S_EXT(5, 2);
#undef TTSK_S_EXT

int launch_skinny_r_0(const SkinnyR &a, int nmt, int nnt, int grid, hipStream_t st);
int launch_skinny_r_1(const SkinnyR &a, int nmt, int nnt, int grid, hipStream_t st);
int launch_skinny_r_2(const SkinnyR &a, int nmt, int nnt, int grid, hipStream_t st);
int launch_skinny_r_3(const SkinnyR &a, int nmt, int nnt, int grid, hipStream_t st);

// out[m, n] (+)= alpha sum_c slab[c][m][n] per (problem, row tile) y; 16 chunk lanes x 16 consecutive n
__global__ __launch_bounds__(256) void skinny_r_reduce(const double *__restrict__ slab_all, int chunks, int M, int N,
                                                       int m_tiles, int64_t Mtot, ReduceOut outs, int64_t c_m,
                                                       int64_t c_n, double alpha, int accumulate)
{
    __shared__ double part[16][17];
    const int prob = blockIdx.y / m_tiles, tile = blockIdx.y - prob * m_tiles;
    const double *__restrict__ slab = slab_all + (int64_t)blockIdx.y * chunks * M * N;
    double *__restrict__ C = outs.C[prob];
    const int x = threadIdx.x & 15, z = threadIdx.x >> 4;
    const int64_t e = (int64_t)blockIdx.x * 16 + x, MN = (int64_t)M * N;
    double sum = 0.0;
    if (e < MN) {
        double v[8];
        for (int c0 = z; c0 < chunks; c0 += 16 * 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = c0 + 16 * u < chunks ? slab[(int64_t)(c0 + 16 * u) * MN + e] : 0.0;
#pragma unroll
            for (int u = 0; u < 8; ++u) sum += v[u];
        }
    }
    part[z][x] = sum;
    __syncthreads();
    if (z == 0 && e < MN) {
        double tot = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) tot += part[k][x];
        const int m = (int)(e / N), n = (int)(e - (int64_t)m * N);
        const int64_t row = (int64_t)tile * M + m;
        if (row < Mtot) {
            double *c = C + row * c_m + n * c_n;
            *c = accumulate ? *c + alpha * tot : alpha * tot;
        }
    }
}

// the same, two consecutive n per lane (16-byte loads and stores): N, c_m even, c_n = 1, 16-byte aligned bases.
// L element pairs x 16 chunk groups per block.  L = 16: 256 threads.  L = 64 (1024 threads) for many chunks of one small
// result (the fused chain step of a single tensor: one partial per mode index): a wave reads 1 KB of one chunk per
// instruction instead of four 256-byte pieces.
template <int L>
__global__ __launch_bounds__(16 * L) void skinny_r_reduce2(const double2 *__restrict__ slab_all, int chunks, int M, int N,
                                                           int m_tiles, int64_t Mtot, ReduceOut outs, int64_t c_m, double alpha,
                                                           int accumulate)
{
    __shared__ double2 part[16][L + 1];
    const int prob = blockIdx.y / m_tiles, tile = blockIdx.y - prob * m_tiles;
    const int64_t MN2 = (int64_t)M * N / 2;
    const double2 *__restrict__ slab = slab_all + (int64_t)blockIdx.y * chunks * MN2;
    double *__restrict__ C = outs.C[prob];
    const int x = threadIdx.x & (L - 1), z = threadIdx.x / L;
    const int64_t e = (int64_t)blockIdx.x * L + x;
    double2 sum = make_double2(0.0, 0.0);
    if (e < MN2) {
        double2 v[8];
        for (int c0 = z; c0 < chunks; c0 += 16 * 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = c0 + 16 * u < chunks ? slab[(int64_t)(c0 + 16 * u) * MN2 + e] : make_double2(0.0, 0.0);
#pragma unroll
            for (int u = 0; u < 8; ++u) { sum.x += v[u].x; sum.y += v[u].y; }
        }
    }
    part[z][x] = sum;
    __syncthreads();
    if (z == 0 && e < MN2) {
        double2 tot = make_double2(0.0, 0.0);
#pragma unroll
        for (int k = 0; k < 16; ++k) { tot.x += part[k][x].x; tot.y += part[k][x].y; }
        const int m = (int)(2 * e / N), n = (int)(2 * e - (int64_t)m * N);
        const int64_t row = (int64_t)tile * M + m;
        if (row < Mtot) {
            double2 *c = reinterpret_cast<double2 *>(C + row * c_m + n);
            double2 o = make_double2(alpha * tot.x, alpha * tot.y);
            if (accumulate) { const double2 old = *c; o.x += old.x; o.y += old.y; }
            *c = o;
        }
    }
}

int launch_r_reduce(hipStream_t st, const double *slab, const RReduceArgs &r)
{
    const RReducePlan p = r_reduce_plan(slab, r);
    const dim3 grid(p.gx, p.gy), block(p.block);
    if (p.variant == R_REDUCE_PAIRED_WIDE)
        return launch(skinny_r_reduce2<64>, grid, block, 0, st, (const double2 *)slab, r.chunks, r.M, r.N, r.m_tiles, r.Mtot, r.out, r.c_m,
                      r.alpha, r.accumulate);
    if (p.variant == R_REDUCE_PAIRED)
        return launch(skinny_r_reduce2<16>, grid, block, 0, st, (const double2 *)slab, r.chunks, r.M, r.N, r.m_tiles, r.Mtot, r.out, r.c_m,
                      r.alpha, r.accumulate);
    return launch(skinny_r_reduce, grid, block, 0, st, slab, r.chunks, r.M, r.N, r.m_tiles, r.Mtot, r.out, r.c_m, r.c_n, r.alpha,
                  r.accumulate);
}

#ifdef TTSK_LAB
static long long *lab_stamps() { const char *e = getenv("TTSK_SK_STAMPS"); return e ? (long long *)strtoull(e, nullptr, 0) : nullptr; }
#endif

int skinny_r_launch(SkinnyRPlan &p, int stream, hipStream_t st)
{
    SkinnyR &r = p.r;
#ifdef TTSK_LAB
    r.stamps = lab_stamps();
#endif
    r.slab = (double *)scratch(stream, SCRATCH_GEMM, p.scratch_bytes);
    if (!r.slab) return TTSK_ERR_HIP;
    ProfBracket prof(st, PROF_CURRENT, p.work, "skinny_r_kernel<%d, %d, 4>", p.nmt, p.nnt);
    const auto go = p.unit == 0 ? launch_skinny_r_0 : p.unit == 1 ? launch_skinny_r_1 : p.unit == 2 ? launch_skinny_r_2 : launch_skinny_r_3;
    const int rc = go(r, p.nmt, p.nnt, p.grid, st);
    prof.close();                                               // the slab kernel alone, not the reduce
    if (rc != TTSK_OK) return rc;
    if (launch_r_reduce(st, r.slab, p.red) != TTSK_OK) {
        set_error("skinny_r_reduce launch failed");
        return TTSK_ERR_HIP;
    }
    return 1;
}

int skinny_s_launch(SkinnySPlan &p, hipStream_t st)
{
#ifdef TTSK_LAB
    p.s.stamps = lab_stamps();
#endif
    ProfBracket prof(st, PROF_CURRENT, p.work, "skinny_s_kernel<%d, %d, %d, %d>", p.npt, p.spt, p.dring, p.str);
#define TTSK_S_GO(D) (p.str == 2 ? launch_skinny_s_depth<D, 2>(p.s, p.npt, p.spt, p.lds, p.grid, st) \
                      : p.str == 1 ? launch_skinny_s_depth<D, 1>(p.s, p.npt, p.spt, p.lds, p.grid, st) \
                                   : launch_skinny_s_depth<D, 0>(p.s, p.npt, p.spt, p.lds, p.grid, st))
    const int rc = p.dring == 4 ? TTSK_S_GO(4) : TTSK_S_GO(5);
#undef TTSK_S_GO
    return rc == TTSK_OK ? 1 : rc;
}

int skinny_try_batch(const ttsk_gemm_desc &d, int nb, const double *const *A, const double *const *B,
                     double *const *C, int stream, hipStream_t st)
{
    const int n_cu = device_num_cu();
    if (n_cu < 1) return TTSK_ERR_HIP;
    SkinnyRPlan r;
    if (skinny_r_plan(d, nb, A, B, C, n_cu, &r)) return skinny_r_launch(r, stream, st);
    SkinnySPlan s;
    if (skinny_s_plan(d, nb, A, B, C, n_cu, &s)) return skinny_s_launch(s, st);
    return 0;
}

}  // namespace ttsk
