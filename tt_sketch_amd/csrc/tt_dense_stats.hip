// A tensor train against a dense tensor in one pass over the tensor: Tensor.error / Tensor.dot / Tensor.norm of the
// reference (tensor.py:53-88) for a DenseTensor argument, and TensorTrain.dense (tensor.py:48-50).
//
// The train is cut at one bond, T^{<k>} = L R with L (M x rho) and R (rho x N) row-major (formed by the caller with the
// contraction kernel: (M + N) rho numbers, small beside the M N of the tensor).  A workgroup of four waves takes tiles of
// 64 rows x 64 columns of T, each wave a 32 x 32 quarter: 2 x 2 accumulator tiles of v_mfma_f64_16x16x4, four matrix
// instructions (256 cycles of the pipe) for four fragment reads per k-block -- 32 bytes per clock and CU from an LDS that
// gives 128.  (A 64 x 32 wave tile halves the reads but, with the X tile in registers beside the accumulators, spilled
// 78 registers at two waves per SIMD; this form needs none.)  The K loop runs over chunks of 32
// of rho; a chunk of L (64 x 32) and of R (32 x 64) goes global -> registers -> LDS with zeros beyond M, N and rho, so
// that edge tiles and any rho >= 1 need no special instruction stream.  LDS images:
//   L chunk  Ls[row][k], row pitch 34 doubles: the 32 lanes of one half of a fragment read (16 rows x 2 k) fall on
//            dword banks 2 (17 row + k) mod 64 -- 17 is odd, so these are 32 different even banks: conflict-free,
//            and so are the staging writes (32 consecutive doubles of one row).
//   R chunk  Rs[k][col], row pitch 80 doubles = 64 + 16: the two k rows of a half read lie 32 banks apart.
// 37 KB per workgroup.  Inside a chunk every fragment address is the lane's base plus an immediate:
// the per-k-block loop carries no vector address arithmetic at all (an fp64 matrix instruction does
// not hide a wave's VALU work).
//
// Epilogue.  The X tile is requested in front of the last chunk's matrix instructions, in the accumulators' own lane
// layout (register r of lane l is row (l >> 4) + 4 r, column l & 15: sixteen lanes read one full 128-byte row segment),
// so its latency runs under that chunk and under the other workgroup of the CU; the barriers of the loop are
// `s_waitcnt lgkmcnt(0); s_barrier`, which does not wait for loads in flight as __syncthreads() would.  Each lane then adds
// x t, t^2, (t - x)^2 and x^2 of its 16 entries to four running sums and stores t only if an output array was given: the reconstruction never exists in memory.
//
// Order of the sums.  The grid is min(tiles rounded up to 8, 4096) workgroups, a function of M and N alone; workgroup b
// walks the tiles (b % 8) (grid / 8) + b / 8 + i grid -- the workgroups of one XCD (b % 8) take neighbouring tiles,
// row blocks fastest, so that they share the R chunk in their L2.  A lane sums its tiles in that order, the lanes of a
// wave and the four waves by block_total (wave.h), then the workgroups' quadruples by sum_partials (reduce.hip): no atomics,
// the same bits on every call, with or without the output array.
#include "common.h"
#include "prof.h"

namespace ttsk {

namespace {

constexpr int DS_BM = 64, DS_BN = 64, DS_KC = 32;
constexpr int DS_LP = DS_KC + 2;                    // row pitch of the L image (doubles)
constexpr int DS_RP = DS_BN + 16;                   // row pitch of the R image
constexpr int DS_LDS_BYTES = (DS_BM * DS_LP + DS_KC * DS_RP) * 8;
constexpr unsigned DS_MAX_BLOCKS = 4096;

struct DenseStats {
    const double *L, *R, *X;
    double *out, *part;
    int64_t M, N, rho, ldx, ldo;                    // ldx / ldo: row strides of X / out (R and the tile grid use N)
    int64_t nrb, tiles;                             // row blocks, tiles = nrb x column tiles
};

__global__ __launch_bounds__(256, 2) void tt_dense_stats_kernel(DenseStats a)
{
    extern __shared__ double ds_img[];
    double *const Ls = ds_img, *const Rs = ds_img + DS_BM * DS_LP;
    const int tid = threadIdx.x, lane = tid & 63, x16 = lane & 15, kq = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    double s[4] = {0.0, 0.0, 0.0, 0.0};             // x.t, t.t, |t - x|^2, x.x
    const int64_t M = a.M, N = a.N, rho = a.rho;
    const bool has_x = a.X != nullptr, has_out = a.out != nullptr, has_sums = a.part != nullptr;
    const unsigned G = gridDim.x;                   // a multiple of 8
    // the lane's fragment bases inside the images
    const int wr = w >> 1, wc = w & 1;              // the wave's 32 x 32 quarter of the tile
    const int la = (32 * wr + x16) * DS_LP + kq, rb_ = kq * DS_RP + 32 * wc + x16;
    // staging: L chunk 8 rows per step (row = tid >> 5, k = tid & 31), R chunk 4 k rows per step (k = tid >> 6, col = tid & 63)
    const int lk = tid & 31, lr = tid >> 5, rc = tid & 63, rk = tid >> 6;

    for (int64_t t = (int64_t)(blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3); t < a.tiles; t += G) {
        const int64_t ct = t / a.nrb, rblk = t - ct * a.nrb;
        const int64_t row0 = rblk * DS_BM, roww = row0 + 32 * wr, colw = ct * DS_BN + 32 * wc;
        v4d acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = v4d{0.0, 0.0, 0.0, 0.0};
        double xv[2][2][4];

        for (int64_t kc = 0; kc < rho; kc += DS_KC) {
            const int kn = (int)(rho - kc < DS_KC ? rho - kc : DS_KC), nkb = (kn + 3) >> 2;
            // ---- operands of the chunk into registers (addresses clamped into the arrays, zeros selected afterwards)
            double lv[8], rv[8];
            {
                const int kk = lk < kn ? lk : kn - 1;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    int64_t r = row0 + lr + 8 * i;
                    if (r >= M) r = M - 1;
                    lv[i] = a.L[r * rho + kc + kk];
                }
                int64_t c = ct * DS_BN + rc;
                if (c >= N) c = N - 1;
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    int k = rk + 4 * i;
                    if (k >= kn) k = kn - 1;
                    rv[i] = a.R[(kc + k) * N + c];
                }
            }
            lds_barrier();                          // the previous chunk's fragment reads are done
            {
                const bool kok = lk < kn;
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    Ls[(lr + 8 * i) * DS_LP + lk] = kok && row0 + lr + 8 * i < M ? lv[i] : 0.0;
                const bool cok = ct * DS_BN + rc < N;
#pragma unroll
                for (int i = 0; i < 8; ++i)
                    if (i < nkb) Rs[(rk + 4 * i) * DS_RP + rc] = cok && rk + 4 * i < kn ? rv[i] : 0.0;
            }
            lds_barrier();
            // ---- the X tile, once per tile: requested in front of the last chunk's matrix instructions, when the staging
            // registers are free again (the loads return under that chunk's k-blocks)
            if (kc + DS_KC >= rho && has_x) {
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        int64_t c = colw + 16 * j + x16;
                        if (c >= N) c = N - 1;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            int64_t m = roww + 16 * i + kq + 4 * r;
                            if (m >= M) m = M - 1;
                            xv[i][j][r] = a.X[m * a.ldx + c];
                        }
                    }
            }
#pragma unroll
            for (int kb = 0; kb < DS_KC / 4; ++kb) {
                if (kb < nkb) {
                    double af[2], bf[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i) af[i] = LDS_UNPAIRED(Ls[la + 16 * i * DS_LP + 4 * kb]);
#pragma unroll
                    for (int j = 0; j < 2; ++j) bf[j] = LDS_UNPAIRED(Rs[rb_ + 4 * kb * DS_RP + 16 * j]);
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) acc[i][j] = mfma16(af[i], bf[j], acc[i][j]);
                }
            }
        }

        // ---- epilogue: rows >= M and columns >= N of T are exact zeros (zero operands); x is masked
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int64_t c = colw + 16 * j + x16;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t m = roww + 16 * i + kq + 4 * r;
                    const bool ok = m < M && c < N;
                    const double tv = acc[i][j][r];
                    if (has_out && ok) a.out[m * a.ldo + c] = tv;
                    if (has_sums) {
                        const double x = has_x && ok ? xv[i][j][r] : 0.0, d = tv - x;
                        s[0] = fma(x, tv, s[0]);
                        s[1] = fma(tv, tv, s[1]);
                        s[2] = fma(d, d, s[2]);
                        s[3] = fma(x, x, s[3]);
                    }
                }
            }
    }
    if (has_sums) {                                 // part[block][4]
        const double v = block_total(s);
        if (tid < 4) a.part[(size_t)blockIdx.x * 4 + tid] = v;
    }
}

// part[block][0] = sum of squares of the workgroup's share (grid-stride, so the share depends on n alone)
__global__ __launch_bounds__(256) void sumsq_kernel(const double *__restrict__ x, size_t n, double *__restrict__ part)
{
    double s[1] = {0.0};
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) s[0] = fma(x[i], x[i], s[0]);
    const double v = block_total(s);
    if (threadIdx.x == 0) part[blockIdx.x] = v;
}

}  // namespace

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_tt_dense_stats_ld(const double *dev_L, int64_t M, const double *dev_R, int64_t N, int64_t rho, const double *dev_x,
                           int64_t ld_x, double *dev_out, int64_t ld_out, double *dev_stats, int accumulate, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(M >= 1 && N >= 1 && rho >= 1, "ttsk_tt_dense_stats: extents M = %lld, N = %lld, rho = %lld must be positive",
             (long long)M, (long long)N, (long long)rho);
    TTSK_ARG(dev_L && dev_R, "ttsk_tt_dense_stats: NULL factor");
    if (!dev_out && !dev_stats) {
        set_error("ttsk_tt_dense_stats: neither dev_out nor dev_stats given");
        return TTSK_ERR_UNSUPPORTED;
    }
    TTSK_ARG(!dev_x || ld_x >= N, "ttsk_tt_dense_stats: row stride %lld of x below N = %lld", (long long)ld_x, (long long)N);
    TTSK_ARG(!dev_out || ld_out >= N, "ttsk_tt_dense_stats: row stride %lld of out below N = %lld", (long long)ld_out, (long long)N);
    DenseStats a{};
    a.L = dev_L; a.R = dev_R; a.X = dev_x; a.out = dev_out;
    a.M = M; a.N = N; a.rho = rho; a.ldx = ld_x; a.ldo = ld_out;
    a.nrb = cdiv(M, DS_BM);
    const int64_t nct = cdiv(N, DS_BN);
    if (nct > (INT64_MAX >> 1) / a.nrb) {
        set_error("ttsk_tt_dense_stats: %lld x %lld tiles", (long long)a.nrb, (long long)nct);
        return TTSK_ERR_UNSUPPORTED;
    }
    a.tiles = a.nrb * nct;
    const int64_t t8 = (a.tiles + 7) & ~(int64_t)7;
    const unsigned blocks = (unsigned)(t8 > DS_MAX_BLOCKS ? DS_MAX_BLOCKS : t8);
    if (dev_stats) {
        a.part = (double *)scratch(stream, SCRATCH_MISC, (size_t)blocks * 4 * 8);
        if (!a.part) return TTSK_ERR_HIP;
    }
    ProfBracket prof(st, PROF_EVAL, 2.0 * (double)rho * (double)M * (double)N, "tt_dense_stats_kernel");
    int rc = launch(tt_dense_stats_kernel, dim3(blocks), dim3(256), (size_t)DS_LDS_BYTES, st, a);
    if (rc == TTSK_OK && dev_stats)
        rc = sum_partials(a.part, blocks, 4, dev_stats, accumulate, st);
    return rc;
}

int ttsk_tt_dense_stats(const double *dev_L, int64_t M, const double *dev_R, int64_t N, int64_t rho, const double *dev_x,
                        double *dev_out, double *dev_stats, int stream)
{
    return ttsk_tt_dense_stats_ld(dev_L, M, dev_R, N, rho, dev_x, N, dev_out, N, dev_stats, 0, stream);
}

int ttsk_sumsq(const double *dev_x, size_t n, double *dev_out, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(dev_out, "ttsk_sumsq: NULL output");
    TTSK_ARG(dev_x || n == 0, "ttsk_sumsq: NULL array of %zu numbers", n);
    const size_t want = (n + 2047) / 2048;          // eight numbers per thread before the grid wraps
    const unsigned blocks = (unsigned)(want > DS_MAX_BLOCKS ? DS_MAX_BLOCKS : want);
    double *part = nullptr;
    if (blocks) {
        part = (double *)scratch(stream, SCRATCH_MISC, (size_t)blocks * 8);
        if (!part) return TTSK_ERR_HIP;
        ProfBracket prof(st, PROF_EVAL, 2.0 * (double)n, "sumsq_kernel");      // closed before the reduce below
        if (int rc = launch(sumsq_kernel, dim3(blocks), dim3(256), 0, st, dev_x, n, part)) return rc;
    }
    return sum_partials(part, blocks, 1, dev_out, 0, st);
}

}  // extern "C"
