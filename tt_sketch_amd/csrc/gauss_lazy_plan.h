// What the two lazy-Gaussian products (gauss_lazy.hip) are launched with, decided on the host.  Both are the same GEMM
//   D[m, n] = sum_k G[lo + m, k] X[k, n],   m < w = hi - lo,  k < K = cols,  n < N,
// whose G operand is sampled on the chip (sampler_dev.h) and never stored:
//   ttsk_gauss_lazy_left   X = Xu (K x N row-major, leading dimension ldx), D = Z (w x N, ldz)
//   ttsk_gauss_lazy_right  X = S^T (S is N x K row-major, lds),             D = Out^T (Out is N x w, ldo)
// A workgroup owns GL_NT columns n and one chunk of k; it walks the chunk GL_KB values of k at a time, and every step's
// (w x GL_KB) tile of samples serves all GL_NT columns.  Few column tiles: k is cut into chunks of a multiple of GL_KCH, the
// partial products go to a workspace (chunk, m, n) and a closing launch sums them in ascending chunk order.
//
// Plain C++: no HIP types, so that the plans are compiled and checked by the host compiler alone
// (tests/test_gauss_lazy_plan.py) before any kernel reads them.  Pointers are tested for NULL, never dereferenced.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "ttsk.h"
#include "plan_common.h"

namespace ttsk {

constexpr int GL_THREADS = 256;                  // four waves, each GL_NT / 4 columns
constexpr int GL_W_MAX = 64;                     // rows of G per call: up to four 16-row MFMA tiles
constexpr int GL_KB = 16;                        // k per step: four v_mfma_f64_16x16x4
constexpr int GL_NT = 256;                       // columns of a workgroup: four 16-column tiles per wave
constexpr int GL_GP = 80;                        // pitch of the sample tile Gs[k][m] in doubles: 16 modulo 32
constexpr int GL_XP = 272;                       // pitch of Xs[k][n] (left: n is contiguous in memory): 16 modulo 32
constexpr int GL_XPK = 17;                       // pitch of Xs[n][k] (right: k is contiguous in memory): odd
constexpr int64_t GL_KCH = 256;                  // a chunk of k is a multiple of this
constexpr int64_t GL_SPLIT_TILES = 256;          // from this many column tiles on, k is not split
constexpr int64_t GL_WG_TARGET = 512;            // workgroups a split aims at; also bounds gridDim.y
constexpr int64_t GL_CLOSE_BLOCKS_MAX = 4096;    // closing launch: one thread per element up to this, then a grid stride
constexpr size_t GL_LDS_LIMIT = 64 * 1024;       // static LDS of a kernel

enum { GL_LEFT = 0, GL_RIGHT = 1 };
enum { GL_NOTHING = 0, GL_DIRECT = 1, GL_SPLIT = 2 };

struct GlPlan {
    int side;                    // GL_LEFT / GL_RIGHT: which of Xs' two layouts the kernel takes
    int branch;                  // GL_NOTHING: no launch; GL_DIRECT: one launch into D; GL_SPLIT: partials, then the closing launch
    int w, mt;                   // rows of G, and 16-row tiles of them (the kernel's instance)
    int64_t K, N;
    int64_t tiles;               // column tiles: gridDim.x
    int64_t chunk, nchunks;      // k per workgroup, chunks: gridDim.y
    int64_t ws_elems;            // doubles of workspace: nchunks * w * N (split), 0 (direct)
    int64_t close_blocks;        // workgroups of the closing launch (split)
    size_t lds;                  // static LDS of the kernel in bytes
    double samples;              // Gaussian samples evaluated: tiles * w * K, once per (column tile, k)
    double flops;                // 2 w K N
    double bytes;                // X once, D once, the workspace written and read
    char msg[200];               // why not, when the status is not TTSK_OK
};

inline size_t gl_lds_bytes()
{
    const size_t xs = (size_t)(GL_KB * GL_XP > GL_NT * GL_XPK ? GL_KB * GL_XP : GL_NT * GL_XPK);
    return (size_t)GL_KB * GL_GP * 8 + xs * 8 + (size_t)GL_KB * GL_GP * 2 + 4;      // Gs, Xs, the tail queue, its length
}

// x: the operand read (K x N for left, N x K for right), ldx its leading dimension; d: the product, ldd its leading dimension
inline int gauss_lazy_plan(int side, int64_t row_lo, int64_t row_hi, int64_t cols, const double *x, int64_t N, int64_t ldx,
                           const double *d, int64_t ldd, GlPlan *p)
{
    *p = GlPlan{};
    const char *who = side == GL_LEFT ? "ttsk_gauss_lazy_left" : "ttsk_gauss_lazy_right";
    p->side = side;
    if (row_lo < 0 || row_hi < row_lo || cols < 1 || N < 0)
        PLAN_FAIL(TTSK_ERR_ARG, "%s: rows [%lld, %lld) of %lld columns against an extent of %lld", who, (long long)row_lo, (long long)row_hi,
                  (long long)cols, (long long)N);
    if (row_hi - row_lo > GL_W_MAX)
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "%s: %lld rows of G, up to %d are covered", who, (long long)(row_hi - row_lo), GL_W_MAX);
    if (cols > PLAN_MAX_EXTENT || N > PLAN_MAX_EXTENT)
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "%s: extents %lld and %lld, below 2^31 are covered", who, (long long)cols, (long long)N);
    if ((unsigned __int128)row_hi * (unsigned __int128)cols > ((unsigned __int128)1 << 63))
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "%s: the flat index of row %lld and %lld columns passes 2^63", who, (long long)(row_hi - 1), (long long)cols);
    const int w = (int)(row_hi - row_lo);
    p->w = w; p->mt = (w + 15) / 16; p->K = cols; p->N = N;
    if (w == 0 || N == 0) return TTSK_OK;
    if (!x || !d) PLAN_FAIL(TTSK_ERR_ARG, "%s: NULL operand or output", who);
    const int64_t x_min = side == GL_LEFT ? N : cols, d_min = side == GL_LEFT ? N : w;
    if (ldx < x_min || ldd < d_min || ldx > PLAN_MAX_EXTENT || ldd > PLAN_MAX_EXTENT)
        PLAN_FAIL(TTSK_ERR_ARG, "%s: leading dimensions %lld and %lld, at least %lld and %lld (and below 2^31) are needed", who, (long long)ldx,
                  (long long)ldd, (long long)x_min, (long long)d_min);
    p->tiles = cdiv(N, GL_NT);
    if (p->tiles >= GL_SPLIT_TILES || cols <= GL_KCH) {
        p->branch = GL_DIRECT;
        p->chunk = cols;
        p->nchunks = 1;
    } else {
        const int64_t most = cdiv(GL_WG_TARGET, p->tiles);                  // chunks at most: >= 2 here
        p->chunk = GL_KCH * cdiv(cdiv(cols, GL_KCH), most);
        p->nchunks = cdiv(cols, p->chunk);
        p->branch = p->nchunks > 1 ? GL_SPLIT : GL_DIRECT;
    }
    if (p->branch == GL_SPLIT) {
        p->ws_elems = p->nchunks * w * N;
        p->close_blocks = cdiv((int64_t)w * N, GL_THREADS);
        if (p->close_blocks > GL_CLOSE_BLOCKS_MAX) p->close_blocks = GL_CLOSE_BLOCKS_MAX;
    }
    p->lds = gl_lds_bytes();
    p->samples = (double)p->tiles * w * (double)cols;
    p->flops = 2.0 * w * (double)cols * (double)N;
    p->bytes = 8.0 * ((double)cols * (double)N + (double)w * (double)N + 2.0 * (double)p->ws_elems);
    return TTSK_OK;
}

}  // namespace ttsk
