// What the two Psi product kernels (stream_small.h) are launched with, decided on the host: the cover tests, the runs of
// k-blocks, the column chunks and their tile structure, the grid rule, the extents of the buffer descriptors, the proofs
// that every 32-bit byte offset fits, the profiling bracket's name and work -- and stream_small_chunks, the rule by which
// the driver (tt_fused.hip) cuts a long contraction into problems of one launch.  A plan holds the filled kernel-argument
// struct, the instantiation the launcher picks and the launch figures; the launchers (stream_small.hip) only carry it out.
//
// Plain C++: no HIP types, so that the plans are compiled and checked by the host compiler alone
// (tests/test_psi_plan.py) before any kernel reads them.  Pointers are tested for alignment and copied, never dereferenced.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "ttsk.h"
#include "plan_common.h"

namespace ttsk {

// ---- the calls ------------------------------------------------------------------------------------------------------
// C_b (J x A) (+)= S_b W_b for nb problems of one shape
struct StreamSmallArgs {
    int nb, J, K1, A;
    const double *const *S;      // nb operands (J x K1), row stride s_j, columns contiguous
    int64_t s_j;
    const double *const *W;      // nb small operands (K1 x A), row stride w_c
    int64_t w_c;
    double *const *C;            // nb results (J x A), row stride c_j
    int64_t c_j;
    int accumulate;
};

// C (J x A) (+)= sum_b S_b W_b, the nb terms equally spaced
struct StreamSmallSumArgs {
    int nb, J, K1, A;
    const double *S;             // term 0 (J x K1, row stride s_j); term b at S + b * s_b
    int64_t s_j, s_b;
    const double *W;             // term 0 (K1 x A, row stride w_c); term b at W + b * w_b
    int64_t w_c, w_b;
    double *C;
    int64_t c_j;
    int accumulate;
};

// ---- the kernel arguments -------------------------------------------------------------------------------------------
struct StreamSmall {
    const double *S[SK_MAXB];
    const double *W[SK_MAXB];
    double *C[SK_MAXB];
    int nb, wpp;                 // problems, row-tile groups per problem
    int nac, ac;                 // column chunks of A (one workgroup each: disjoint outputs), columns per chunk
    int J, K1, A;
    int64_t s_j, w_c, c_j;       // row strides (elements): S rows, W rows, C rows; columns contiguous
    int64_t s_extent, c_extent;
    int AP;
    int accumulate;
};

struct StreamSmallSum {
    const double *S, *W;         // term 0; term b at + b * s_b / + b * w_b
    double *C;
    int nb, groups;              // terms, row-tile groups (8 tiles each)
    int nac, ac;
    int J, K1, A;
    int64_t s_j, w_c, c_j, s_b, w_b;
    int64_t s_extent, w_extent, c_extent;
    int AP, xcd_map;
    int accumulate;
};

// The (full 16-wide tiles, 4-wide strips) structures of a column chunk that are instantiated, each with runs of 5 and of
// 25 k-blocks: the launch tables of stream_small.hip are written from these lists.
#define PSI_STREAM_STRUCTURES(X) X(1, 0) X(1, 1) X(1, 2) X(2, 0) X(2, 1) X(2, 2) X(3, 0) X(3, 1) X(3, 2) X(4, 0) X(4, 1) X(4, 2) \
    X(5, 0) X(5, 1) X(5, 2) X(6, 0) X(6, 1) X(6, 2) X(7, 0)
#define PSI_STREAM_SUM_STRUCTURES(X) X(1, 0) X(1, 1) X(1, 2) X(2, 0) X(2, 1) X(2, 2) X(3, 0) X(3, 1) X(3, 2)

constexpr size_t PSI_LDS_MAX = 160 * 1024;
constexpr int PSI_SUM_IMAGE_MAX = 512 * 12;      // doubles of one W image of the sum kernel: 12 per thread (its BATCH)
constexpr int64_t PSI_LIM32 = (1ll << 32) - 64;

// ---- the plans ------------------------------------------------------------------------------------------------------
struct PsiLaunch {
    size_t lds;                  // dynamic LDS bytes of a workgroup
    int grid;                    // workgroups (of 512 threads)
    double flops;
    char name[64];               // the profiling bracket's name: the instantiation
};

struct PsiStreamPlan {
    StreamSmall a;
    int nf, str, unr, KB1;       // tiles and strips of a chunk, k-blocks per straight-line run, k-blocks padded to whole runs
    PsiLaunch l;
};

struct PsiStreamSumPlan {
    StreamSmallSum a;
    int nf, str, unr, KB1;
    PsiLaunch l;
};

// k-blocks are issued in straight-line runs of 25 or of 5 and padded to whole runs (the padded ones meet zero rows of
// the W image): 25 when that pads at most one k-block more than 5 does
inline void psi_runs(int K1, int &unr, int &KB1)
{
    const int kb = (K1 + 3) / 4;
    const int pad25 = (kb + 24) / 25 * 25, pad5 = (kb + 4) / 5 * 5;
    unr = pad25 <= pad5 + 1 ? 25 : 5;
    KB1 = unr == 25 ? pad25 : pad5;
}

// A in t chunks: columns per chunk (a multiple of 4) and their tiles + strips (a remainder of 9..15 is a zero-padded full tile)
inline void psi_chunk_split(int A, int t, int &need, int &nf, int &str)
{
    need = (int)((cdiv(A, t) + 3) / 4 * 4);
    nf = need / 16;
    const int rem = need % 16;
    if (rem == 0) str = 0;
    else if (rem <= 4) str = 1;
    else if (rem <= 8) str = 2;
    else { nf += 1; str = 0; }
}

// ---- stream_small_kernel: 1 = covered, 0 = not, < 0 = error ----------------------------------------------------------
inline int psi_stream_plan(const StreamSmallArgs &c, int n_cu, PsiStreamPlan &p)
{
    if (c.nb < 1 || c.nb > SK_MAXB) return 0;
    if (c.K1 < 1 || c.A < 4 || c.J < 1024) return 0;
    if (c.s_j < c.K1 || c.w_c < c.A || c.c_j < c.A) return 0;
    p = PsiStreamPlan{};
    int unr, KB1;
    psi_runs(c.K1, unr, KB1);
    // column chunks: the fewest whose W image fits the LDS and whose structure (<= 7 tiles) is instantiated
    int nac = 0, nf = 0, str = 0, need = 0;
    size_t lds = 0;
    for (int t = 1; t <= 16 && !nac; ++t) {
        psi_chunk_split(c.A, t, need, nf, str);
        if (nf < 1 || nf + (str ? 1 : 0) > 7) continue;
        lds = (size_t)4 * (KB1 + 1) * (16 * nf + 4 * str) * 8;
        if (lds <= PSI_LDS_MAX) nac = t;
    }
    if (!nac) return 0;
    StreamSmall &a = p.a;
    a.nb = c.nb; a.J = c.J; a.K1 = c.K1; a.A = c.A;
    a.nac = nac; a.ac = nac == 1 ? c.A : need;
    a.s_j = c.s_j; a.w_c = c.w_c; a.c_j = c.c_j;
    a.accumulate = c.accumulate;
    a.AP = 16 * nf + 4 * str;
    const int ntiles = (c.J + 15) / 16;
    if (n_cu < 1) return TTSK_ERR_HIP;
    int wpp = n_cu / (c.nb * nac) > 0 ? n_cu / (c.nb * nac) : 1;
    if (wpp > (ntiles + 7) / 8) wpp = (ntiles + 7) / 8;
    a.wpp = wpp;
    a.s_extent = (int64_t)(c.J - 1) * c.s_j + c.K1;
    a.c_extent = (int64_t)(c.J - 1) * c.c_j + c.A;
    // 32-bit byte offsets incl. the look-ahead one visit past the last tile
    if (((int64_t)(ntiles + wpp * 8 + 2) * 16 * c.s_j + 256) * 8 >= PSI_LIM32) return 0;
    if (((int64_t)(ntiles + 1) * 16 * c.c_j + 256) * 8 >= PSI_LIM32) return 0;
    // (W: the launcher this plan replaces had no such test -- the driver's row stride is a DRM rank; a direct caller's may be anything)
    if (((int64_t)c.K1 * c.w_c + 256) * 8 >= PSI_LIM32) return 0;
    for (int b = 0; b < c.nb; ++b) {
        if (((uintptr_t)c.S[b] | (uintptr_t)c.W[b] | (uintptr_t)c.C[b]) & 7) return 0;
        a.S[b] = c.S[b]; a.W[b] = c.W[b]; a.C[b] = c.C[b];
    }
    p.nf = nf; p.str = str; p.unr = unr; p.KB1 = KB1;
    p.l.lds = lds; p.l.grid = c.nb * wpp * nac;
    p.l.flops = 2.0 * c.nb * (double)c.J * c.K1 * c.A;
    snprintf(p.l.name, sizeof(p.l.name), "stream_small_kernel<%d, %d, 5, %d>", nf, str, unr);
    return 1;
}

// the fewest equal chunks (<= max_chunks, SK_MAXB) of whole k-blocks into which a contraction of length K splits so that
// a chunk's W image (A columns) fits the kernel's LDS in one column chunk: the problems of one launch; 0 = none
inline int stream_small_chunks(int64_t K, int64_t A, int max_chunks)
{
    for (int t = 1; t <= max_chunks && t <= SK_MAXB; ++t)
        if (K % t == 0 && (K / t) % 4 == 0 && 4 * (K / t / 4 + 6) * ((A + 3) / 4 * 4) * 8 <= 150 * 1024) return t;
    return 0;
}

// ---- stream_small_sum_kernel: 1 = covered, 0 = not, < 0 = error ------------------------------------------------------
inline int psi_stream_sum_plan(const StreamSmallSumArgs &c, int n_cu, PsiStreamSumPlan &p)
{
    if (c.nb < 2 || c.K1 < 1 || c.A < 8 || c.J < 1024) return 0;
    if (c.s_j < c.K1 || c.w_c < c.A || c.c_j < c.A || c.s_b < 0 || c.w_b < 0) return 0;
    if (((uintptr_t)c.S | (uintptr_t)c.W | (uintptr_t)c.C) & 7) return 0;
    p = PsiStreamSumPlan{};
    int unr, KB1;
    psi_runs(c.K1, unr, KB1);
    const int ntiles = (c.J + 15) / 16, groups = (ntiles + 7) / 8, cus = n_cu;
    if (cus < 1) return TTSK_ERR_HIP;
    // column chunks: at least two (two W images of <= 6144 doubles), as many as fill the chip in one round
    int nac = 0, nf = 0, str = 0, need = 0;
    auto plan = [&](int t, int &nf_, int &str_, int &need_) {
        psi_chunk_split(c.A, t, need_, nf_, str_);
        if (nf_ < 1 || nf_ + (str_ ? 1 : 0) > 4 || (nf_ == 3 && str_ > 2) || nf_ > 3) return false;
        return (size_t)4 * (KB1 + 1) * (16 * nf_ + 4 * str_) <= (size_t)PSI_SUM_IMAGE_MAX;
    };
    for (int t = 2; t <= 16 && !nac; ++t)
        if (plan(t, nf, str, need)) nac = t;
    if (!nac) return 0;
    while (groups * (nac + 1) <= cus + cus / 8 && (c.A + nac) / (nac + 1) >= 16) {
        int nf2, str2, need2;
        if (!plan(nac + 1, nf2, str2, need2)) break;
        ++nac; nf = nf2; str = str2; need = need2;
    }
    // Chunks are `need` columns wide, a multiple of 4: grown past the fewest, the last ones can lie wholly behind A (A = 113
    // in 7 chunks of 20: six cover it).  Such a workgroup staged zeros, streamed all of S and stored nothing; it is not launched.
    nac = (int)cdiv(c.A, need);
    StreamSmallSum &a = p.a;
    a.S = c.S; a.W = c.W; a.C = c.C;
    a.nb = c.nb; a.groups = groups; a.nac = nac; a.ac = need;
    a.J = c.J; a.K1 = c.K1; a.A = c.A;
    a.s_j = c.s_j; a.w_c = c.w_c; a.c_j = c.c_j; a.s_b = c.s_b; a.w_b = c.w_b;
    a.accumulate = c.accumulate;
    a.AP = 16 * nf + 4 * str;
    a.s_extent = (int64_t)(c.nb - 1) * c.s_b + (int64_t)(c.J - 1) * c.s_j + c.K1;
    a.w_extent = (int64_t)(c.nb - 1) * c.w_b + (int64_t)(c.K1 - 1) * c.w_c + c.A;
    a.c_extent = (int64_t)(c.J - 1) * c.c_j + c.A;
    // 32-bit byte offsets incl. the prefetch into the term behind the last one
    if (((int64_t)c.nb * c.s_b + (int64_t)(ntiles + 1) * 16 * c.s_j + 4 * KB1 + 256) * 8 >= PSI_LIM32) return 0;
    if (((int64_t)c.nb * c.w_b + (int64_t)c.K1 * c.w_c + 256) * 8 >= PSI_LIM32) return 0;
    if (((int64_t)(ntiles + 1) * 16 * c.c_j + 256) * 8 >= PSI_LIM32) return 0;
    const int units = groups * nac;
    a.xcd_map = units % 8 == 0 ? 1 : 0;
    p.nf = nf; p.str = str; p.unr = unr; p.KB1 = KB1;
    p.l.lds = (size_t)2 * 4 * (KB1 + 1) * a.AP * 8;
    p.l.grid = units;
    p.l.flops = 2.0 * c.nb * (double)c.J * c.K1 * c.A;
    snprintf(p.l.name, sizeof(p.l.name), "stream_small_sum_kernel<%d, %d, 5, %d>", nf, str, unr);
    return 1;
}

}  // namespace ttsk
