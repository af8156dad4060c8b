// What the Gram pass of tensor trains (tt_gram.hip) is launched with, decided on the host: per mode the chunks of the
// n_k slices a pair is cut into, the body (matrix instruction or vector FMA), the LDS stage (slices and 16-column tiles of
// T held at once, row pitch of acc), the slab of chunk partials in the scratch block; and the number of launches.
//
// Plain C++: no HIP types, so that the plan is compiled and checked by the host compiler alone
// (tests/test_tt_gram_plan.py) before any kernel reads it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "ttsk.h"
#include "plan_common.h"

namespace ttsk {

constexpr int GRAM_MAX_MODES = 32;
constexpr int GRAM_MAX_RANK = 128;               // acc (128 x 128) and one 16-column tile of T just fill the LDS of a CU
constexpr int GRAM_MAX_TRAINS = 128;             // K + M: the mode's view of every train travels as a kernel argument
constexpr int GRAM_MAX_CHUNKS = 64;              // bounds the fused reduce: a workgroup reads chunks x ra x rb partials
constexpr int GRAM_MAX_STAGE_TILES = 4;          // 16-column tiles of T per LDS stage (slices x tiles of a')
constexpr int GRAM_FMA_CELLS = 2048;             // FMA body: a thread keeps 8 of the ra' x rb' sums of its pair
constexpr size_t GRAM_LDS_BUDGET = 156 * 1024;   // of the 160 KB of a CU

enum { GRAM_BODY_FMA = 0, GRAM_BODY_MFMA = 1 };

struct GramModePlan {
    int chunks;                  // per pair, 1 <= chunks <= n_k
    int body;
    int S, TA;                   // slices per stage; 16-column tiles of a' per stage (FMA body: TA = 0, all of a')
    int pitch;                   // row pitch of acc in LDS (doubles)
    int acc_rows, t_rows;        // rows of acc and of one T tile as laid out (padded for the MFMA body)
    size_t acc_doubles, t_doubles;
    size_t lds;                  // dynamic LDS bytes of a workgroup
    size_t slab_off, slab_bytes; // chunk partials of this mode: [pair][chunk][ra' x rb'], ragged over the pairs
    int ra, rb, ra1, rb1;        // widest ranks of the mode over the trains of each side: (r_k, r_{k+1})
    int64_t sum_a1, sum_b1;      // sums of r_{k+1} over the trains of each side
};

struct GramPlan {
    int d, K, M;
    int64_t pairs;
    GramModePlan m[GRAM_MAX_MODES];
    int fold_last;               // the last mode has one chunk: it writes G itself
    int launches;                // d + 1 - fold_last
    size_t scratch;              // bytes
    char msg[160];               // why not, when the status is not TTSK_OK
};

inline int gram_round(int x, int m) { return (x + m - 1) / m * m; }

// LDS of one stage (doubles): acc, then T
inline void gram_lds(GramModePlan &m, bool pad)
{
    if (m.body == GRAM_BODY_MFMA) {
        const int rbp = gram_round(m.rb, 16);
        // the two k rows of a half-wave's fragment read lie 16 doubles apart modulo 32: conflict-free
        m.pitch = pad && rbp % 32 == 0 ? rbp + 16 : rbp;
        m.acc_rows = gram_round(m.ra, 4);
        m.t_rows = rbp;
        m.t_doubles = (size_t)m.S * m.TA * m.t_rows * 16;
    } else {
        m.pitch = m.rb;
        m.acc_rows = m.ra;
        m.t_rows = m.rb;
        m.t_doubles = (size_t)m.S * m.rb * m.ra1;
    }
    m.acc_doubles = (size_t)m.acc_rows * m.pitch;
    m.lds = (m.acc_doubles + m.t_doubles) * 8;
}

// ranks_a: K rows of d + 1 ranks, ranks_b: M rows
inline int gram_plan(const int64_t *ranks_a, const int64_t *ranks_b, const int64_t *shape, int d, int K, int M, int n_cu, GramPlan *p)
{
    *p = GramPlan{};
    if (!ranks_a || !ranks_b || !shape) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_tt_gram: NULL rank table or shape");
    if (d < 1 || K < 1 || M < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_tt_gram: d = %d, K = %d, M = %d must be positive", d, K, M);
    if (d > GRAM_MAX_MODES) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_tt_gram: %d modes, at most %d are covered", d, GRAM_MAX_MODES);
    for (int side = 0; side < 2; ++side) {
        const int64_t *rk = side ? ranks_b : ranks_a;
        for (int t = 0; t < (side ? M : K); ++t, rk += d + 1) {
            if (rk[0] != 1 || rk[d] != 1)
                PLAN_FAIL(TTSK_ERR_ARG, "ttsk_tt_gram: boundary ranks (%lld, %lld) of train %d of side %d are not 1", (long long)rk[0],
                          (long long)rk[d], t, side);
            for (int k = 0; k <= d; ++k)
                if (rk[k] < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_tt_gram: rank %d of train %d of side %d is %lld", k, t, side, (long long)rk[k]);
        }
    }
    for (int k = 0; k < d; ++k)
        if (shape[k] < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_tt_gram: mode %d has size %lld", k, (long long)shape[k]);
    // ---- the cover
    for (int k = 0; k < d; ++k)
        if (shape[k] >= (1ll << 31)) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_tt_gram: mode %d of size %lld, below 2^31 is covered", k, (long long)shape[k]);
    for (int side = 0; side < 2; ++side) {
        const int64_t *rk = side ? ranks_b : ranks_a;
        for (int i = 0; i < (side ? M : K) * (d + 1); ++i)
            if (rk[i] > GRAM_MAX_RANK) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_tt_gram: rank %lld, up to %d is covered", (long long)rk[i], GRAM_MAX_RANK);
    }
    if (K + M > GRAM_MAX_TRAINS) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_tt_gram: %d trains in one call, up to %d are covered", K + M, GRAM_MAX_TRAINS);
    p->d = d; p->K = K; p->M = M;
    p->pairs = (int64_t)K * M;
    if (n_cu < 1) n_cu = 1;
    size_t widest[2] = {0, 0};                       // slabs alternate between two halves of the scratch block
    for (int k = 0; k < d; ++k) {
        GramModePlan &m = p->m[k];
        for (int t = 0; t < K; ++t) {
            const int r0 = (int)ranks_a[t * (d + 1) + k], r1 = (int)ranks_a[t * (d + 1) + k + 1];
            if (r0 > m.ra) m.ra = r0;
            if (r1 > m.ra1) m.ra1 = r1;
            m.sum_a1 += r1;
        }
        for (int t = 0; t < M; ++t) {
            const int r0 = (int)ranks_b[t * (d + 1) + k], r1 = (int)ranks_b[t * (d + 1) + k + 1];
            if (r0 > m.rb) m.rb = r0;
            if (r1 > m.rb1) m.rb1 = r1;
            m.sum_b1 += r1;
        }
        // pairs x chunks fills the chip once
        int64_t c = (n_cu + p->pairs - 1) / p->pairs;
        if (c > GRAM_MAX_CHUNKS) c = GRAM_MAX_CHUNKS;
        if (c > shape[k]) c = shape[k];
        m.chunks = c < 1 ? 1 : (int)c;
        const int64_t slices = (shape[k] + m.chunks - 1) / m.chunks;      // the longest run of a chunk
        // the matrix instruction where both extents of a product's tile reach 16: T is (rb x ra'), part (ra' x rb')
        m.body = m.ra1 >= 16 && (m.rb >= 16 || m.rb1 >= 16) ? GRAM_BODY_MFMA : GRAM_BODY_FMA;
        if (m.body == GRAM_BODY_MFMA) {
            const int nat = (m.ra1 + 15) / 16;
            m.TA = nat < GRAM_MAX_STAGE_TILES ? nat : GRAM_MAX_STAGE_TILES;
            m.S = GRAM_MAX_STAGE_TILES / m.TA;
        } else {
            m.TA = 0;
            m.S = 4;
        }
        if (m.S > slices) m.S = (int)slices;
        bool pad = true;
        for (gram_lds(m, pad); m.lds > GRAM_LDS_BUDGET; gram_lds(m, pad)) {
            if (m.S > 1) --m.S;
            else if (m.TA > 1) --m.TA;
            else if (pad) pad = false;
            else PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_tt_gram: mode %d: acc (%d x %d) and one tile of T do not fit the LDS", k, m.ra, m.rb);
        }
        if (m.body == GRAM_BODY_FMA && (int64_t)m.ra1 * m.rb1 > GRAM_FMA_CELLS)
            PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_tt_gram: mode %d: %d x %d sums on the FMA body", k, m.ra1, m.rb1);
        m.slab_bytes = (size_t)m.chunks * (size_t)m.sum_a1 * (size_t)m.sum_b1 * 8;
        if (m.slab_bytes > widest[k & 1]) widest[k & 1] = m.slab_bytes;
    }
    widest[0] = (widest[0] + 255) & ~(size_t)255;
    for (int k = 0; k < d; ++k) p->m[k].slab_off = k & 1 ? widest[0] : 0;
    p->scratch = widest[0] + widest[1] + 256;
    p->fold_last = p->m[d - 1].chunks == 1;
    p->launches = d + 1 - p->fold_last;
    return TTSK_OK;
}

}  // namespace ttsk
