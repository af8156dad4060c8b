// What the operator-times-train pass (op_apply.hip) is launched with, decided on the host: the argument checks and the
// cover of ttsk_op_apply, the kernel-argument table of its terms, each term's share of the grid, the LDS of a workgroup
// and the flops of the call.
//
// Plain C++: no HIP types, so that the plan is compiled and checked by the host compiler alone
// (tests/test_operator_product_host.py) before any kernel reads it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "ttsk.h"
#include "plan_common.h"

namespace ttsk {

constexpr int OP_MAX_TERMS = 24;                 // terms of one call: the table below travels as the kernel's argument (4 KB at most)
constexpr int OP_KC = 32;                        // (beta, j) rows of T1 held in LDS at once
constexpr int OP_COL_TILES = 8;                  // 16-column tiles of (i, beta') a workgroup accumulates: 16 l x 8 = 128 tiles
constexpr int OP_COLS = 16 * OP_COL_TILES;
// one (beta, j) row of T1 is a 16 x 16 tile; rows 16 doubles apart modulo 32, so that the two rows a half-wave's
// ds_read_b64 touches (32 lanes x 2 dwords) fall on 64 different banks
constexpr int OP_PITCH = 16 * 16 + 16;
constexpr size_t OP_LDS = ((size_t)OP_KC * OP_PITCH + OP_KC) * 8;      // T1 rows, then the operator-row offset of each

// one term as the kernel sees it
struct OpTerm {
    const double *L, *M, *C;     // M of a plain-train term: any readable address (never used), strides 0
    int64_t sM[4];               // element strides of M over (beta, j, i, beta')
    int64_t sC[3];               // of C over (a, j, a')
    int64_t w_off;
    int R, R1, r, r1, n_in;
    int plain;
    int block0;                  // first workgroup of the term; its workgroups are (l tile, a' tile, column block), the last fastest
    int atiles, cblocks;
};

struct OpApplyArgs {
    OpTerm t[OP_MAX_TERMS];
    double *W;
    int64_t w_cols;
    int K, l, n_out;
};

struct OpPlan {
    OpApplyArgs a;
    int64_t blocks;              // workgroups of the launch
    double flops;                // sum over the terms of 2 l (R r n_in r' + R n_in n_out R' r')
    char msg[200];               // why not, when the status is not TTSK_OK
};

// dims: K x 7 (R, R', r, r', n_in, n_out, w_off); strides: K x 7 in elements, M (beta, j, i, beta') then C (a, j, a')
inline int op_apply_plan(int K, const double *const *L, const double *const *M, const double *const *C, const int64_t *dims,
                         const int64_t *strides, int64_t l, double *W, int64_t w_cols, OpPlan *p)
{
    *p = OpPlan{};
    if (!L || !M || !C || !dims || !strides || !W) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_apply: NULL argument");
    if (K < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_apply: K = %d terms", K);
    if (l < 1 || w_cols < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_apply: l = %lld, w_cols = %lld must be positive", (long long)l, (long long)w_cols);
    bool wide = l > PLAN_MAX_EXTENT || w_cols > PLAN_MAX_EXTENT;
    for (int t = 0; t < K; ++t) {
        const int64_t *d = dims + 7 * t;
        if (!L[t] || !C[t]) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_apply: term %d: NULL chain or train core", t);
        for (int i = 0; i < 6; ++i)
            if (d[i] < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_apply: term %d: extent %d is %lld", t, i, (long long)d[i]);
        if (d[6] < 0) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_apply: term %d: column offset %lld", t, (long long)d[6]);
        if (!M[t] && (d[0] != 1 || d[1] != 1 || d[4] != d[5]))
            PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_apply: term %d has no operator: R = %lld, R' = %lld must be 1 and n_in = %lld equal n_out = %lld", t,
                      (long long)d[0], (long long)d[1], (long long)d[4], (long long)d[5]);
        if (d[5] != dims[5]) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_apply: term %d: n_out = %lld, term 0 has %lld", t, (long long)d[5], (long long)dims[5]);
        for (int i = 0; i < 7; ++i)
            if (d[i] > PLAN_MAX_EXTENT) wide = true;
        if (wide) continue;
        if (d[6] + d[1] * d[3] > w_cols)
            PLAN_FAIL(TTSK_ERR_ARG, "ttsk_op_apply: term %d: columns %lld + %lld x %lld pass w_cols = %lld", t, (long long)d[6], (long long)d[1],
                      (long long)d[3], (long long)w_cols);
    }
    // ---- the cover
    if (wide) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_op_apply: an extent of 2^31 or more; below 2^31 is covered");
    if (K > OP_MAX_TERMS) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_op_apply: %d terms in one call, up to %d are covered", K, OP_MAX_TERMS);
    OpApplyArgs &a = p->a;
    a.W = W; a.w_cols = w_cols; a.K = K; a.l = (int)l; a.n_out = (int)dims[5];
    const int64_t ltiles = (l + 15) / 16;
    for (int t = 0; t < K; ++t) {
        const int64_t *d = dims + 7 * t, *s = strides + 7 * t;
        if (d[0] * d[4] > PLAN_MAX_EXTENT || d[5] * d[1] > PLAN_MAX_EXTENT)
            PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_op_apply: term %d: R n_in = %lld or n_out R' = %lld; below 2^31 is covered", t,
                      (long long)(d[0] * d[4]), (long long)(d[5] * d[1]));
        OpTerm &T = a.t[t];
        T.L = L[t]; T.C = C[t];
        T.plain = M[t] ? 0 : 1;
        T.M = M[t] ? M[t] : L[t];
        for (int i = 0; i < 4; ++i) T.sM[i] = M[t] ? s[i] : 0;
        for (int i = 0; i < 3; ++i) T.sC[i] = s[4 + i];
        T.R = (int)d[0]; T.R1 = (int)d[1]; T.r = (int)d[2]; T.r1 = (int)d[3]; T.n_in = (int)d[4];
        T.w_off = d[6];
        T.atiles = (int)((d[3] + 15) / 16);
        T.cblocks = (int)((d[5] * d[1] + OP_COLS - 1) / OP_COLS);
        if (p->blocks > PLAN_MAX_EXTENT) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_op_apply: more than 2^31 workgroups");
        T.block0 = (int)p->blocks;
        const int64_t tiles = ltiles * T.atiles;                 // below 2^56
        if (tiles > PLAN_MAX_EXTENT) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_op_apply: more than 2^31 workgroups");
        p->blocks += tiles * T.cblocks;
        p->flops += 2.0 * (double)l * ((double)d[0] * d[2] * d[4] * d[3] + (double)d[0] * d[4] * d[5] * d[1] * d[3]);
    }
    if (p->blocks > PLAN_MAX_EXTENT) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_op_apply: more than 2^31 workgroups");
    return TTSK_OK;
}

}  // namespace ttsk
