// ttsk_tt_assemble_batch: assemble_sketched_tt (reference sketch.py:400-443) for `count` streaming sketches of one
// signature at once -- the second half of stream_sketch_batch(...) + to_tt().  Per tensor the contract of
// ttsk_tt_assemble; per Omega shape the launches are a fixed handful whatever the batch size:
//
//   1. gram:   every Omega_{b,k} copied into one contiguous staging buffer and its Gram matrix formed (one launch);
//   2. chol:   the batched Cholesky inverse of all Gram matrices (cholesky.hip's chol_inv_kernel, one launch);
//   3. solve:  X = Omega^T G^-1 (l <= r) or G^-1 Omega^T, the normal-equations pseudo-inverse (one launch);
//   4. jacobi: jacobi.hip's one-sided Jacobi pseudo-inverse, a workgroup per matrix, each predicated on its own Cholesky
//      verdict (one launch; it leaves at once where the attempt was accepted): a rank-deficient or ill-conditioned Omega
//      takes the robust path on the device, alone, without a read-back -- ttsk_pinv_batch's numerics, no 32-matrix limit;
//   5. apply:  the fused refined product below (one launch per 16 groups of equally spaced pairs).
//
// Fused apply (assemble_apply_kernel), per pair (P = pinv(Omega), Psi) and per row tile of the unfolding:
//     C = Psi P;   R = Psi - C Omega;   C += R P           ("right": Psi_k unfolded (l_{k-1} n_k) x r, C (.) x l)
// The three products are row-local: a TM-row tile of Psi gives its TM rows of C from P and Omega alone.  The "left"
// direction, C = P Psi_mat, is the same computation on the transposes (Psi_mat^T tiles of TM columns, P^T, Omega^T).
// The residual form is kept on purpose: the accuracy comes from computing Psi - C Omega explicitly.
// A workgroup (4 waves) holds P' (a x b) and Omega' (b x a) in LDS for its pair and sweeps its share of the row tiles:
// each Psi tile is read from HBM once (into LDS), C of the first product stays in MFMA accumulators through the
// refinement, R overwrites the tile in LDS, C is written once.  fp64 MFMA 16x16x4 throughout.
//   a = columns of the Psi tile (right: r, left: l), b = columns of C (right: l, left: r).
//   Cover: min(l, r) <= 56 and max(l, r) <= 112 (LDS: P', Omega', Psi tile, C tile <= 150 KB), any row / column count:
//   C3 (l = 50, r = 100, n = 200) and the ref150 shape (l = 55, r = 110), both directions.  Outside it the pairs go
//   through ttsk_pinv_begin / _end and ttsk_gemm one by one, with the same three products.
#include <algorithm>
#include <map>
#include <utility>
#include <vector>
#include "common.h"
#include "linalg_int.h"
#include "assemble_batch_plan.h"

using namespace ttsk;

namespace {

// AB_TM, AB_THREADS, AB_MAXG, AB_TILES_PER_WG and the cover: assemble_batch_plan.h, with every launch decision below

// one mode of `count` tensors whose operands are equally spaced (base + tensor * stride)
struct AbGroup {
    const double *psi, *om, *pin;    // Psi, Omega (Gram stage: the caller's; apply: staging or caller's), P source
    double *pout, *c;                // copy of P to the caller's work (nullptr: none), C
    int64_t s_psi, s_om, s_pin, s_pout, s_c;
    int64_t m;                       // rows of the unfolding (right) / columns of Psi_mat (left)
    int count, chunks, first;        // tensors, workgroups per tensor, first workgroup (apply) or pair index (pinv stages)
};
struct AbTable {
    AbGroup g[AB_MAXG];
    int ng;
};

__device__ __forceinline__ int find_group(const AbTable &t, int wg)
{
    int gi = 0;
    while (gi + 1 < t.ng && wg >= t.g[gi + 1].first) ++gi;
    return gi;
}

__device__ __forceinline__ int up4(int x) { return (x + 3) & ~3; }
__device__ __forceinline__ int up16(int x) { return (x + 15) & ~15; }

template <bool LEFT>
__global__ __launch_bounds__(AB_THREADS) void assemble_apply_kernel(AbTable t, int a, int b)
{
    extern __shared__ double sm[];
    const int wg = blockIdx.x, tid = threadIdx.x;
    const AbGroup &G = t.g[find_group(t, wg)];
    const int local = wg - G.first, tb = local / G.chunks, ch = local % G.chunks;
    const double *psi = G.psi + tb * G.s_psi, *Om = G.om + tb * G.s_om, *P = G.pin + tb * G.s_pin;
    double *C = G.c + tb * G.s_c;
    const int64_t m = G.m;
    const int a4 = up4(a), a16 = up16(a), b4 = up4(b), b16 = up16(b);
    const int ldx = a16 + 2, ldc = b16 + 2;          // row strides = 2 mod 4 doubles: the A-fragment reads are conflict-free
    double *sP = sm;                                  // P'     a4 x b16
    double *sO = sP + a4 * b16;                       // Omega' b4 x a16
    double *sX = sO + b4 * a16;                       // Psi tile, then R: TM x ldx
    double *sC = sX + AB_TM * ldx;                    // C tile: TM x ldc
    // P (r x l) and Omega (l x r), row-major; right: P' = P, Omega' = Omega; left: their transposes.  Zero padding.
#pragma unroll 8
    for (int e = tid; e < a4 * b16; e += AB_THREADS) {
        const int i = e / b16, j = e % b16;
        sP[e] = (i < a && j < b) ? (LEFT ? P[(int64_t)j * a + i] : P[(int64_t)i * b + j]) : 0.0;
    }
#pragma unroll 8
    for (int e = tid; e < b4 * a16; e += AB_THREADS) {
        const int i = e / a16, j = e % a16;
        sO[e] = (i < b && j < a) ? (LEFT ? Om[(int64_t)j * b + i] : Om[(int64_t)i * a + j]) : 0.0;
    }
    if (G.pout && ch == 0) {
        double *Po = G.pout + tb * G.s_pout;
        for (int e = tid; e < a * b; e += AB_THREADS) Po[e] = P[e];
    }
    const int lane = tid & 63, w = tid >> 6, rb = w & 1, cb0 = w >> 1, lr = lane & 15, lk = lane >> 4;
    const int nbc = b16 / 16, nba = a16 / 16;         // column blocks of C (<= 7) and of R (<= 7): wave w takes cb0 + 2 j
    const int64_t ntiles = (m + AB_TM - 1) / AB_TM;
    // The Psi tile goes through registers: the next tile's loads are issued before the current tile's products, so that
    // their latency hides behind them (one workgroup per CU: nothing else would).  Element q of a thread: e = tid + 256 q.
    constexpr int NPRE = AB_TM * AB_COVER_MAX / AB_THREADS;
    double pre[NPRE];
    auto fetch = [&](int64_t tile) {
        const int64_t row0 = tile * AB_TM;
        const int rows = (int)std::min<int64_t>(AB_TM, m - row0);
#pragma unroll
        for (int q = 0; q < NPRE; ++q) {
            const int e = tid + AB_THREADS * q;
            int i, c;
            if (!LEFT) { i = e / a16; c = e % a16; } else { c = e / AB_TM; i = e % AB_TM; }
            pre[q] = (e < AB_TM * a16 && i < rows && c < a) ? (LEFT ? psi[(int64_t)c * m + row0 + i] : psi[(row0 + i) * a + c]) : 0.0;
        }
    };
    if (ch < ntiles) fetch(ch);
    for (int64_t tile = ch; tile < ntiles; tile += G.chunks) {
        const int64_t row0 = tile * AB_TM;
        const int rows = (int)std::min<int64_t>(AB_TM, m - row0);
        // ---- Psi tile -> sX (zero beyond the rows and the a columns)
#pragma unroll
        for (int q = 0; q < NPRE; ++q) {
            const int e = tid + AB_THREADS * q;
            if (e < AB_TM * a16) {
                int i, c;
                if (!LEFT) { i = e / a16; c = e % a16; } else { c = e / AB_TM; i = e % AB_TM; }
                sX[i * ldx + c] = pre[q];
            }
        }
        __syncthreads();
        if (tile + G.chunks < ntiles) fetch(tile + G.chunks);
        // ---- C = X P'
        v4d acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = v4d{0.0, 0.0, 0.0, 0.0};
        const double *xa = sX + (rb * 16 + lr) * ldx + lk;
#pragma unroll 5
        for (int k = 0; k < a4; k += 4) {
            const double av = xa[k];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cb = cb0 + 2 * j;
                if (cb < nbc) acc[j] = mfma16(av, sP[(k + lk) * b16 + cb * 16 + lr], acc[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cb = cb0 + 2 * j;
            if (cb < nbc)
#pragma unroll
                for (int q = 0; q < 4; ++q) sC[(rb * 16 + lk + 4 * q) * ldc + cb * 16 + lr] = acc[j][q];
        }
        __syncthreads();
        // ---- R = X - C Omega'
        v4d racc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cb = cb0 + 2 * j;
#pragma unroll
            for (int q = 0; q < 4; ++q) racc[j][q] = cb < nba ? sX[(rb * 16 + lk + 4 * q) * ldx + cb * 16 + lr] : 0.0;
        }
        const double *ca = sC + (rb * 16 + lr) * ldc + lk;
#pragma unroll 5
        for (int k = 0; k < b4; k += 4) {
            const double av = -ca[k];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cb = cb0 + 2 * j;
                if (cb < nba) racc[j] = mfma16(av, sO[(k + lk) * a16 + cb * 16 + lr], racc[j]);
            }
        }
        __syncthreads();                                   // every read of X and C done: R replaces X
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cb = cb0 + 2 * j;
            if (cb < nba)
#pragma unroll
                for (int q = 0; q < 4; ++q) sX[(rb * 16 + lk + 4 * q) * ldx + cb * 16 + lr] = racc[j][q];
        }
        __syncthreads();
        // ---- C += R P'
#pragma unroll 5
        for (int k = 0; k < a4; k += 4) {
            const double av = xa[k];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cb = cb0 + 2 * j;
                if (cb < nbc) acc[j] = mfma16(av, sP[(k + lk) * b16 + cb * 16 + lr], acc[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int cb = cb0 + 2 * j;
            if (cb < nbc)
#pragma unroll
                for (int q = 0; q < 4; ++q) sC[(rb * 16 + lk + 4 * q) * ldc + cb * 16 + lr] = acc[j][q];
        }
        __syncthreads();
        // ---- C tile -> HBM, coalesced along memory order
        if (!LEFT) {
            for (int e = tid; e < rows * b; e += AB_THREADS) {
                const int i = e / b, j = e % b;
                C[(row0 + i) * b + j] = sC[i * ldc + j];
            }
        } else {
            for (int e = tid; e < AB_TM * b; e += AB_THREADS) {
                const int j = e / AB_TM, i = e % AB_TM;
                if (i < rows) C[(int64_t)j * m + row0 + i] = sC[i * ldc + j];
            }
        }
        // (the next tile's load writes sX only, read last before the barrier above; sC is written again after a barrier)
    }
}

// Gram stage: workgroup = pair (group, tensor); Omega (l x r) -> staging Os[pair] and G[pair] (n x n, n = min(l, r)):
// W (K x n, K = max(l, r)) is Omega^T (l <= r) or Omega, G = W^T W
__global__ __launch_bounds__(AB_THREADS) void assemble_gram_kernel(AbTable t, int l, int r, double *Os, double *Gm)
{
    extern __shared__ double sm[];
    const int wg = blockIdx.x, tid = threadIdx.x;
    const AbGroup &Gp = t.g[find_group(t, wg)];
    const int tb = wg - Gp.first, pair = Gp.first + tb;     // chunks = 1: `first` is the pair index of the group's first tensor
    const double *Om = Gp.om + tb * Gp.s_om;
    const int n = l <= r ? l : r, K = l <= r ? r : l;
    double *os = Os + (int64_t)pair * l * r, *g = Gm + (int64_t)pair * n * n;
    for (int e = tid; e < l * r; e += AB_THREADS) {
        const double v = Om[e];
        os[e] = v;
        const int i = e / r, j = e % r;
        if (l <= r) sm[j * n + i] = v; else sm[i * n + j] = v;
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += AB_THREADS) {
        const int p = e / n, q = e % n;
        double s = 0.0;
        for (int c = 0; c < K; ++c) s = fma(sm[c * n + p], sm[c * n + q], s);
        g[e] = s;
    }
}

// Solve stage: Y = W G^-1 (K x n); X = Y (l <= r: Omega^T G^-1, r x l) or Y^T (G^-1 Omega^T, r x l) -> Ps[pair]
__global__ __launch_bounds__(AB_THREADS) void assemble_solve_kernel(int l, int r, const double *Os, const double *Ginv, double *Ps)
{
    extern __shared__ double sm[];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int n = l <= r ? l : r, K = l <= r ? r : l;
    const double *os = Os + (int64_t)pair * l * r, *gi = Ginv + (int64_t)pair * n * n;
    double *W = sm, *Gi = sm + K * n, *X = Ps + (int64_t)pair * l * r;
    for (int e = tid; e < l * r; e += AB_THREADS) {
        const int i = e / r, j = e % r;
        if (l <= r) W[j * n + i] = os[e]; else W[i * n + j] = os[e];
    }
    for (int e = tid; e < n * n; e += AB_THREADS) Gi[e] = gi[e];
    __syncthreads();
    for (int e = tid; e < K * n; e += AB_THREADS) {
        const int c = e / n, j = e % n;
        double s = 0.0;
        for (int p = 0; p < n; ++p) s = fma(W[c * n + p], Gi[p * n + j], s);
        if (l <= r) X[(int64_t)c * l + j] = s;          // r x l, row c
        else        X[(int64_t)j * l + c] = s;          // r x l, row j
    }
}

// one pair's operands, before grouping
struct AbPair {
    const double *psi, *om;
    double *c, *work;
    int64_t m;
    int k, b;
};

// the group table of one launch: the plan's groups [t.g0, t.g0 + t.ng) with the operands of their first pairs
AbTable make_table(const std::vector<AbPair> &pairs, const std::vector<AbGroupPlan> &groups, const AbLaunchPlan &lp)
{
    AbTable t{};
    t.ng = lp.ng;
    for (int i = 0; i < lp.ng; ++i) {
        const AbGroupPlan &gp = groups[lp.g0 + i];
        const AbPair &p0 = pairs[gp.first];
        AbGroup &g = t.g[i];
        g.psi = p0.psi; g.om = p0.om; g.pin = p0.work; g.pout = p0.work; g.c = p0.c;
        g.s_psi = gp.s_psi; g.s_om = gp.s_om; g.s_pin = gp.s_work; g.s_pout = gp.s_work; g.s_c = gp.s_c;
        g.m = gp.m; g.count = gp.count; g.chunks = lp.chunks[i]; g.first = lp.first[i];
    }
    return t;
}

int apply_fallback(const std::vector<AbPair> &pairs, int64_t l, int64_t r, int direction, int stream, hipStream_t st)
{
    int rc;
    for (const AbPair &p : pairs) {
        double *R = (double *)scratch(stream, SCRATCH_DRIVER, (size_t)p.m * (direction == 0 ? r : l) * 8);
        if (!R) return TTSK_ERR_HIP;
        if (direction == 0) {
            if ((rc = gemm_plain(p.m, l, r, p.psi, r, 1, p.work, l, 1, p.c, stream, 1.0, 0))) return rc;            // C = Psi P
            TTSK_HIP(hipMemcpyAsync(R, p.psi, (size_t)p.m * r * 8, hipMemcpyDeviceToDevice, st));
            if ((rc = gemm_plain(p.m, r, l, p.c, l, 1, p.om, r, 1, R, stream, -1.0, 1))) return rc;                 // R = Psi - C Omega
            if ((rc = gemm_plain(p.m, l, r, R, r, 1, p.work, l, 1, p.c, stream, 1.0, 1))) return rc;                // C += R P
        } else {
            if ((rc = gemm_plain(r, p.m, l, p.work, l, 1, p.psi, p.m, 1, p.c, stream, 1.0, 0))) return rc;          // C = P Psi
            TTSK_HIP(hipMemcpyAsync(R, p.psi, (size_t)l * p.m * 8, hipMemcpyDeviceToDevice, st));
            if ((rc = gemm_plain(l, p.m, r, p.om, r, 1, p.c, p.m, 1, R, stream, -1.0, 1))) return rc;               // R = Psi - Omega C
            if ((rc = gemm_plain(r, p.m, l, p.work, l, 1, R, p.m, 1, p.c, stream, 1.0, 1))) return rc;              // C += P R
        }
    }
    return TTSK_OK;
}

// the pairs of one Omega shape (l x r): what is launched is decided by assemble_batch_plan.h
int assemble_shape(const std::vector<AbPair> &pairs, int64_t l, int64_t r, int direction, int stream, hipStream_t st)
{
    int rc;
    AbShapePlan sp;
    ab_shape_plan(l, r, direction, (int)pairs.size(), pinv_batch_fast(l, r), &sp);
    if (!sp.covered) {
        for (const AbPair &p : pairs) {
            if ((rc = ttsk_pinv_begin(p.om, l, r, -1.0, p.work, stream)) < 0) return rc;
            if ((rc = ttsk_pinv_end(p.om, l, r, -1.0, p.work, nullptr, stream)) < 0) return rc;
        }
        return apply_fallback(pairs, l, r, direction, stream, st);
    }
    double *ws = (double *)scratch(stream, SCRATCH_ORTH, sp.bytes);
    if (!ws) return TTSK_ERR_HIP;
    double *Os = ws + sp.off_Os, *Ps = ws + sp.off_Ps, *Gm = ws + sp.off_Gm, *Rinv = ws + sp.off_Rinv, *Ginv = ws + sp.off_Ginv;
    int *status = (int *)(ws + sp.off_status);
    // the grouping works on element offsets from the first pair's operands
    std::vector<AbPairOff> offs(pairs.size());
    for (size_t i = 0; i < pairs.size(); ++i)
        offs[i] = AbPairOff{pairs[i].psi - pairs[0].psi, pairs[i].om - pairs[0].om, pairs[i].c - pairs[0].c, pairs[i].work - pairs[0].work,
                            pairs[i].m, pairs[i].k};
    const std::vector<AbGroupPlan> groups = ab_make_groups(offs);
    char msg[200];
    AbLaunchPlan lp;
    // ---- pseudo-inverses: gram, chol, solve, jacobi
    for (size_t g0 = 0; g0 < groups.size(); g0 += AB_MAXG) {
        ab_gram_launch(groups, g0, &lp);
        if ((rc = launch(assemble_gram_kernel, dim3((unsigned)lp.wgs), dim3(AB_THREADS), sp.gram_lds, st, make_table(pairs, groups, lp), (int)l,
                         (int)r, Os + (size_t)lp.base * sp.lr, Gm + (size_t)lp.base * sp.nn))) return rc;
    }
    if ((rc = chol_inv_batch(Gm, sp.n, Rinv, Ginv, status, sp.T, st))) return rc;
    if ((rc = launch(assemble_solve_kernel, dim3((unsigned)sp.T), dim3(AB_THREADS), sp.solve_lds, st, (int)l, (int)r, Os, Ginv, Ps))) return rc;
    rc = jacobi_pinv_spaced(sp.T, Os, (int64_t)sp.lr, l, r, Ps, (int64_t)sp.lr, status, st);
    if (rc < 0) return rc;
    if (rc == 0) { ab_msg_jacobi(msg, sizeof(msg), l, r); set_error("%s", msg); return TTSK_ERR_UNSUPPORTED; }
    // ---- fused apply: P and Omega from the staging buffers, P copied out to the caller's work
    if (!sp.apply_lds_ok) { ab_msg_lds(msg, sizeof(msg)); set_error("%s", msg); return TTSK_ERR_UNSUPPORTED; }
    for (size_t g0 = 0; g0 < groups.size(); g0 += AB_MAXG) {
        ab_apply_launch(groups, g0, &lp);
        AbTable t = make_table(pairs, groups, lp);
        for (int i = 0; i < t.ng; ++i) {
            const int pair = groups[g0 + i].first;
            t.g[i].om = Os + (size_t)pair * sp.lr; t.g[i].s_om = (int64_t)sp.lr;
            t.g[i].pin = Ps + (size_t)pair * sp.lr; t.g[i].s_pin = (int64_t)sp.lr;
        }
        if ((rc = launch(direction == 0 ? assemble_apply_kernel<false> : assemble_apply_kernel<true>, dim3((unsigned)lp.wgs), dim3(AB_THREADS),
                         sp.apply_lds, st, t, sp.a, sp.b))) return rc;
    }
    return TTSK_OK;
}

}  // namespace

extern "C" {

int ttsk_tt_assemble_batch(int count, int d, const int64_t *n, const int64_t *lr, const int64_t *rr, const double *const *psi,
                           const double *const *omega, double *const *cores_out, double *const *work, int direction, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(count >= 1 && d >= 2 && d <= 64 && n && lr && rr && psi && omega && cores_out && work && (direction == 0 || direction == 1),
             "ttsk_tt_assemble_batch: bad argument");
    for (int mu = 0; mu < d; ++mu) TTSK_ARG(n[mu] >= 1, "ttsk_tt_assemble_batch: bad mode size %d", mu);
    for (int k = 0; k < d - 1; ++k) TTSK_ARG(lr[k] >= 1 && rr[k] >= 1, "ttsk_tt_assemble_batch: bad rank %d", k);
    for (int64_t i = 0; i < (int64_t)count * d; ++i) TTSK_ARG(psi[i] && cores_out[i], "ttsk_tt_assemble_batch: NULL core %lld", (long long)i);
    for (int64_t i = 0; i < (int64_t)count * (d - 1); ++i)
        TTSK_ARG(omega[i] && work[i], "ttsk_tt_assemble_batch: NULL Omega or work %lld", (long long)i);
    // pairs by Omega shape, mode-major: within a mode the tensors follow one another (their operands usually equally spaced)
    std::map<std::pair<int64_t, int64_t>, std::vector<AbPair>> shapes;
    for (int k = 0; k < d - 1; ++k)
        for (int b = 0; b < count; ++b) {
            AbPair p{};
            p.k = k; p.b = b;
            p.om = omega[(size_t)b * (d - 1) + k];
            p.work = work[(size_t)b * (d - 1) + k];
            if (direction == 0) {
                p.psi = psi[(size_t)b * d + k]; p.c = cores_out[(size_t)b * d + k];
                p.m = (k ? lr[k - 1] : 1) * n[k];
            } else {
                p.psi = psi[(size_t)b * d + k + 1]; p.c = cores_out[(size_t)b * d + k + 1];
                p.m = n[k + 1] * (k + 1 < d - 1 ? rr[k + 1] : 1);
            }
            shapes[{lr[k], rr[k]}].push_back(p);
        }
    int rc;
    for (auto &kv : shapes)
        if ((rc = assemble_shape(kv.second, kv.first.first, kv.first.second, direction, stream, st)) < 0) return rc;
    // the core that is copied unchanged (it may alias its Psi)
    const int e = direction == 0 ? d - 1 : 0;
    const int64_t sz = direction == 0 ? lr[d - 2] * n[d - 1] : n[0] * rr[0];
    for (int b = 0; b < count; ++b) {
        const double *src = psi[(size_t)b * d + e];
        double *dst = cores_out[(size_t)b * d + e];
        if (dst != src) TTSK_HIP(hipMemcpyAsync(dst, src, (size_t)sz * 8, hipMemcpyDeviceToDevice, st));
    }
    return TTSK_OK;
}

}  // extern "C"
