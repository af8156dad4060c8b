// TT input x TT DRMs: the whole streaming sketch (both chains, Omega, Psi) as one C call.
// See include/ttsk.h (ttsk_tt_sketch) for the contract and the reference lines it replaces.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <vector>
#include "common.h"
#include "prof.h"
#include "skinny.h"
#include "chain_fused.h"
#include "chain_wide.h"
#include "chain_sum.h"
#include "tt_chain.h"
#include "stream_small.h"
#include "sketch_split.h"

namespace ttsk {

// C (+)= A * B as described by d, tagged with its profiling class.
static int gemm(int cls, const ttsk_gemm_desc &d, const double *A, const double *B, double *C, int stream)
{
    ProfClass pc(cls);
    return ttsk_gemm(&d, A, B, C, nullptr, stream);
}

// One product for every tensor of a batch: the chain kernels take all nb problems in one launch
// (skinny_try_batch); shapes they do not cover fall back to one ttsk_gemm per tensor.
struct BatchPtrs {
    const double *A[SK_MAXB], *B[SK_MAXB];
    double *C[SK_MAXB];
};

static int gemm_batch(int cls, int nb, ttsk_gemm_desc d, const BatchPtrs &p, int stream, hipStream_t st,
                      bool chain_only = false)
{
    ProfClass pc(cls);
    ttsk_gemm_desc n = d;
    if (n.Ki == 1) { n.Ki = n.Ko; n.Ko = 1; n.a_ki = n.a_ko; n.b_ki = n.b_ko; }
    else if (n.Ko > 1 && n.a_ko == n.Ki * n.a_ki && n.b_ko == n.Ki * n.b_ki) { n.Ki *= n.Ko; n.Ko = 1; }
    int rc = skinny_try_batch(n, nb, p.A, p.B, p.C, stream, st);
    if (rc == 0 && !chain_only) rc = small_try_batch(n, nb, p.A, p.B, p.C, stream, st);
    if (rc == 0 && !chain_only) {
        rc = 1;
        for (int b = 0; b < nb && rc == 1; ++b) {
            const int e = ttsk_gemm(&d, p.A[b], p.B[b], p.C[b], nullptr, stream);
            if (e != TTSK_OK) rc = e;
        }
    }
    return rc;   // 1 = done, 0 = not covered (chain_only), < 0 = error
}

// A Psi product on the streamed kernel (stream_small.h), profiling class 4, with a.J set here from J: the kernel's row
// count is an int, taller products are not covered.  1 = launched, 0 = not covered, < 0 = error.
// cus: the CU budget of the Psi products of this call (sketch_split.h).
template <class Args>
static int psi_stream(int (*try_launch)(const Args &, int, hipStream_t, int), Args a, int64_t J, int q, hipStream_t st, int cus)
{
    if (J >= (1ll << 30)) return 0;
    a.J = (int)J;
    ProfClass pc(4);
    return try_launch(a, q, st, cus);
}

// The process-wide setting of ttsk_tt_sketch_split: per class -1 = the policy's budget, 0 = the whole device, > 0 = that many CUs
static std::atomic<int> split_set[3] = {{-1}, {-1}, {-1}};
// The stream of the one-call sketch queued last in this process (run_chains: how a pipelining caller is known)
static std::atomic<int> last_sketch_stream{-1};

// Where Psi_mu and Omega_mu sit in one sketch (when psi_at / om_at are given), and the sketch's size
static int64_t sketch_offsets(int d, const int64_t *n, const int64_t *l_lo, const int64_t *l_hi, const int64_t *r_lo,
                              const int64_t *r_hi, size_t *psi_at = nullptr, size_t *om_at = nullptr)
{
    int64_t tot = 0;
    for (int mu = 0; mu < d; ++mu) {
        int64_t l = mu == 0 ? 1 : l_hi[mu - 1] - l_lo[mu - 1];
        int64_t r = mu == d - 1 ? 1 : r_hi[d - 2 - mu] - r_lo[d - 2 - mu];
        if (psi_at) psi_at[mu] = tot;
        tot += l * n[mu] * r;
    }
    for (int mu = 0; mu < d - 1; ++mu) {
        if (om_at) om_at[mu] = tot;
        tot += (l_hi[mu] - l_lo[mu]) * (r_hi[d - 2 - mu] - r_lo[d - 2 - mu]);
    }
    return tot;
}

// Workspace (slot DRIVER of the caller's stream) of a call's signature -- nb tensors of d modes, TT ranks s, DRM
// ranks lt / rt, rank slices [lo, hi) -- one block per QUANTITY with the nb tensors behind one another:
// Lc[mu] (s[mu+1] x lt[mu+1]), Rc[j] (s[d-1-j] x rt[j+1]), T[mu] per left mode (kept for the Psi phase), one
// T buffer for the right chain.  Tensor b of a quantity of size sz sits at block + b * stride(sz), stride =
// sz rounded up to even (16-byte operand loads).  Where sz is even the nb chain matrices of a mode are ONE
// (nb s) x rank matrix: the two-launch chain step and the Psi / Omega of a sum then run as one product over
// all tensors ("merged" below) and read the DRM core once instead of once per tensor.
// Also where Psi_mu / Omega_mu sit in one sketch (psi_at / om_at).
struct SketchWs {
    int nb, d;
    const int64_t *n, *s, *lt, *l_lo, *l_hi, *rt, *r_lo, *r_hi;
    bool sum;                     // ONE sketch, of the sum of the nb tensors
    std::vector<size_t> offL, offR, offT, szL, szR, szT;
    size_t offTR, szTR, offP0, szP0, offPs, szPs, bytes;
    std::vector<size_t> psi_at, om_at;
    std::vector<int> t_inter;     // T[mu] stored interleaved: T[(q,k)][(b,p')], row length nb * s[mu+1] (the left chain decides)
    double *ws0 = nullptr;

    static size_t even(size_t v) { return v + (v & 1); }
    static size_t blk(size_t v) { return (v + 31) & ~(size_t)31; }
    int64_t lw(int mu) const { return l_hi[mu] - l_lo[mu]; }   // width of left slice mu
    int64_t rw(int j) const { return r_hi[j] - r_lo[j]; }      // width of right slice j

    SketchWs(int nb_, int d_, const int64_t *n_, const int64_t *s_, const int64_t *lt_, const int64_t *l_lo_, const int64_t *l_hi_,
             const int64_t *rt_, const int64_t *r_lo_, const int64_t *r_hi_, bool sum_)
        : nb(nb_), d(d_), n(n_), s(s_), lt(lt_), l_lo(l_lo_), l_hi(l_hi_), rt(rt_), r_lo(r_lo_), r_hi(r_hi_), sum(sum_), offL(d - 1),
          offR(d - 1), offT(d), szL(d - 1), szR(d - 1), szT(d), psi_at(d), om_at(d - 1), t_inter(d, 0)
    {
        size_t tot = 0;
        for (int mu = 0; mu < d - 1; ++mu) { szL[mu] = even((size_t)s[mu + 1] * lt[mu + 1]); offL[mu] = tot; tot += blk(nb * szL[mu]); }
        for (int j = 0; j < d - 1; ++j) { szR[j] = even((size_t)s[d - 1 - j] * rt[j + 1]); offR[j] = tot; tot += blk(nb * szR[j]); }
        for (int mu = 1; mu < d; ++mu) { szT[mu] = even((size_t)lt[mu] * n[mu] * s[mu + 1]); offT[mu] = tot; tot += blk(nb * szT[mu]); }
        size_t tr_max = 0;
        for (int mu = 1; mu < d - 1; ++mu) tr_max = std::max(tr_max, (size_t)rt[d - 1 - mu] * n[mu] * s[mu]);
        szTR = even(tr_max), offTR = tot;
        tot += blk(nb * szTR);
        szP0 = even((size_t)n[0] * rw(d - 2)), offP0 = tot;   // sum mode: Psi_0 per tensor
        if (sum) tot += blk(nb * szP0);
        // sum mode, larger TT ranks: Psi_mu per tensor (the streamed kernel), then one sum -- faster than the generic
        // tiles on a contracted index of nb * s (measured: s = 60, 100); one block per stream of the Psi phase
        // (small TT ranks: the same blocks take the partial Psi of the K chunks of the one product over (tensor, rank))
        szPs = 0;
        for (int mu = 1; sum && mu < d - 1; ++mu) szPs = std::max(szPs, even((size_t)lw(mu - 1) * n[mu] * rw(d - 2 - mu)));
        offPs = tot;
        tot += 2 * blk(nb * szPs);
        bytes = tot * 8;
        sketch_offsets(d, n, l_lo, l_hi, r_lo, r_hi, psi_at.data(), om_at.data());
    }

    double *Lp(int b, int mu) const { return ws0 + offL[mu] + (size_t)b * szL[mu]; }
    double *Rp(int b, int j) const { return ws0 + offR[j] + (size_t)b * szR[j]; }
    double *Tp0(int b, int mu) const { return ws0 + offT[mu] + (size_t)b * szT[mu]; }     // per-tensor T[q][k][p']
    double *TRp(int b) const { return ws0 + offTR + (size_t)b * szTR; }
    double *P0(int b) const { return ws0 + offP0 + (size_t)b * szP0; }
    double *Ps(int half) const { return ws0 + offPs + (size_t)half * blk(nb * szPs); }
    // "merged" needs the tensors of a chain matrix exactly behind one another
    bool packedL(int mu) const { return szL[mu] == (size_t)s[mu + 1] * lt[mu + 1]; }
    bool packedR(int j) const { return szR[j] == (size_t)s[d - 1 - j] * rt[j + 1]; }
    // the rank slices that Omega and Psi read: columns [l_lo, l_hi) of L_mu, [r_lo, r_hi) of R_j, and the rows
    // (q, k), q >= l_lo[mu-1], of T_b[mu] (row stride t_ld(mu))
    const double *Lslice(int b, int mu) const { return Lp(b, mu) + l_lo[mu]; }
    const double *Rslice(int b, int j) const { return Rp(b, j) + r_lo[j]; }
    int64_t t_ld(int mu) const { return t_inter[mu] ? (int64_t)nb * s[mu + 1] : s[mu + 1]; }
    const double *Tslice(int b, int mu) const
    {
        const size_t row0 = (size_t)(l_lo[mu - 1] * n[mu]);
        return t_inter[mu] ? ws0 + offT[mu] + row0 * t_ld(mu) + (size_t)b * s[mu + 1] : Tp0(b, mu) + row0 * s[mu + 1];
    }
};

// One call: its workspace layout and what the chain steps and the tails need besides.
struct Ctx : SketchWs {
    const double *const *X, *const *DL, *const *DR;
    double *out;              // sketch b at out + b * out_stride (one sketch when sum)
    int64_t out_stride;
    int accumulate, stream;
    hipStream_t st;
    bool keep_t;              // keep the left chain's T for the Psi phase (false: the chains only)
    int aux = 0; hipStream_t st_aux = nullptr;   // the helper stream (set by run_chains, with the workspace)
    SketchSplit cus = SKETCH_SPLIT_FULL;         // the CU budgets of this call (set by run_chains, asked once per call)
    const double *Xc(int b, int mu) const { return X[(size_t)b * d + mu]; }
    double *outb(int b) const { return out + (size_t)b * out_stride; }
};

#define CK(x) do { rc = (x); if (rc < 0) return rc; } while (0)

static int check_ranks(const char *who, int d, const int64_t *s, const int64_t *lt, const int64_t *l_lo, const int64_t *l_hi,
                       const int64_t *rt, const int64_t *r_lo, const int64_t *r_hi)
{
    TTSK_ARG(s[0] == 1 && s[d] == 1 && lt[0] == 1 && rt[0] == 1, "%s: boundary ranks must be 1", who);
    for (int mu = 0; mu < d - 1; ++mu) {
        TTSK_ARG(0 <= l_lo[mu] && l_lo[mu] <= l_hi[mu] && l_hi[mu] <= lt[mu + 1], "%s: left rank slice %d out of range", who, mu);
        TTSK_ARG(0 <= r_lo[mu] && r_lo[mu] <= r_hi[mu] && r_hi[mu] <= rt[mu + 1], "%s: right rank slice %d out of range", who, mu);
    }
    return TTSK_OK;
}

// One chain step in one launch, first choice first: the fused kernel (every extent <= 128, chain_fused.h); many
// low-rank tensors (the terms of a sum): rows of several terms stacked into full tiles (chain_sum.h); then the wide
// kernel (chain_wide.h).  2 = launched by the stacked-terms kernel (its T went to ca.Tint), 1 = launched by another,
// 0 = no kernel covers the shape, < 0 = error.  cus: the CU budget of this chain's steps (sketch_split.h); the stacked-terms
// kernel keeps its own grid rule (it leaves a quarter of the CUs to the other chain itself).
static bool chain_step_fits_fused(int64_t K1, int64_t J, int64_t A, int64_t A2) { return K1 <= 128 && J <= 128 && A <= 128 && A2 <= 128; }

// Whether chain_fused_plan will take an unforced step of these extents, as far as the extents alone decide it (its rules on
// J, the parity of A2, the depth of phase A and the tile structures, chain_plan.h): what the split policy is asked with.
static bool step_on_fused(int64_t K1, int64_t J, int64_t A, int64_t A2)
{
    if (!chain_step_fits_fused(K1, J, A, A2) || J > 112 || A < 4 || A2 < 4 || (A2 & 1) || 2 * K1 < A) return false;
    int nq, sq, nn, sn;
    chain_tile_split((int)A, nq, sq);
    chain_tile_split((int)A2, nn, sn);
    return nq == nn && sq == sn && nq >= 1 && nq + (sq ? 1 : 0) <= 7;
}

static int chain_step_try(int cls, const ChainSumArgs &ca, int stream, hipStream_t st, int cus)
{
    const ChainStepArgs &cs = ca.s;
    ProfClass pc(cls);
    int fz = chain_step_fits_fused(cs.K1, cs.J, cs.A, cs.A2) ? chain_fused_try(cs, stream, st, false, cus) : 0;
    if (fz == 0 && (fz = chain_sum_try(ca, stream, st)) == 1) return 2;
    if (fz == 0) fz = chain_wide_try(cs, stream, st, false, cus);
    return fz;
}

// right chain: walks modes d-1, ..., 1 on the transposed tensor (views only).  Xt_j[p,k,p''] = X_mu[p'',k,p], mu = d-1-j.
static int right_step(const Ctx &c, int j)
{
    const int nb = c.nb, mu = c.d - 1 - j;
    const int64_t sp = c.s[mu + 1], sn = c.s[mu], nn = c.n[mu], rho = c.rt[j], rhop = c.rt[j + 1];
    int rc;
    BatchPtrs p{};
    if (j == 0) {
        // Rc_0[p'',q'] = sum_k X[p'',k,0] E[0,k,q']
        for (int b = 0; b < nb; ++b) { p.A[b] = c.Xc(b, mu); p.B[b] = c.DR[j]; p.C[b] = c.Rp(b, j); }
        CK(gemm_batch(5, nb, gemm_desc2(sn, rhop, 1, nn, nn * sp, 0, sp, 0, rhop, 1, rhop, 1, 0), p, c.stream, c.st));
        return TTSK_OK;
    }
    // first choice: both products in one launch, T never written (chain_fused.h)
    for (int b = 0; b < nb; ++b) { p.A[b] = c.Rp(b, j - 1); p.B[b] = c.Xc(b, mu); p.C[b] = c.Rp(b, j); }
    const ChainStepArgs cs{nb, (int)nn, (int)sp, (int)rho, (int)rhop, (int)sn, p.A, rho, p.B, nn * sp, sp, 1, sn * nn * sp,
                           c.DR[j], nullptr, p.C};
    CK(chain_step_try(1, ChainSumArgs{cs, nullptr, 0, 0, 0}, c.stream, c.st, c.cus.right));
    if (rc) return TTSK_OK;
    // otherwise two launches.  T[q, k, b, p''] = sum_p Rc_b[p,q] X_b[p'',k,p]: a product batched over k whose
    // batch index joins the streamed index, written interleaved over the tensors (row (q,k), columns (b,p'')) ...
    const bool merged = nb > 1 && c.packedR(j) && (int64_t)nb * sn * rho * nn <= (int64_t)nb * c.szTR;
    const int64_t ldt = merged ? (int64_t)nb * sn : sn;
    for (int b = 0; b < nb; ++b) { p.A[b] = c.Rp(b, j - 1); p.B[b] = c.Xc(b, mu); p.C[b] = merged ? c.TRp(0) + (size_t)b * sn : c.TRp(b); }
    ttsk_gemm_desc g1 = gemm_desc2(rho, sn, 1, sp, 1, 0, rho, 0, 1, nn * sp, nn * ldt, 1, 0);
    g1.batch = nn; g1.b_b = sp; g1.c_b = ldt;
    const int fast = gemm_batch(0, nb, g1, p, c.stream, c.st, !merged);
    if (fast < 0) return fast;
    BatchPtrs q{};
    if (merged) {
        // ... so that Rn_all[(b,p''), q'] = sum_{q,k} T[(q,k), (b,p'')] E[q,k,q'] is ONE long product: E is read
        // once, not once per tensor
        q.A[0] = c.TRp(0); q.B[0] = c.DR[j]; q.C[0] = c.Rp(0, j);
        CK(gemm_batch(1, 1, gemm_desc2((int64_t)nb * sn, rhop, rho, nn, 1, nn * ldt, ldt, nn * rhop, rhop, 1, rhop, 1, 0), q,
                      c.stream, c.st));
        return TTSK_OK;
    }
    for (int b = 0; b < nb; ++b) { q.A[b] = c.TRp(b); q.B[b] = c.DR[j]; q.C[b] = c.Rp(b, j); }
    if (fast == 1) {
        // Rn[p'', q'] = sum_{q,k} T[q,k,p''] E[q,k,q']
        CK(gemm_batch(1, nb, gemm_desc2(sn, rhop, rho, nn, 1, nn * sn, sn, nn * rhop, rhop, 1, rhop, 1, 0), q, c.stream, c.st));
    } else {
        // T[q, p'', k] = sum_p Rc[p,q] X[p'',k,p]    (M=q, N=(p'',k), K=p)
        CK(gemm_batch(0, nb, gemm_desc2(rho, sn * nn, 1, sp, 1, 0, rho, 0, 1, sp, sn * nn, 1, 0), p, c.stream, c.st));
        // Rn[p'', q'] = sum_{q,k} T[q,p'',k] E[q,k,q']
        CK(gemm_batch(1, nb, gemm_desc2(sn, rhop, rho, nn, nn, sn * nn, 1, nn * rhop, rhop, 1, rhop, 1, 0), q, c.stream, c.st));
    }
    return TTSK_OK;
}

// left chain: L_mu and the shared products T_mu = L_{mu-1}^T X_mu (the last step only makes T_{d-1} = Psi_{d-1}: of a sketch
// per tensor straight into the sketch, of a sum into the workspace)
static int left_step(Ctx &c, int mu)
{
    const int nb = c.nb, d = c.d;
    const int64_t sn = c.s[mu], sp = c.s[mu + 1], nn = c.n[mu], *lt = c.lt;
    int rc;
    BatchPtrs p{};
    if (mu == 0) {
        // L_0[p',q'] = sum_k X_0[0,k,p'] D_0[0,k,q']
        for (int b = 0; b < nb; ++b) { p.A[b] = c.Xc(b, 0); p.B[b] = c.DL[0]; p.C[b] = c.Lp(b, 0); }
        CK(gemm_batch(5, nb, gemm_desc2(sp, lt[1], 1, nn, 1, 0, sp, 0, lt[1], 1, lt[1], 1, 0), p, c.aux, c.st_aux));
        return TTSK_OK;
    }
    const int64_t lfull = lt[mu];
    if (mu < d - 1) {
        // first choice: T and L_mu from one launch (chain_fused.h); T is still stored, Psi_mu needs it
        double *Tp[SK_MAXB];
        for (int b = 0; b < nb; ++b) { p.A[b] = c.Lp(b, mu - 1); p.B[b] = c.Xc(b, mu); p.C[b] = c.Lp(b, mu); Tp[b] = c.Tp0(b, mu); }
        const ChainStepArgs cs{nb, (int)nn, (int)sn, (int)lfull, (int)lt[mu + 1], (int)sp, p.A, lfull, p.B, 1, sp, nn * sp,
                               sn * nn * sp, c.DL[mu], c.keep_t ? Tp : nullptr, p.C};
        // stacked-terms kernel: T goes out interleaved over the terms for the Psi of a sum (one product over (term,
        // rank)), per term otherwise
        const bool inter = c.sum && nb > 1 && c.packedL(mu);
        const ChainSumArgs ca = c.keep_t ? ChainSumArgs{cs, c.Tp0(0, mu), inter ? sp : (int64_t)c.szT[mu], inter ? (int64_t)nb * sp : sp,
                                                        (int64_t)nb * (int64_t)c.szT[mu]}
                                         : ChainSumArgs{cs, nullptr, 0, 0, 0};
        CK(chain_step_try(3, ca, c.aux, c.st_aux, c.cus.left));
        if (rc == 2 && inter) c.t_inter[mu] = 1;
        if (rc) return TTSK_OK;
    }
    const bool merged = nb > 1 && mu < d - 1 && c.packedL(mu);
    if (merged) {
        // T[q, k, b, p'] = sum_p Lc_b[p,q] X_b[p,k,p'] interleaved over the tensors (batched over k) ...
        c.t_inter[mu] = 1;
        const int64_t ldt = (int64_t)nb * sp;
        double *T0 = c.Tp0(0, mu);
        for (int b = 0; b < nb; ++b) { p.A[b] = c.Lp(b, mu - 1); p.B[b] = c.Xc(b, mu); p.C[b] = T0 + (size_t)b * sp; }
        ttsk_gemm_desc g1 = gemm_desc2(lfull, sp, 1, sn, 1, 0, lfull, 0, nn * sp, 1, nn * ldt, 1, 0);
        g1.batch = nn; g1.b_b = sp; g1.c_b = ldt;
        CK(gemm_batch(2, nb, g1, p, c.aux, c.st_aux));
        // ... and L_all[(b,p'), q'] = sum_{q,k} T[(q,k), (b,p')] D[q,k,q'] as one long product
        BatchPtrs q{};
        q.A[0] = T0; q.B[0] = c.DL[mu]; q.C[0] = c.Lp(0, mu);
        CK(gemm_batch(3, 1, gemm_desc2((int64_t)nb * sp, lt[mu + 1], lfull, nn, 1, nn * ldt, ldt, nn * lt[mu + 1], lt[mu + 1], 1,
                                  lt[mu + 1], 1, 0), q, c.aux, c.st_aux));
        return TTSK_OK;
    }
    if (mu == d - 1 && !c.sum) {
        // last mode, a sketch per tensor: Psi_{d-1}[q,k,0] = T[q,k,0] for q in [l_lo, l_hi) -- the same product on those
        // columns of L_{d-2}, written (or accumulated) straight into the sketch: no T_{d-1}, no copy per tensor behind it
        if (c.lw(mu - 1) == 0) return TTSK_OK;
        for (int b = 0; b < nb; ++b) { p.A[b] = c.Lslice(b, mu - 1); p.B[b] = c.Xc(b, mu); p.C[b] = c.outb(b) + c.psi_at[mu]; }
        CK(gemm_batch(5, nb, gemm_desc2(c.lw(mu - 1), nn * sp, 1, sn, 1, 0, lfull, 0, nn * sp, 1, nn * sp, 1, c.accumulate), p, c.aux,
                      c.st_aux));
        return TTSK_OK;
    }
    // T[q,k,p'] = sum_p Lc[p,q] X[p,k,p']      (M=q (all lfull columns), N=(k,p'), K=p)
    for (int b = 0; b < nb; ++b) { p.A[b] = c.Lp(b, mu - 1); p.B[b] = c.Xc(b, mu); p.C[b] = c.Tp0(b, mu); }
    CK(gemm_batch(mu == d - 1 ? 5 : 2, nb, gemm_desc2(lfull, nn * sp, 1, sn, 1, 0, lfull, 0, nn * sp, 1, nn * sp, 1, 0), p,
                  c.aux, c.st_aux));
    if (mu < d - 1) {
        // L_mu[p',q'] = sum_{q,k} T[q,k,p'] D[q,k,q']
        BatchPtrs q{};
        for (int b = 0; b < nb; ++b) { q.A[b] = c.Tp0(b, mu); q.B[b] = c.DL[mu]; q.C[b] = c.Lp(b, mu); }
        CK(gemm_batch(3, nb, gemm_desc2(sp, lt[mu + 1], 1, lfull * nn, 1, 0, sp, 0, lt[mu + 1], 1, lt[mu + 1], 1, 0), q,
                      c.aux, c.st_aux));
    }
    return TTSK_OK;
}

// The right chain runs on the caller's stream, the left chain (when `left`) on a helper stream `aux` (the two are
// independent until Psi / Omega need both); the Psi products are then dealt over both.  The
// helper is forked from / joined into `stream`, so callers (and hipGraph capture) see one stream.
// TTSK_SINGLE_STREAM=1 keeps everything on `stream`: per-kernel event times are then free of
// cross-stream sharing and match rocprofv3's kernel durations (bench.py roofline leg).
// Requests the workspace, forks `aux` (does not join it), enqueues the steps alternately (neither chain waits for the
// host to have queued the other: 335 -> 319 us for one C3 tensor).  (Starting Psi_mu / Omega_mu on a third stream as
// soon as left step mu and right step d-2-mu are done was measured too: 325 us eager, 377 us replayed from a hipGraph,
// slower for 6-8 tensors -- the early products compete with the chain steps for the CUs.  Not kept.)
// The CU budgets (sketch_split.h) are asked here once per call: the right steps, the left steps and the Psi products of the
// tails all plan for them.
static int run_chains(Ctx &c, bool left)
{
    const char *single = getenv("TTSK_SINGLE_STREAM");
    c.aux = (single && single[0] == '1') ? c.stream : (c.stream + 1) % TTSK_NUM_STREAMS;
    const int n_cu = device_num_cu();
    if (n_cu < 1) return TTSK_ERR_HIP;
    bool fused = true;
    for (int mu = 1; mu < c.d - 1 && fused; ++mu) {
        const int j = c.d - 1 - mu;
        fused = step_on_fused(c.s[mu + 1], c.s[mu], c.rt[j], c.rt[j + 1]) && (!left || step_on_fused(c.s[mu], c.s[mu + 1], c.lt[mu], c.lt[mu + 1]));
    }
    const int set[3] = {split_set[0].load(), split_set[1].load(), split_set[2].load()};
    // A caller that queues its sketches on one stream pair has one step in flight, and a split only lengthens that step
    // (sketch_split.h); one that keeps several in flight hands consecutive calls to different stream pairs -- that is what
    // the stream argument is for -- and is known by it: the call before this one went to another stream.
    const int before = last_sketch_stream.exchange(c.stream);
    const bool pipelined = before >= 0 && before != c.stream;
    // (the chains-only calls of tt_orth.hip, T not kept, were not measured with budgets: the whole device)
    if (c.keep_t)
        c.cus = sketch_split_resolve(SketchSplitIn{n_cu, c.nb, c.d, c.n, c.s, c.lt, c.rt, left && c.aux != c.stream, pipelined,
                                                   fused ? SKETCH_FUSED : SKETCH_OTHER}, set);
    if (!(c.st_aux = stream_of(c.aux))) return TTSK_ERR_ARG;
    if (!(c.ws0 = (double *)scratch(c.stream, SCRATCH_DRIVER, c.bytes))) return TTSK_ERR_HIP;
    int rc;
    CK(ttsk_stream_wait(c.aux, c.stream));   // fork
    for (int t = 0; t < c.d; ++t) {
        if (t < c.d - 1) CK(right_step(c, t));
        if (left && (t < c.d - 1 || c.keep_t)) CK(left_step(c, t));
    }
    return TTSK_OK;
}

// sum mode, larger TT ranks: Psi_mu per tensor on the streamed kernel, then one sum (SketchWs::szPs)
constexpr int sum_psi_split = 48;

// Psi_mu of a sum, 0 < mu < d - 1, small TT ranks: Psi[(q,k), c] = sum_{b, p'} T_b[(q,k), p'] R_b[p', c]: (b, p') is
// one contracted index when both operands hold the tensors behind one another, a two-level one otherwise
static int psi_sum_one_product(const Ctx &c, int mu, int q)
{
    const int nb = c.nb, jr = c.d - 2 - mu;
    const int64_t sp = c.s[mu + 1], nn = c.n[mu], l = c.lw(mu - 1), r = c.rw(jr), ldr = c.rt[jr + 1], ldt = c.t_ld(mu);
    double *psi = c.out + c.psi_at[mu];
    int rc;
    const bool one_index = c.t_inter[mu] && c.packedR(jr);
    if (one_index && l * nn >= 1024) {
        // K = nb * sp (640 at C5) in chunks whose R image fits the LDS of the streamed kernel (stream_small.h:
        // fragments of T straight from memory, R in LDS, no barrier after staging): the chunks are the
        // "problems" of one launch, their partial Psi meet in one sum.  (One product on the generic tiles: 52 us
        // per mode at C5.)
        const int64_t K = (int64_t)nb * sp;
        const int nch = stream_small_chunks(K, r, nb);
        if (nch >= 1) {
            const int64_t Kc = K / nch;
            double *blk0 = c.Ps(mu & 1);
            BatchPtrs p{};
            for (int cidx = 0; cidx < nch; ++cidx) {
                p.A[cidx] = c.Tslice(0, mu) + (size_t)cidx * Kc; p.B[cidx] = c.Rslice(0, jr) + (size_t)cidx * Kc * ldr;
                p.C[cidx] = nch == 1 ? psi : blk0 + (size_t)cidx * c.szPs;
            }
            const StreamSmallArgs ss{nch, 0 /* J: psi_stream */, (int)Kc, (int)r, p.A, ldt, p.B, ldr, p.C, r, nch == 1 ? c.accumulate : 0};
            CK(psi_stream(stream_small_try, ss, l * nn, q, stream_of(q), c.cus.psi));
            if (rc == 1) return nch > 1 ? ttsk_sum_slices(psi, blk0, nch, c.szPs, (size_t)(l * nn * r), c.accumulate, q) : TTSK_OK;
        }
    }
    return gemm(4, one_index ? gemm_desc2(l * nn, r, 1, (int64_t)nb * sp, ldt, 0, 1, 0, ldr, 1, r, 1, c.accumulate)
                             : gemm_desc2(l * nn, r, nb, sp, ldt, c.t_inter[mu] ? sp : (int64_t)c.szT[mu], 1, (int64_t)c.szR[jr], ldr, 1,
                                     r, 1, c.accumulate), c.Tslice(0, mu), c.Rslice(0, jr), psi, q);
}

// Psi_mu (do_psi) and Omega_mu (do_omega) of one mode on stream q
static int psi_omega(const Ctx &c, int mu, int q, bool do_psi, bool do_omega)
{
    const int nb = c.nb, d = c.d;
    const int64_t sp = c.s[mu + 1], nn = c.n[mu];
    hipStream_t stq = stream_of(q);
    // right contraction of modes mu+1.. : Rc[j] with j = d-2-mu, columns [r_lo, r_hi)
    const int jr = d - 2 - mu;
    const int64_t ldr = mu < d - 1 ? c.rt[jr + 1] : 0, r = mu < d - 1 ? c.rw(jr) : 1;
    int rc = 0;
    BatchPtrs p{};
    if (!do_psi) {
    } else if (mu == 0) {
        // Psi_0[0,k,c] = sum_{p'} X_0[0,k,p'] R_0[p',c].  Of a sum: the cores X_b,0 are anywhere in memory: per-tensor
        // products into the workspace, then one sum
        for (int b = 0; b < nb; ++b) { p.A[b] = c.Xc(b, 0); p.B[b] = c.Rslice(b, jr); p.C[b] = c.sum ? c.P0(b) : c.outb(b) + c.psi_at[0]; }
        CK(gemm_batch(5, nb, gemm_desc2(nn, r, 1, sp, sp, 0, 1, 0, ldr, 1, r, 1, c.sum ? 0 : c.accumulate), p, q, stq));
        if (c.sum) CK(ttsk_sum_slices(c.out + c.psi_at[0], c.P0(0), nb, c.szP0, (size_t)(nn * r), c.accumulate, q));
    } else if (mu == d - 1) {
        // last mode: Psi_{d-1}[q,k,0] = T[q,k,0].  A sketch per tensor: left_step wrote it in place.  Of a sum: sum_b T_b[q,k,0]
        if (c.sum) CK(ttsk_sum_slices(c.out + c.psi_at[mu], c.Tslice(0, mu), nb, c.szT[mu], (size_t)(c.lw(mu - 1) * nn), c.accumulate, q));
    } else if (c.sum && sp <= sum_psi_split) {
        CK(psi_sum_one_product(c, mu, q));
    } else {
        const int64_t l = c.lw(mu - 1), ldt = c.t_ld(mu);
        if (c.sum && !c.t_inter[mu]) {
            // Psi_mu of the sum in ONE launch: every wave keeps its tile of the output over all terms (stream_small.h).
            // One descriptor spans all terms, and the kernel reads the last row of a term on to whole k-blocks against
            // zero rows of R: where lt n s is odd that is the pad double of even() between two terms, which no chain
            // step writes and which holds whatever the scratch slot held before -- it must be finite (stream_small.h:
            // the caller's guarantee), so it is zeroed here, on the Psi stream.  Even sizes (no pad) queue nothing.
            const size_t t_len = (size_t)c.lt[mu] * nn * sp;
            if (c.szT[mu] != t_len)
                TTSK_HIP(hipMemset2DAsync(c.Tp0(0, mu) + t_len, c.szT[mu] * 8, 0, 8, (size_t)nb, stq));
            const StreamSmallSumArgs sa{nb, 0 /* J: psi_stream */, (int)sp, (int)r, c.Tslice(0, mu), ldt, (int64_t)c.szT[mu],
                                        c.Rslice(0, jr), ldr, (int64_t)c.szR[jr], c.out + c.psi_at[mu], r, c.accumulate};
            CK(psi_stream(stream_small_sum_try, sa, l * nn, q, stq, c.cus.psi));
        }
        if (rc == 0) {
            // Psi[q,k,c] = sum_{p'} T[q,k,p'] R[p',c]   (M=(q,k), N=c, K=p') per tensor; of a sum into the workspace,
            // then one sum
            double *blk0 = c.Ps(mu & 1);
            for (int b = 0; b < nb; ++b) {
                p.A[b] = c.Tslice(b, mu); p.B[b] = c.Rslice(b, jr); p.C[b] = c.sum ? blk0 + (size_t)b * c.szPs : c.outb(b) + c.psi_at[mu];
            }
            const int acc = c.sum ? 0 : c.accumulate;
            const StreamSmallArgs ss{nb, 0 /* J: psi_stream */, (int)sp, (int)r, p.A, ldt, p.B, ldr, p.C, r, acc};
            CK(psi_stream(stream_small_try, ss, l * nn, q, stq, c.cus.psi));
            if (rc == 0) CK(gemm_batch(4, nb, gemm_desc2(l * nn, r, 1, sp, ldt, 0, 1, 0, ldr, 1, r, 1, acc), p, q, stq));
            if (c.sum) CK(ttsk_sum_slices(c.out + c.psi_at[mu], blk0, nb, c.szPs, (size_t)(l * nn * r), c.accumulate, q));
        }
    }
    if (mu == d - 1 || !do_omega) return TTSK_OK;
    const int64_t l = c.lw(mu);
    if (c.sum)   // Omega[q, c] = sum_{b, p} L_b[p, q] R_b[p, c]
        return gemm(5, c.packedL(mu) && c.packedR(jr)
                           ? gemm_desc2(l, r, 1, (int64_t)nb * sp, 1, 0, c.lt[mu + 1], 0, ldr, 1, r, 1, c.accumulate)
                           : gemm_desc2(l, r, nb, sp, 1, (int64_t)c.szL[mu], c.lt[mu + 1], (int64_t)c.szR[jr], ldr, 1, r, 1, c.accumulate),
                    c.Lslice(0, mu), c.Rslice(0, jr), c.out + c.om_at[mu], q);
    // Omega_mu = L_mu[:, lo:hi]^T R_mu[:, lo:hi]; the workspace blocks and the outputs of a
    // batch are equally spaced, so the nb products are one batched launch
    ttsk_gemm_desc od = gemm_desc2(l, r, 1, sp, 1, 0, c.lt[mu + 1], 0, ldr, 1, r, 1, c.accumulate);
    od.batch = nb; od.a_b = (int64_t)c.szL[mu]; od.b_b = (int64_t)c.szR[jr]; od.c_b = c.out_stride;
    return gemm(5, od, c.Lslice(0, mu), c.Rslice(0, jr), c.outb(0) + c.om_at[mu], q);
}

// Few tensors of one shape in every mode (one C3 tensor: 4 Psi, 5 Omega of equal shapes): the interior Psi
// products as ONE launch of the streamed kernel, all Omega as one batched launch -- the tail after the chains is
// then two launches deep on either stream instead of five.  1 = done, 0 = not this case (mode by mode then).
static int tail_grouped(const Ctx &c, bool ends_early)
{
    const int nb = c.nb, d = c.d;
    if (c.sum || d < 4 || nb * (d - 1) > SK_MAXB) return 0;
    // cores, TT and DRM ranks, rank slices and T layout of every mode those of mode 1 (Psi) / mode 0 (Omega)
    bool psis_and_omegas_one_shape = c.s[d - 1] == c.s[1] && c.lw(d - 2) == c.lw(0) && c.lt[d - 1] == c.lt[1] && c.rw(d - 2) == c.rw(0) &&
                                     c.rt[d - 1] == c.rt[1];
    for (int mu = 1; mu < d - 1; ++mu)
        psis_and_omegas_one_shape = psis_and_omegas_one_shape && c.n[mu] == c.n[1] && c.s[mu] == c.s[1] && c.s[mu + 1] == c.s[1] &&
                                    c.t_inter[mu] == c.t_inter[1] && c.lw(mu - 1) == c.lw(0) && c.lt[mu] == c.lt[1] &&
                                    c.lt[mu + 1] == c.lt[1] && c.rw(d - 2 - mu) == c.rw(0) && c.rt[d - 1 - mu] == c.rt[1];
    if (!psis_and_omegas_one_shape) return 0;
    const int64_t sp = c.s[1], nn = c.n[1], l = c.lw(0), r = c.rw(0), ldr = c.rt[1];
    int rc;
    BatchPtrs p{};
    int cnt = 0;
    for (int mu = 1; mu < d - 1; ++mu)
        for (int b = 0; b < nb; ++b, ++cnt) {
            p.A[cnt] = c.Tslice(b, mu); p.B[cnt] = c.Rslice(b, d - 2 - mu); p.C[cnt] = c.outb(b) + c.psi_at[mu];
        }
    const StreamSmallArgs ss{cnt, 0 /* J: psi_stream */, (int)sp, (int)r, p.A, c.t_ld(1), p.B, ldr, p.C, r, c.accumulate};
    CK(psi_stream(stream_small_try, ss, l * nn, c.stream, c.st, c.cus.psi));
    if (rc == 0) return 0;                 // shape outside the streamed kernel's cover: mode by mode
    BatchPtrs o{};
    cnt = 0;
    for (int mu = 0; mu < d - 1; ++mu)
        for (int b = 0; b < nb; ++b, ++cnt) {
            o.A[cnt] = c.Lslice(b, mu); o.B[cnt] = c.Rslice(b, d - 2 - mu); o.C[cnt] = c.outb(b) + c.om_at[mu];
        }
    CK(gemm_batch(5, cnt, gemm_desc2(l, r, 1, sp, 1, 0, c.lt[1], 0, ldr, 1, r, 1, c.accumulate), o, c.aux, c.st_aux));
    if (!ends_early) CK(psi_omega(c, 0, c.aux, true, false));
    CK(psi_omega(c, d - 1, c.stream, true, false));
    return 1;
}

// The batched launches of a sum of tensors, where all modes have one shape (the rest goes mode by mode):
static int tail_sum(const Ctx &c, bool &om_batched, bool &psi_batched)
{
    const int nb = c.nb, d = c.d;
    int rc;
    // the d - 1 Omega_mu = sum_{(b,p)} L_all[(b,p), q] R_all[(b,p), c] as ONE batched small launch (they were 5
    // launches of 15 us at C5, K = 640 each) where every Omega_mu has mode 0's shape and packed chain matrices
    bool omegas_one_packed_shape = d - 1 <= SK_MAXB && d >= 3;
    for (int mu = 0; mu < d - 1 && omegas_one_packed_shape; ++mu)
        omegas_one_packed_shape = c.s[mu + 1] == c.s[1] && c.lt[mu + 1] == c.lt[1] && c.rt[d - 1 - mu] == c.rt[d - 1] && c.packedL(mu) &&
                                  c.packedR(d - 2 - mu) && c.lw(mu) == c.lw(0) && c.rw(d - 2 - mu) == c.rw(d - 2);
    if (omegas_one_packed_shape) {
        BatchPtrs o{};
        for (int mu = 0; mu < d - 1; ++mu) { o.A[mu] = c.Lslice(0, mu); o.B[mu] = c.Rslice(0, d - 2 - mu); o.C[mu] = c.out + c.om_at[mu]; }
        const int64_t l = c.lw(0), r = c.rw(d - 2);
        CK(gemm_batch(5, d - 1, gemm_desc2(l, r, 1, (int64_t)nb * c.s[1], 1, 0, c.lt[1], 0, c.rt[d - 1], 1, r, 1, c.accumulate), o, c.aux, c.st_aux));
        om_batched = true;
    }
    // ... and the interior Psi: the K chunks of EVERY mode as the problems of ONE launch of the streamed kernel (4 modes x
    // 4 chunks at C5: 800 workgroups instead of four launches of 200 on two streams) where every interior Psi_mu has
    // mode 1's shape, T interleaved over the tensors and packed R
    if (d < 4) return TTSK_OK;
    const int64_t sp = c.s[2], nn = c.n[1], l = c.lw(0), r = c.rw(d - 3), ldr = c.rt[d - 2];
    bool psis_one_interleaved_shape = l * nn >= 1024;
    for (int mu = 1; mu < d - 1 && psis_one_interleaved_shape; ++mu) {
        const int jr = d - 2 - mu;
        psis_one_interleaved_shape = c.t_inter[mu] && c.packedR(jr) && c.n[mu] == nn && c.s[mu + 1] == sp && c.lw(mu - 1) == l &&
                                     c.rw(jr) == r && c.rt[jr + 1] == ldr;
    }
    if (!psis_one_interleaved_shape) return TTSK_OK;
    const int64_t K = (int64_t)nb * sp;
    const int nch = stream_small_chunks(K, r, nb);
    if (!(nch > 1 && (d - 2) * nch <= SK_MAXB && (d - 2) * nch <= 2 * nb && c.szPs >= (size_t)(l * nn * r))) return TTSK_OK;
    const int64_t Kc = K / nch, ldt = (int64_t)nb * sp;
    double *blk0 = c.Ps(0);
    BatchPtrs p{};
    int cnt = 0;
    for (int mu = 1; mu < d - 1; ++mu) {
        const double *T0 = c.Tslice(0, mu), *R0 = c.Rslice(0, d - 2 - mu);
        for (int cidx = 0; cidx < nch; ++cidx, ++cnt) {
            p.A[cnt] = T0 + (size_t)cidx * Kc; p.B[cnt] = R0 + (size_t)cidx * Kc * ldr; p.C[cnt] = blk0 + (size_t)cnt * c.szPs;
        }
    }
    const StreamSmallArgs ss{cnt, 0 /* J: psi_stream */, (int)Kc, (int)r, p.A, ldt, p.B, ldr, p.C, r, 0};
    CK(psi_stream(stream_small_try, ss, l * nn, c.stream, c.st, c.cus.psi));
    if (rc == 0) return TTSK_OK;
    psi_batched = true;
    CK(ttsk_stream_wait(c.aux, c.stream));
    for (int mu = 1; mu < d - 1; ++mu)
        CK(ttsk_sum_slices(c.out + c.psi_at[mu], blk0 + (size_t)(mu - 1) * nch * c.szPs, nch, c.szPs, (size_t)(l * nn * r),
                           c.accumulate, (mu & 1) ? c.aux : c.stream));
    return TTSK_OK;
}

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int64_t ttsk_tt_sketch_size(int d, const int64_t *n, const int64_t *l_lo, const int64_t *l_hi,
                            const int64_t *r_lo, const int64_t *r_hi)
{
    return sketch_offsets(d, n, l_lo, l_hi, r_lo, r_hi);
}

int ttsk_tt_sketch_split(int right_cus, int left_cus, int psi_cus)
{
    TTSK_ARG(right_cus >= -1 && left_cus >= -1 && psi_cus >= -1, "ttsk_tt_sketch_split: budgets (%d, %d, %d) must be >= -1", right_cus,
             left_cus, psi_cus);
    split_set[0] = right_cus; split_set[1] = left_cus; split_set[2] = psi_cus;
    return TTSK_OK;
}

int ttsk_tt_sketch(int d, const int64_t *n, const int64_t *s, const int64_t *lt, const int64_t *l_lo,
                   const int64_t *l_hi, const int64_t *rt, const int64_t *r_lo, const int64_t *r_hi,
                   const double *const *X, const double *const *DL, const double *const *DR, double *out,
                   int accumulate, int stream)
{
    return ttsk_tt_sketch_batch(1, d, n, s, lt, l_lo, l_hi, rt, r_lo, r_hi, X, DL, DR, out, 0, accumulate, stream);
}

// sum = false: sketch b at out + b * out_stride.  sum = true: ONE sketch, of the sum of the nb tensors -- the chains
// run per tensor as before (a sum of TTs is a TT with block-diagonal cores), Psi and Omega contract over
// (tensor, rank) at once: the per-tensor workspaces are equally spaced, so that pair is a two-level contracted
// index of one product, and no per-tensor sketch is ever written or summed.
static int tt_sketch_core(int nb, int d, const int64_t *n, const int64_t *s, const int64_t *lt, const int64_t *l_lo,
                          const int64_t *l_hi, const int64_t *rt, const int64_t *r_lo, const int64_t *r_hi,
                          const double *const *X, const double *const *DL, const double *const *DR, double *out,
                          int64_t out_stride, int accumulate, int stream, bool sum)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(nb >= 1, "ttsk_tt_sketch_batch: need nb >= 1, got %d", nb);
    TTSK_ARG(d >= 2, "ttsk_tt_sketch: need d >= 2, got %d", d);
    TTSK_ARG(n && s && lt && l_lo && l_hi && rt && r_lo && r_hi && X && DR && DL && out, "ttsk_tt_sketch: NULL argument");
    int rc;
    CK(check_ranks("ttsk_tt_sketch", d, s, lt, l_lo, l_hi, rt, r_lo, r_hi));
    const int64_t one = ttsk_tt_sketch_size(d, n, l_lo, l_hi, r_lo, r_hi);
    TTSK_ARG(sum || nb == 1 || out_stride >= one, "ttsk_tt_sketch_batch: out_stride %lld < sketch size %lld",
             (long long)out_stride, (long long)one);
    if (nb > SK_MAXB) {   // larger batches in slices of SK_MAXB tensors
        for (int b0 = 0; b0 < nb; b0 += SK_MAXB) {
            const int cnt = nb - b0 < SK_MAXB ? nb - b0 : SK_MAXB;
            rc = tt_sketch_core(cnt, d, n, s, lt, l_lo, l_hi, rt, r_lo, r_hi, X + (size_t)b0 * d, DL, DR,
                                sum ? out : out + (size_t)b0 * out_stride, out_stride, (sum && b0) ? 1 : accumulate,
                                stream, sum);
            if (rc) return rc;
        }
        return TTSK_OK;
    }
    if (nb == 1) sum = false;
    Ctx c{SketchWs(nb, d, n, s, lt, l_lo, l_hi, rt, r_lo, r_hi, sum), X, DL, DR, out, out_stride, accumulate, stream, st, true};
    CK(run_chains(c, true));
    // both chains are needed from here on, on both streams.
    // Psi_0 = X_0 R_0 needs the right chain only (this stream): queued BEFORE the join, it runs while this stream would wait for the
    // left chain (the join costs ~16 us of cross-queue latency) instead of standing behind the Omega launch at the very end
    // (one C3 tensor: 0.254 -> 0.239 ms).  (Psi_{d-1} of a sketch per tensor is the left chain's last product itself, written
    // into the sketch on the helper stream; of a sum it is summed from the T_b behind the join.)
    const bool ends_early = !sum && d >= 3;
    if (ends_early) CK(psi_omega(c, 0, stream, true, false));
    CK(ttsk_stream_wait(stream, c.aux));
    CK(ttsk_stream_wait(c.aux, stream));
    CK(tail_grouped(c, ends_early));
    if (rc == 0) {
        // mode by mode, dealt over the two streams, but for what a sum takes as batched launches
        bool om_batched = false, psi_batched = false;
        if (sum) CK(tail_sum(c, om_batched, psi_batched));
        for (int mu = 0; mu < d; ++mu) {
            const bool psi_here = !(psi_batched && mu >= 1 && mu < d - 1) && !(ends_early && mu == 0);
            if (!psi_here && (om_batched || mu == d - 1)) continue;
            CK(psi_omega(c, mu, (mu & 1) ? c.aux : stream, psi_here, !om_batched));
        }
    }
    CK(ttsk_stream_wait(stream, c.aux));   // join
    return TTSK_OK;
}

int ttsk_tt_sketch_batch(int nb, int d, const int64_t *n, const int64_t *s, const int64_t *lt, const int64_t *l_lo,
                         const int64_t *l_hi, const int64_t *rt, const int64_t *r_lo, const int64_t *r_hi,
                         const double *const *X, const double *const *DL, const double *const *DR, double *out,
                         int64_t out_stride, int accumulate, int stream)
{
    return tt_sketch_core(nb, d, n, s, lt, l_lo, l_hi, rt, r_lo, r_hi, X, DL, DR, out, out_stride, accumulate, stream, false);
}

int ttsk_tt_sketch_sum(int nb, int d, const int64_t *n, const int64_t *s, const int64_t *lt, const int64_t *l_lo,
                       const int64_t *l_hi, const int64_t *rt, const int64_t *r_lo, const int64_t *r_hi,
                       const double *const *X, const double *const *DL, const double *const *DR, double *out,
                       int accumulate, int stream)
{
    return tt_sketch_core(nb, d, n, s, lt, l_lo, l_hi, rt, r_lo, r_hi, X, DL, DR, out, 0, accumulate, stream, true);
}

}  // extern "C"

namespace ttsk {

int tt_chains(int d, const int64_t *n, const int64_t *s, const int64_t *lt, const int64_t *rt, const double *const *X,
              const double *const *DL, const double *const *DR, TTChains *out, int stream)
{
    return tt_chains_batch(1, d, n, s, lt, rt, X, DL, DR, out, stream);
}

// The chain steps of the streaming sketch over full rank ranges, no Psi, T not kept; the chain matrices stay in the
// workspace and their addresses are handed back (the orthogonalising sketches of tt_orth.hip go on from there).
int tt_chains_batch(int nb, int d, const int64_t *n, const int64_t *s, const int64_t *lt, const int64_t *rt, const double *const *X,
                    const double *const *DL, const double *const *DR, TTChains *out, int stream)
{
    if (d < 2 || d > 64 || !out) { set_error("tt_chains: bad argument"); return TTSK_ERR_ARG; }
    const bool left = out->want_left;
    std::vector<int64_t> zero(d, 0), lhi(d, 1), rhi(d, 1), ones(d + 1, 1);
    for (int mu = 0; mu < d - 1; ++mu) rhi[mu] = rt[mu + 1];
    for (int mu = 0; left && mu < d - 1; ++mu) lhi[mu] = lt[mu + 1];
    if (nb < 1 || nb > SK_MAXB) { set_error("tt_chains: %d tensors (1 .. %d)", nb, SK_MAXB); return TTSK_ERR_ARG; }
    TTSK_STREAM(st, stream);
    const int64_t *lt_ = left ? lt : ones.data();
    TTSK_ARG(n && s && lt_ && rt && X && DR && (DL || !left), "tt_chains: NULL argument");
    int rc;
    CK(check_ranks("tt_chains", d, s, lt_, zero.data(), lhi.data(), rt, zero.data(), rhi.data()));
    Ctx c{SketchWs(nb, d, n, s, lt_, zero.data(), lhi.data(), rt, zero.data(), rhi.data(), false), X, DL, DR, nullptr, 0, 0, stream,
          st, false};
    CK(run_chains(c, left));
    for (int j = 0; j < d - 1; ++j) { out->Rc[j] = c.Rp(0, j); out->r_stride[j] = (int64_t)c.szR[j]; }
    for (int mu = 0; mu < d - 1; ++mu) { out->Lc[mu] = left ? c.Lp(0, mu) : nullptr; out->l_stride[mu] = (int64_t)c.szL[mu]; }
    if (!left) return TTSK_OK;
    CK(ttsk_stream_wait(stream, c.aux));   // join
    // Omega_mu = L_mu^T R_mu: one launch per (tensor, mode), or per SK_MAXB of them when every mode's chain matrices
    // have mode 0's shape
    bool chain_pairs_one_shape = true;
    for (int mu = 1; mu < d - 1; ++mu)
        chain_pairs_one_shape = chain_pairs_one_shape && s[mu + 1] == s[1] && lt[mu + 1] == lt[1] && rt[d - 1 - mu] == rt[d - 1];
    BatchPtrs o{};
    int cnt = 0;
    for (int b = 0; b < nb; ++b)
        for (int mu = 0; mu < d - 1; ++mu) {
            o.A[cnt] = c.Lp(b, mu); o.B[cnt] = c.Rp(b, d - 2 - mu); o.C[cnt] = out->omega[(size_t)b * (d - 1) + mu];
            if (chain_pairs_one_shape && ++cnt < SK_MAXB && !(b == nb - 1 && mu == d - 2)) continue;
            const int64_t l = lt[mu + 1], r = rt[d - 1 - mu];
            CK(gemm_batch(5, chain_pairs_one_shape ? cnt : 1, gemm_desc2(l, r, 1, s[mu + 1], 1, 0, l, 0, r, 1, r, 1, 0), o, stream, st));
            cnt = 0;
        }
    return TTSK_OK;
}

#undef CK

}  // namespace ttsk
