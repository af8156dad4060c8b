// The normal-equations pseudo-inverse of the sketch path and the entry points of the small solves.
//
// Omega is an (l x r) sketch of full row or column rank nearly always, and for those pinv(Omega) = Omega^T (Omega Omega^T)^-1
// (l <= r) or (Omega^T Omega)^-1 Omega^T is a handful of small products around an n x n Cholesky inverse (cholesky.hip),
// n = min(l, r): ~0.1 ms instead of 2 ms for the one-workgroup Jacobi SVD at C3 (jacobi.hip).  The Cholesky kernel reports
// a rejection (not positive definite, or diag(R) spread beyond the gate) and the Jacobi kernel then runs on the untouched
// input -- queued behind the attempt with its verdict as predicate (ttsk_pinv_end, ttsk_pinv_batch), or read back once at
// the end through the stream's deferred flag (ttsk_orth_step, ttsk_pinv_batch_deferred: the caller repeats the sketch).
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include "skinny.h"
#include "solver.h"

namespace ttsk {

__global__ void add_diag_kernel(double *E, int n, double v)
{
    E += (size_t)blockIdx.x * n * n;               // batch: one n x n matrix per workgroup
    for (int i = threadIdx.x; i < n; i += blockDim.x) E[(size_t)i * n + i] += v;
}

// pinv(Omega) through the normal equations; 1 = done, 0 = rejected (caller runs the Jacobi SVD)
// Two phases, so that the d - 1 pseudo-inverses of an assembly can be in flight on their own streams
// before the host looks at the first verdict: `begin` queues Gram matrix, factorisation, the product
// Omega^T G^-1 (speculatively: it is overwritten if the factorisation is rejected) and the copy of the
// verdict into a pinned per-stream slot; `verdict` waits for the stream and reads it.
static int *pinv_host_status()
{
    return (int *)persistent_alloc(PA_PINV_HOST, TTSK_NUM_STREAMS * sizeof(int), true, false);
}
static int g_pinv_began[TTSK_NUM_STREAMS];
// the verdict of the attempt on the device, outside the scratch arena (which the Jacobi fallback reuses)
static int *pinv_dev_status(int stream)
{
    int *p = (int *)persistent_alloc(PA_PINV_DEV, TTSK_NUM_STREAMS * sizeof(int), false, false);
    return p ? p + stream : nullptr;
}

// deferred verdicts (ttsk_orth_step): one sticky word per stream, set by any rejected fast-path factorisation since the
// last ttsk_deferred_status
int *deferred_flag(int stream)
{
    int *p = (int *)persistent_alloc(PA_DEFERRED, TTSK_NUM_STREAMS * sizeof(int), false, true);
    return p ? p + stream : nullptr;
}

// gelsd's truncation rcond (rcond < 0: machine epsilon) with the rank-decision floor
static double pinv_rcond(int64_t l, int64_t r, double rcond)
{
    if (rcond < 0) rcond = DBL_EPSILON;
    // Rank-decision floor: one-sided Jacobi returns the rounding noise of a numerically rank
    // deficient Omega as singular values of size ~eps*||Omega||; gelsd's eps*sigma_max rule then
    // becomes a coin flip and a kept noise direction is amplified by 1/sigma^2.  Anything within
    // 16*sqrt(max(l,r)) of that noise level is treated as zero (documented in DESIGN.md).
    const double floor_ = 16.0 * DBL_EPSILON * sqrt((double)(l > r ? l : r));
    return rcond < floor_ ? floor_ : rcond;
}
// the normal equations stand in for gelsd where its truncation rule keeps every direction of a full-rank Omega
static bool pinv_fast(int64_t l, int64_t r, double rcond = -1.0) { return pinv_rcond(l, r, rcond) <= PINV_FAST_RCOND; }

// ---- the normal-equations pseudo-inverse as a list of stages, both orientations: Gram matrix, Cholesky inverse, solve and,
// with `refine`, one Newton-Schulz step, which squares the residual of the normal-equations inverse (kappa^2 eps -> ~kappa eps)
// and keeps the minimum-norm property (X stays in the row / column space of Omega): X1 = X0 (2 I - Omega X0) (l <= r) or
// (2 I - X0 Omega) X0.  Two executors run the list: one matrix through ttsk_gemm and chol_inv_any (pinv_cholesky_begin),
// `count` matrices of one shape through the batched small kernel and chol_inv_kernel, every stage one launch (pinv_batch).
enum NeBuf { NE_OM, NE_G, NE_GINV, NE_X0, NE_X1, NE_BUFS };   // Omega (l x r); G, later E (n x n); G^-1; X0, X1 (r x l)
struct NeStage {
    enum Op { PROD, CHOL, ADD_DIAG } op;                      // C = alpha A B; G^-1 from G; E += 2 I
    int64_t M, N, K, a_m, a_k, b_k, b_n;                      // PROD: gemm_desc's plain product ...
    double alpha;
    NeBuf a, b, c;                                            // ... of these buffers
    ttsk_gemm_desc desc() const { return gemm_desc(M, N, K, a_m, a_k, b_k, b_n, alpha); }
};
constexpr int NE_MAX_STAGES = 6;

static int ne_stages(int64_t l, int64_t r, bool refine, NeStage *s)
{
    int k = 0;
    auto prod = [&](int64_t M, int64_t N, int64_t K, int64_t a_m, int64_t a_k, int64_t b_k, int64_t b_n, double alpha, NeBuf a, NeBuf b,
                    NeBuf c) { s[k++] = NeStage{NeStage::PROD, M, N, K, a_m, a_k, b_k, b_n, alpha, a, b, c}; };
    auto step = [&](NeStage::Op op) { s[k++] = NeStage{op, 0, 0, 0, 0, 0, 0, 0, 0.0, NE_OM, NE_OM, NE_OM}; };
    if (l <= r) {                                                            // n = l
        prod(l, l, r, r, 1, 1, r, 1.0, NE_OM, NE_OM, NE_G);              // G = Omega Omega^T
        step(NeStage::CHOL);
        prod(r, l, l, 1, r, l, 1, 1.0, NE_OM, NE_GINV, NE_X0);           // X0 = Omega^T G^-1
        if (refine) {
            prod(l, l, r, r, 1, l, 1, -1.0, NE_OM, NE_X0, NE_G);         // E = -Omega X0
            step(NeStage::ADD_DIAG);                                     // E = 2 I - Omega X0
            prod(r, l, l, l, 1, l, 1, 1.0, NE_X0, NE_G, NE_X1);          // X1 = X0 E
        }
    } else {                                                                 // n = r
        prod(r, r, l, 1, r, r, 1, 1.0, NE_OM, NE_OM, NE_G);              // G = Omega^T Omega
        step(NeStage::CHOL);
        prod(r, l, r, r, 1, 1, r, 1.0, NE_GINV, NE_OM, NE_X0);           // X0 = G^-1 Omega^T
        if (refine) {
            prod(r, r, l, l, 1, r, 1, -1.0, NE_X0, NE_OM, NE_G);         // E = -X0 Omega
            step(NeStage::ADD_DIAG);                                     // E = 2 I - X0 Omega
            prod(r, l, r, r, 1, l, 1, 1.0, NE_G, NE_X0, NE_X1);          // X1 = E X0
        }
    }
    return k;
}

static size_t pinv_ws_elems(int n, int64_t mx) { return (size_t)3 * n * n + 16 + chol_ws_elems(n) + (size_t)mx * n; }   // mx = max(l, r)

// 1 = attempt queued, 0 = not applicable, < 0 = error.  ws_in: pinv_ws_elems(n) doubles of the caller's, or nullptr
// (then from the stream's arena).  sticky: deferred mode -- no copy of the verdict to the host, the rejection is
// recorded in *sticky and the caller decides at the end; the stages with the Newton-Schulz step and the gate at
// kappa = 3e4 (the refinement only where a rejection is expensive -- the deferred mode of ttsk_orth_step repeats the whole
// sketch; ttsk_pinv has the Jacobi kernel queued behind each attempt and keeps the plain gate at kappa = 300)
static int pinv_cholesky_begin(const double *omega, int64_t l, int64_t r, double *pinv, int stream, hipStream_t st,
                               double *ws_in = nullptr, int *sticky = nullptr)
{
    const int n = (int)(l <= r ? l : r);
    int *hs = pinv_host_status();
    int *status = pinv_dev_status(stream);
    if (n > CHOL_MAX_N || !hs || !status) return 0;
    const int64_t mx = l > r ? l : r;
    double *ws = ws_in ? ws_in : (double *)scratch(stream, SCRATCH_MISC, pinv_ws_elems(n, mx) * 8);
    if (!ws) return TTSK_ERR_HIP;
    double *G = ws, *Rinv = ws + n * n, *Ginv = ws + 2 * n * n, *cws = ws + 3 * n * n + 16;
    double *x1 = cws + chol_ws_elems(n);        // r x l: the refined pseudo-inverse before it replaces the first one
    const bool refine = sticky != nullptr;
    double *buf[NE_BUFS] = {const_cast<double *>(omega), G, Ginv, pinv, x1};      // (Omega is only ever read)
    NeStage s[NE_MAX_STAGES];
    const int ns = ne_stages(l, r, refine, s);
    for (int i = 0; i < ns; ++i) {
        const NeStage &e = s[i];
        int rc;
        if (e.op == NeStage::PROD) {
            const ttsk_gemm_desc g = e.desc();
            rc = ttsk_gemm(&g, buf[e.a], buf[e.b], buf[e.c], nullptr, stream);
        } else if (e.op == NeStage::ADD_DIAG) {
            rc = launch(add_diag_kernel, dim3(1), dim3(256), 0, st, G, n, 2.0);
        } else {
            rc = chol_inv_any(G, n, Rinv, Ginv, status, refine ? CHOL_GATE_REFINED : CHOL_GATE, stream, st, n > CHOL_ONE_N ? cws : nullptr,
                              sticky);
            if (rc == TTSK_OK && !sticky) {
                hs[stream] = 1;
                TTSK_HIP(hipMemcpyAsync(hs + stream, status, sizeof(int), hipMemcpyDeviceToHost, st));
            }
        }
        if (rc) return rc;
    }
    if (refine) TTSK_HIP(hipMemcpyAsync(pinv, x1, (size_t)r * l * 8, hipMemcpyDeviceToDevice, st));
    return 1;
}
// one pseudo-inverse with a deferred verdict (ranks up to 256); ws: pinv_deferred_ws_elems doubles
size_t pinv_deferred_ws_elems(int64_t l, int64_t r) { return pinv_ws_elems((int)(l < r ? l : r), l > r ? l : r); }
int pinv_deferred(const double *omega, int64_t l, int64_t r, double *pinv, int stream, hipStream_t st, double *ws, int *sticky)
{
    return pinv_cholesky_begin(omega, l, r, pinv, stream, st, ws, sticky);
}

// 1 = accepted (pinv is final), 0 = rejected
static int pinv_cholesky_verdict(int64_t l, int64_t r, int stream, hipStream_t st)
{
    TTSK_HIP(hipStreamSynchronize(st));
    const int host_status = pinv_host_status()[stream];
    static int trace = [] { const char *e = getenv("TTSK_GEMM_TRACE"); return e ? atoi(e) : 0; }();
    if (trace) fprintf(stderr, "ttsk_pinv %lld x %lld: normal equations %s\n", (long long)l, (long long)r,
                       host_status ? "rejected -> Jacobi SVD" : "accepted");
    return host_status ? 0 : 1;
}

bool pinv_batch_fast(int64_t l, int64_t r)
{
    return (l < r ? l : r) <= CHOL_ONE_N && pinv_fast(l, r);
}

bool pinv_batch_covers(int count, int64_t l, int64_t r, bool refine)
{
    if (!pinv_batch_fast(l, r)) return false;
    NeStage s[NE_MAX_STAGES];
    const int ns = ne_stages(l, r, refine, s);
    for (int i = 0; i < ns; ++i)
        if (s[i].op == NeStage::PROD && !small_batch_covers(s[i].desc(), count)) return false;
    return true;
}

// The pseudo-inverses of `count` matrices of ONE shape, every stage of the normal equations ONE batched launch.  refine = false
// (ttsk_pinv_batch): ttsk_pinv's contract -- the plain gate, and the Jacobi kernels queued behind the attempt, each with its own
// matrix's verdict as predicate (gelsd's truncation on rejection): 3 + count launches instead of 6 count (assemble_sketched_tt:
// the launches are what its d - 1 independent pseudo-inverses cost).  refine = true (ttsk_pinv_batch_deferred): the Newton-Schulz
// step behind them, verdicts deferred to `stream`'s flag (7 launches for the d - 1 Omega of an orthogonal sketch instead of 7
// each).  No read-back.  TTSK_ERR_UNSUPPORTED, with nothing queued: outside pinv_batch_covers (min(l, r) > 128, a stage beyond
// the small kernel), count > 32.
static int pinv_batch(const char *who, int count, const double *const *dev_omegas, int64_t l, int64_t r, double *const *dev_pinvs,
                      int stream, bool refine)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(count >= 1 && count <= SK_MAXB && dev_omegas && dev_pinvs && l >= 1 && r >= 1, "%s: bad argument", who);
    const int n = (int)(l < r ? l : r);
    // verdicts: the stream's deferred flag (refine), else one per matrix outside the scratch arena (the Jacobi kernel works there)
    int *sticky = refine ? deferred_flag(stream) : nullptr;
    int *vd = refine ? nullptr : (int *)persistent_alloc(PA_PINV_BATCH_VD, TTSK_NUM_STREAMS * SK_MAXB * sizeof(int), false, false);
    if (!(refine ? sticky : vd) || !pinv_batch_covers(count, l, r, refine)) {
        set_error("%s: (%lld x %lld) is outside the batched fast path", who, (long long)l, (long long)r);
        return TTSK_ERR_UNSUPPORTED;
    }
    const int transposed = r >= l;
    const int64_t mW = transposed ? r : l, nW = transposed ? l : r;
    const size_t jws = refine ? 0 : (size_t)(mW * nW + nW * nW) + 1;       // the Jacobi kernel's global working set
    const size_t nn = (size_t)n * n, rl = (size_t)r * l;
    double *ws = (double *)scratch(stream, SCRATCH_MISC, (jws + (size_t)count * (3 * nn + (refine ? rl : 0)) + 64) * 8);
    if (!ws) return TTSK_ERR_HIP;
    double *G0 = ws + jws, *R0 = G0 + count * nn, *I0 = R0 + count * nn, *X0 = I0 + count * nn;   // X0: count r x l (refine)
    int *status = refine ? (int *)(X0 + count * rl) : vd + (size_t)stream * SK_MAXB;
    double *buf[NE_BUFS][SK_MAXB];
    for (int b = 0; b < count; ++b) {
        TTSK_ARG(dev_omegas[b] && dev_pinvs[b], "%s: NULL matrix %d", who, b);
        buf[NE_OM][b] = const_cast<double *>(dev_omegas[b]);                   // (only ever read)
        buf[NE_G][b] = G0 + b * nn;
        buf[NE_GINV][b] = I0 + b * nn;
        buf[NE_X0][b] = refine ? X0 + b * rl : dev_pinvs[b];
        buf[NE_X1][b] = dev_pinvs[b];
    }
    NeStage s[NE_MAX_STAGES];
    const int ns = ne_stages(l, r, refine, s);
    int rc;
    for (int i = 0; i < ns; ++i) {
        const NeStage &e = s[i];
        if (e.op == NeStage::PROD) {
            rc = small_try_batch(e.desc(), count, buf[e.a], buf[e.b], buf[e.c], stream, st);
            if (rc == 0) { set_error("%s: internal error: the small kernel declined a covered stage", who); return TTSK_ERR_HIP; }
            if (rc == 1) rc = TTSK_OK;
        } else if (e.op == NeStage::ADD_DIAG) {
            rc = launch(add_diag_kernel, dim3((unsigned)count), dim3(256), 0, st, G0, n, 2.0);
        } else {
            rc = launch_chol(G0, n, R0, I0, status, refine ? CHOL_GATE_REFINED : CHOL_GATE, st, sticky, nullptr, count);
        }
        if (rc) return rc;
    }
    if (refine) return TTSK_OK;
    // rejected ones: the Jacobi kernel on the untouched input (it leaves at once where the attempt was accepted)
    const double *const *Om = dev_omegas;
    double *const *P = dev_pinvs;
    const double rcond = pinv_rcond(l, r, -1.0);
    // equally spaced inputs and outputs, matrices that live in LDS (no shared global scratch): ONE launch, a workgroup per matrix
    // (five launches of a kernel that leaves at once were 23 us of a 0.26 ms to_tt at C3)
    bool spaced = jacobi_fits_lds(mW, nW) && count >= 2;
    const int64_t os = count >= 2 ? Om[1] - Om[0] : 0, ps = count >= 2 ? P[1] - P[0] : 0;
    for (int b = 2; b < count && spaced; ++b) spaced = Om[b] - Om[b - 1] == os && P[b] - P[b - 1] == ps;
    if (spaced && os >= 0 && ps > 0)
        return launch_jacobi(count, Om[0], l, r, transposed, ws, ws + mW * nW, rcond, P[0], nullptr, nullptr, nullptr, nullptr, status, os,
                             ps, st);
    for (int b = 0; b < count; ++b)
        if ((rc = launch_jacobi(1, Om[b], l, r, transposed, ws, ws + mW * nW, rcond, P[b], nullptr, nullptr, nullptr, nullptr, status + b,
                                0, 0, st))) return rc;
    return TTSK_OK;
}

// ttsk_tt_assemble_batch (assemble_batch.hip): the stages of ttsk_pinv_batch over `count` matrices of one shape that lie
// equally spaced in the caller's staging buffer, without the 32-matrix limit of the pointer-array products.
int chol_inv_batch(const double *G, int n, double *Rinv, double *Ginv, int *status, int count, hipStream_t st)
{
    if (n > CHOL_ONE_N || count < 1) return TTSK_ERR_UNSUPPORTED;
    return launch_chol(G, n, Rinv, Ginv, status, CHOL_GATE, st, nullptr, nullptr, count);
}

// the Jacobi kernel behind the batched attempt, ONE launch, workgroup b on omega + b * os -> P + b * ps, predicated on
// status[b]; 1 = queued, 0 = the matrices do not fit the kernel's LDS (nothing queued)
int jacobi_pinv_spaced(int count, const double *omega, int64_t os, int64_t l, int64_t r, double *P, int64_t ps,
                       const int *status, hipStream_t st)
{
    const int transposed = r >= l;
    if (!jacobi_fits_lds(transposed ? r : l, transposed ? l : r)) return 0;
    if (int rc = launch_jacobi(count, omega, l, r, transposed, nullptr, nullptr, pinv_rcond(l, r, -1.0), P, nullptr, nullptr, nullptr,
                               nullptr, status, os, ps, st)) return rc;
    return 1;
}

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_pinv_begin(const double *dev_omega, int64_t l, int64_t r, double rcond, double *dev_pinv, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(dev_omega && dev_pinv, "ttsk_pinv: NULL argument");
    TTSK_ARG(l >= 1 && r >= 1, "ttsk_pinv: bad shape (%lld, %lld)", (long long)l, (long long)r);
    TTSK_ARG((r >= l ? l : r) <= 1024, "ttsk_pinv: min(l, r) = %lld > 1024 unsupported", (long long)(r >= l ? l : r));
    g_pinv_began[stream] = 0;
    if (pinv_fast(l, r, rcond)) {
        const int fr = pinv_cholesky_begin(dev_omega, l, r, dev_pinv, stream, st);
        if (fr < 0) return fr;
        g_pinv_began[stream] = fr;
    }
    return TTSK_OK;
}

int ttsk_pinv_end(const double *dev_omega, int64_t l, int64_t r, double rcond, double *dev_pinv,
                  int *host_rank, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(dev_omega && dev_pinv, "ttsk_pinv: NULL argument");
    TTSK_ARG(l >= 1 && r >= 1, "ttsk_pinv: bad shape (%lld, %lld)", (long long)l, (long long)r);
    const int transposed = r >= l;
    const int64_t mW = transposed ? r : l, nW = transposed ? l : r;
    TTSK_ARG(nW <= 1024, "ttsk_pinv: min(l, r) = %lld > 1024 unsupported", (long long)nW);
    rcond = pinv_rcond(l, r, rcond);
    const int *predicate = nullptr;
    if (g_pinv_began[stream]) {
        g_pinv_began[stream] = 0;
        if (!host_rank) {
            // nobody waits for the rank: the Jacobi kernel is queued behind the attempt and returns at once if the
            // attempt was accepted -- no read-back, the stream keeps running (to_tt: d - 1 of these per call)
            predicate = pinv_dev_status(stream);
        } else {
            const int fr = pinv_cholesky_verdict(l, r, stream, st);
            if (fr < 0) return fr;
            if (fr == 1) {
                *host_rank = (int)(l < r ? l : r);
                return TTSK_OK;
            }
        }
    }
    const size_t ws_elems = (size_t)(mW * nW + nW * nW) + 1;
    double *ws = (double *)scratch(stream, SCRATCH_MISC, ws_elems * 8);
    if (!ws) return TTSK_ERR_HIP;
    int *drank = (int *)(ws + mW * nW + nW * nW);
    if (int rc = launch_jacobi(1, dev_omega, l, r, transposed, ws, ws + mW * nW, rcond, dev_pinv, host_rank ? drank : nullptr, nullptr,
                               nullptr, nullptr, predicate, 0, 0, st)) return rc;
    if (host_rank) {
        TTSK_HIP(hipMemcpyAsync(host_rank, drank, sizeof(int), hipMemcpyDeviceToHost, st));
        TTSK_HIP(hipStreamSynchronize(st));
    }
    return TTSK_OK;
}

int ttsk_pinv_batch(int count, const double *const *dev_omegas, int64_t l, int64_t r, double *const *dev_pinvs, int stream)
{
    return pinv_batch("ttsk_pinv_batch", count, dev_omegas, l, r, dev_pinvs, stream, false);
}

int ttsk_pinv_batch_deferred(int count, const double *const *dev_omegas, int64_t l, int64_t r, double *const *dev_pinvs, int stream)
{
    return pinv_batch("ttsk_pinv_batch_deferred", count, dev_omegas, l, r, dev_pinvs, stream, true);
}

int ttsk_pinv(const double *dev_omega, int64_t l, int64_t r, double rcond, double *dev_pinv,
              int *host_rank, int stream)
{
    const int rc = ttsk_pinv_begin(dev_omega, l, r, rcond, dev_pinv, stream);
    if (rc != TTSK_OK) return rc;
    return ttsk_pinv_end(dev_omega, l, r, rcond, dev_pinv, host_rank, stream);
}

// One orthogonalisation step of orthogonal_sketch / hmt_sketch (sketch_dispatch.py:160-174) as ONE call without a
// read-back: Q = qr_thin(Psi_mat pinv(Omega)) (Omega == NULL: qr_thin(Psi_mat)) through the normal equations and
// CholeskyQR2.  The verdicts of the factorisations (Omega not of full rank / too ill conditioned, Psi_mat Omega^+ too
// ill conditioned) are NOT waited for: a rejection sets the stream's deferred flag and the numbers in Q are then
// meaningless; the caller reads the flag once at the end (ttsk_deferred_status) and repeats the sketch on the robust
// kernels (ttsk_pinv / ttsk_qr_thin).  TTSK_ERR_UNSUPPORTED: ranks beyond 256.
int ttsk_orth_step(const double *dev_psi, int64_t m, int64_t r2, const double *dev_omega, int64_t l, double *dev_q, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(dev_psi && dev_q && m >= 1 && r2 >= 1, "ttsk_orth_step: bad argument");
    const int64_t k = dev_omega ? l : r2;
    TTSK_ARG(k >= 1 && m >= k, "ttsk_orth_step: cannot orthogonalise a %lld x %lld unfolding", (long long)m, (long long)k);
    int *sticky = deferred_flag(stream);
    const int64_t nmin = dev_omega ? (l < r2 ? l : r2) : 0;
    if (!sticky || k > CHOL_MAX_N || nmin > CHOL_MAX_N || (dev_omega && !pinv_fast(l, r2))) {
        set_error("ttsk_orth_step: (%lld x %lld, rank %lld) is outside the fast path", (long long)m, (long long)r2, (long long)k);
        return TTSK_ERR_UNSUPPORTED;
    }
    const size_t pw = dev_omega ? pinv_ws_elems((int)nmin, l > r2 ? l : r2) + (size_t)r2 * l : 0;
    double *ws = (double *)scratch(stream, SCRATCH_MISC, (pw + qr_ws_elems(m, (int)k)) * 8);
    if (!ws) return TTSK_ERR_HIP;
    int rc;
    if (dev_omega) {
        double *pinv = ws + pinv_ws_elems((int)nmin, l > r2 ? l : r2);
        rc = pinv_cholesky_begin(dev_omega, l, r2, pinv, stream, st, ws, sticky);
        if (rc < 0) return rc;
        if (rc == 0) { set_error("ttsk_orth_step: pseudo-inverse outside the fast path"); return TTSK_ERR_UNSUPPORTED; }
        if ((rc = gemm_plain(m, l, r2, dev_psi, r2, 1, pinv, l, 1, dev_q, stream))) return rc;      // M = Psi_mat Omega^+
    } else if (dev_q != dev_psi) {
        TTSK_HIP(hipMemcpyAsync(dev_q, dev_psi, (size_t)m * r2 * 8, hipMemcpyDeviceToDevice, st));
    }
    rc = qr_cholesky(dev_q, m, k, stream, st, ws + pw, sticky);
    if (rc < 0) return rc;
    if (rc == 0) { set_error("ttsk_orth_step: QR outside the fast path"); return TTSK_ERR_UNSUPPORTED; }
    return TTSK_OK;
}

// ttsk_orth_step with the pseudo-inverse already made (ttsk_pinv_batch_deferred): Q = qr_thin(Psi_mat P), P (r2, l)
int ttsk_orth_step_pinv(const double *dev_psi, int64_t m, int64_t r2, const double *dev_pinv, int64_t l, double *dev_q, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(dev_psi && dev_pinv && dev_q && m >= 1 && r2 >= 1 && l >= 1, "ttsk_orth_step_pinv: bad argument");
    TTSK_ARG(m >= l, "ttsk_orth_step_pinv: cannot orthogonalise a %lld x %lld unfolding", (long long)m, (long long)l);
    int *sticky = deferred_flag(stream);
    if (!sticky || l > CHOL_MAX_N) {
        set_error("ttsk_orth_step_pinv: rank %lld is outside the fast path", (long long)l);
        return TTSK_ERR_UNSUPPORTED;
    }
    double *ws = (double *)scratch(stream, SCRATCH_DRIVER, qr_ws_elems(m, (int)l) * 8);      // (the pinvs may live in SCRATCH_MISC)
    if (!ws) return TTSK_ERR_HIP;
    int rc;
    if ((rc = gemm_plain(m, l, r2, dev_psi, r2, 1, dev_pinv, l, 1, dev_q, stream))) return rc;      // M = Psi_mat Omega^+
    rc = qr_cholesky(dev_q, m, l, stream, st, ws, sticky);
    if (rc < 0) return rc;
    if (rc == 0) { set_error("ttsk_orth_step_pinv: QR outside the fast path"); return TTSK_ERR_UNSUPPORTED; }
    return TTSK_OK;
}

// 1 in *host_flag if a fast-path factorisation queued on `stream` by ttsk_orth_step was rejected since the last call
// (waits for the stream; clears the flag)
int ttsk_deferred_status(int stream, int *host_flag)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(host_flag, "ttsk_deferred_status: NULL argument");
    int *sticky = deferred_flag(stream);
    TTSK_ARG(sticky, "ttsk_deferred_status: no device flag");
    // through a pinned word: a copy into the caller's pageable int is staged and blocks for ~40 us before the reset is
    // even queued
    int *pinned = (int *)persistent_alloc(PA_DEFERRED_PINNED, TTSK_NUM_STREAMS * sizeof(int), true, false);
    int *dst = pinned ? pinned + stream : host_flag;
    TTSK_HIP(hipMemcpyAsync(dst, sticky, sizeof(int), hipMemcpyDeviceToHost, st));
    TTSK_HIP(hipMemsetAsync(sticky, 0, sizeof(int), st));
    TTSK_HIP(hipStreamSynchronize(st));
    if (pinned) *host_flag = *dst;
    return TTSK_OK;
}

}  // extern "C"
