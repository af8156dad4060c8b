// Host side of the fused chain step (chain_fused.h).  What is launched is decided by chain_fused_plan (chain_plan.h, plain
// C++, checked on the host by tests/test_chain_plan.py); left here: the slab request, the profiling bracket, the lab hooks,
// the pick of the instantiation file, the launch and the closing slab reduce.
#include <cstdlib>
#include "chain_fused.h"
#include "prof.h"

namespace ttsk {

int launch_chain_step_a(const ChainStep &a, int nf, int str, bool wt, int ebuf, int unr, int waves, size_t lds, int grid, hipStream_t st);
int launch_chain_step_b(const ChainStep &a, int nf, int str, bool wt, int ebuf, int unr, int waves, size_t lds, int grid, hipStream_t st);
int launch_chain_step_c(const ChainStep &a, int nf, int str, bool wt, int ebuf, int unr, int waves, size_t lds, int grid, hipStream_t st);
int launch_chain_step_d(const ChainStep &a, int nf, int str, bool wt, int ebuf, int unr, int waves, size_t lds, int grid, hipStream_t st);
int launch_chain_step_e(const ChainStep &a, int nf, int str, bool wt, int ebuf, int unr, int waves, size_t lds, int grid, hipStream_t st);

static int launch_chain_step(const ChainStep &a, int nf, int str, bool wt, int ebuf, int unr, int waves, size_t lds, int grid, hipStream_t st)
{
    if (nf <= 2) return launch_chain_step_a(a, nf, str, wt, ebuf, unr, waves, lds, grid, st);
    if (nf <= 4) return launch_chain_step_b(a, nf, str, wt, ebuf, unr, waves, lds, grid, st);
    if (nf == 5) return launch_chain_step_c(a, nf, str, wt, ebuf, unr, waves, lds, grid, st);
    if (nf == 6) return launch_chain_step_d(a, nf, str, wt, ebuf, unr, waves, lds, grid, st);
    return launch_chain_step_e(a, nf, str, wt, ebuf, unr, waves, lds, grid, st);
}

int chain_fused_try(const ChainStepArgs &c, int stream, hipStream_t st, bool force, int cus)
{
    const int n_cu = device_num_cu();
    if (n_cu < 1) return TTSK_ERR_HIP;
    ChainFusedPlan p;
    if (!chain_fused_plan(c, cus > 0 ? cus : n_cu, force, p)) return 0;
    ChainStep &a = p.a;
    a.slab = chain_slab_request(stream, p.l);
    if (!a.slab) return TTSK_ERR_HIP;
    a.Epk = drm_packed_lookup(c.E, c.A, c.n, c.A2, a.A2P, a.eunits);
    // flops of BOTH products of the step (the pair this kernel replaces), reduce launch inside the bracket; the name as
    // profiles/*_traffic.json is keyed by it: the nine parameters from before the deal (no NWV), NN / SN given as NQ / SQ
    ProfBracket prof(st, PROF_CURRENT, p.l.flops,
                     "chain_step_kernel<%d, %d, %d, %d, 5, %s, 1, %d, %d>", p.nq, p.sq, p.nq, p.sq, p.wt ? "true" : "false", p.ebuf, p.unr);
#ifdef TTSK_LAB
    { static int dg = [] { const char *e = getenv("TTSK_CF_DIAG"); return e ? atoi(e) : 0; }(); a.diag = dg; }
    static int stamps_on = [] { const char *e = getenv("TTSK_CF_STAMPS"); return e ? atoi(e) : 0; }();
#else
    constexpr int stamps_on = 0;
#endif
    long long *stamps_dev = nullptr;
    if (stamps_on) {
        if (hipMalloc(&stamps_dev, 8 * CD_WAVES * 8 * 8) != hipSuccess) return TTSK_ERR_HIP;
        (void)hipMemset(stamps_dev, 0, 8 * CD_WAVES * 8 * 8);
        a.stamps = stamps_dev;
    }
    int rc = launch_chain_step(a, p.nq, p.sq, p.wt, p.ebuf, p.unr, p.waves, p.l.lds, p.l.grid, st);
    if (stamps_on) {
        long long h[8 * CD_WAVES * 8];
        (void)hipStreamSynchronize(st);
        (void)hipMemcpy(h, stamps_dev, sizeof(h), hipMemcpyDeviceToHost);
        (void)hipFree(stamps_dev);
        long long t0 = 0;
        for (int i = 0; i < 8 * CD_WAVES * 8; ++i) if (h[i] && (!t0 || h[i] < t0)) t0 = h[i];
        fprintf(stderr, "[cf stamps] workgroup 0: cycles since its first stamp; per slice, wave: start | endA | afterB1 | endB | afterB2\n");
        for (int sl = 0; sl < 8; ++sl)
            for (int w = 0; w < CD_WAVES; ++w) {
                const long long *r = h + (sl * CD_WAVES + w) * 8;
                if (!r[1] && !r[4]) continue;
                fprintf(stderr, "  slice %d wave %d: %8lld %8lld %8lld %8lld %8lld\n", sl, w, r[0] ? r[0] - t0 : -1, r[1] - t0, r[2] - t0,
                        r[3] - t0, r[4] - t0);
            }
    }
    if (rc == TTSK_OK) rc = chain_slab_reduce(st, a.slab, p.l, c);
    return rc == TTSK_OK ? 1 : (rc == 1 ? 0 : rc);
}

}  // namespace ttsk

using namespace ttsk;

extern "C" int ttsk_chain_step(int nb, int n, int K1, int A, int A2, int J, const double *const *W, int64_t w_c,
                               const double *const *X, int64_t x_j, int64_t x_k, int64_t x_c, int64_t x_extent,
                               const double *E, double *const *T, double *const *Out, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(W && X && E && Out && nb >= 1, "ttsk_chain_step: NULL argument");
    ChainStepArgs c{nb, n, K1, A, A2, J, W, w_c, X, x_j, x_k, x_c, x_extent, E, T, Out};
    const int rc = chain_fused_try(c, stream, st, true);
    if (rc == 0) {
        set_error("ttsk_chain_step: shape (n=%d K1=%d A=%d A2=%d J=%d nb=%d) is not covered by the fused kernel", n, K1, A,
                  A2, J, nb);
        return TTSK_ERR_UNSUPPORTED;
    }
    return rc < 0 ? rc : TTSK_OK;
}
