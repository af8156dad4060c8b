// Host side of the stacked-terms chain step (chain_sum.h).  What is launched -- the table that deals the work of the second
// product over the eight waves included -- is decided by chain_sum_plan (chain_plan.h, plain C++, checked on the host by
// tests/test_chain_plan.py); left here: the slab request, the profiling bracket, the lab hooks, the launch and the closing
// slab reduce.
#include <cstdlib>
#include "chain_sum.h"
#include "prof.h"

namespace ttsk {

int chain_sum_try(const ChainSumArgs &cc, int stream, hipStream_t st, bool force, int cus)
{
    const ChainStepArgs &c = cc.s;
    const int n_cu = device_num_cu();
    if (n_cu < 1) return TTSK_ERR_HIP;
    ChainSumPlan p;
    if (!chain_sum_plan(cc, cus > 0 ? cus : n_cu, force, p)) return 0;
    ChainSum &ka = p.ka;
    ChainSumS &a = ka.s;
    a.slab = chain_slab_request(stream, p.l);
    if (!a.slab) return TTSK_ERR_HIP;
    ProfBracket prof(st, PROF_CURRENT, p.l.flops,
                     "chain_sum_kernel<5, 5, NA, %s>", p.wt ? "true" : "false");
#ifdef TTSK_LAB
    { static int dg = [] { const char *e = getenv("TTSK_CS_DIAG"); return e ? atoi(e) : 0; }(); a.diag = dg; }
    static int stamps_on = [] { const char *e = getenv("TTSK_CS_STAMPS"); return e ? atoi(e) : 0; }();
    long long *stamps_dev = nullptr;
    if (stamps_on) {
        if (hipMalloc(&stamps_dev, 8 * 8 * 8 * 8) != hipSuccess) return TTSK_ERR_HIP;
        (void)hipMemset(stamps_dev, 0, 8 * 8 * 8 * 8);
        a.stamps = stamps_dev;
    }
#endif
    int rc = p.na_run <= 2 ? launch_chain_sum_2(ka, p.wt, p.l.lds, p.l.grid, st) : launch_chain_sum_4(ka, p.wt, p.l.lds, p.l.grid, st);
#ifdef TTSK_LAB
    if (stamps_on) {
        long long h[8 * 8 * 8];
        (void)hipStreamSynchronize(st);
        (void)hipMemcpy(h, stamps_dev, sizeof(h), hipMemcpyDeviceToHost);
        (void)hipFree(stamps_dev);
        long long t0 = 0;
        for (int i = 0; i < 8 * 8 * 8; ++i) if (h[i] && (!t0 || h[i] < t0)) t0 = h[i];
        for (int w = 0; w < 8; ++w)
            fprintf(stderr, "[cs stamps] wave %d: kernel entry -> first slice %lld cycles, last barrier -> behind the stores %lld cycles\n", w,
                    h[w * 8 + 0] - h[w * 8 + 6], h[w * 8 + 7] - h[(3 * 8 + w) * 8 + 5]);
        for (int w = 0; w < 8; ++w) {
            const long long *r = h + (4 * 8 + w) * 8, e = h[w * 8 + 6];
            fprintf(stderr, "[cs stamps] prologue wave %d: picked %lld | G issued %lld | W issued %lld | E offsets %lld | lane offsets %lld | body entered %lld | G store begins %lld | G stored %lld | barrier passed %lld | first slice %lld\n", w,
                    r[6] - e, r[0] - e, r[1] - e, r[2] - e, r[3] - e, h[(5 * 8 + w) * 8] - e, r[4] - e, r[5] - e, r[7] - e, h[w * 8 + 0] - e);
        }
        fprintf(stderr, "[cs stamps] workgroup 0, cycles since its first stamp; slice, wave (body): start | endA | dma landed | afterB1 | endB | afterB2\n");
        for (int sl = 0; sl < 4; ++sl)
            for (int w = 0; w < 8; ++w) {
                const long long *r = h + (sl * 8 + w) * 8;
                fprintf(stderr, "  slice %d wave %d (%02x): %8lld %8lld %8lld %8lld %8lld %8lld\n", sl, w, ka.role[w].body, r[0] - t0, r[1] - t0, r[2] - t0,
                        r[3] - t0, r[4] - t0, r[5] - t0);
            }
    }
#endif
    if (rc == TTSK_OK) rc = chain_slab_reduce(st, a.slab, p.l, c);
    return rc == TTSK_OK ? 1 : rc;
}

}  // namespace ttsk

using namespace ttsk;

// One chain step of nb low-rank tensor trains through the stacked-terms kernel (tests, tools).  T (optional): the
// intermediate T[b * t_b + (a * n + k) * t_ld + j], t_extent elements addressable.
extern "C" int ttsk_chain_step_sum(int nb, int n, int K1, int A, int A2, int J, const double *const *W, int64_t w_c,
                                   const double *const *X, int64_t x_j, int64_t x_k, int64_t x_c, int64_t x_extent,
                                   const double *E, double *T, int64_t t_b, int64_t t_ld, int64_t t_extent,
                                   double *const *Out, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(W && X && E && Out && nb >= 1, "ttsk_chain_step_sum: NULL argument");
    ChainSumArgs c{{nb, n, K1, A, A2, J, W, w_c, X, x_j, x_k, x_c, x_extent, E, nullptr, Out}, T, t_b, t_ld, t_extent};
    const int rc = chain_sum_try(c, stream, st, true);
    if (rc == 0) {
        set_error("ttsk_chain_step_sum: shape (n=%d K1=%d A=%d A2=%d J=%d nb=%d) is not covered by the stacked-terms kernel", n,
                  K1, A, A2, J, nb);
        return TTSK_ERR_UNSUPPORTED;
    }
    return rc < 0 ? rc : TTSK_OK;
}
