// Host side of the chunked fused chain step (chain_wide.h).  What is launched is decided by chain_wide_plan (chain_plan.h,
// plain C++, checked on the host by tests/test_chain_plan.py); left here: the slab request, the profiling bracket, the pick
// of the instantiation file, the launch and the closing slab reduce.
#include "chain_wide.h"
#include "prof.h"

namespace ttsk {

#define TTSK_CW_DECL(T) \
    int launch_chain_wide_##T(const ChainWide &a, int nn, int sn, bool wt, int unr, size_t lds, int grid, hipStream_t st);
TTSK_CW_DECL(0a) TTSK_CW_DECL(0b) TTSK_CW_DECL(1a) TTSK_CW_DECL(1b) TTSK_CW_DECL(2a) TTSK_CW_DECL(2b) TTSK_CW_DECL(3a)
TTSK_CW_DECL(3b) TTSK_CW_DECL(4a) TTSK_CW_DECL(4b) TTSK_CW_DECL(5a) TTSK_CW_DECL(5b) TTSK_CW_DECL(6a) TTSK_CW_DECL(6b)
#undef TTSK_CW_DECL

static int launch_chain_wide(int ci, const ChainWide &a, int nn, int sn, bool wt, int unr, size_t lds, int grid, hipStream_t st)
{
    const bool lo = nn <= 4;
    switch (ci) {
    case 0: return lo ? launch_chain_wide_0a(a, nn, sn, wt, unr, lds, grid, st) : launch_chain_wide_0b(a, nn, sn, wt, unr, lds, grid, st);
    case 1: return lo ? launch_chain_wide_1a(a, nn, sn, wt, unr, lds, grid, st) : launch_chain_wide_1b(a, nn, sn, wt, unr, lds, grid, st);
    case 2: return lo ? launch_chain_wide_2a(a, nn, sn, wt, unr, lds, grid, st) : launch_chain_wide_2b(a, nn, sn, wt, unr, lds, grid, st);
    case 3: return lo ? launch_chain_wide_3a(a, nn, sn, wt, unr, lds, grid, st) : launch_chain_wide_3b(a, nn, sn, wt, unr, lds, grid, st);
    case 4: return lo ? launch_chain_wide_4a(a, nn, sn, wt, unr, lds, grid, st) : launch_chain_wide_4b(a, nn, sn, wt, unr, lds, grid, st);
    case 5: return lo ? launch_chain_wide_5a(a, nn, sn, wt, unr, lds, grid, st) : launch_chain_wide_5b(a, nn, sn, wt, unr, lds, grid, st);
    default: return lo ? launch_chain_wide_6a(a, nn, sn, wt, unr, lds, grid, st) : launch_chain_wide_6b(a, nn, sn, wt, unr, lds, grid, st);
    }
}

int chain_wide_try(const ChainStepArgs &c, int stream, hipStream_t st, bool force, int cus)
{
    const int n_cu = device_num_cu();
    if (n_cu < 1) return TTSK_ERR_HIP;
    ChainWidePlan p;
    if (!chain_wide_plan(c, cus > 0 ? cus : n_cu, force, p)) return 0;
    ChainWide &a = p.a;
    a.slab = chain_slab_request(stream, p.l);
    if (!a.slab) return TTSK_ERR_HIP;
    ProfBracket prof(st, PROF_CURRENT, p.l.flops,
                     "chain_wide_kernel<%d, %d, %d, %d, %s, %d, %s>", CW_NQ[p.ci], CW_SQ[p.ci], p.nn, p.sn, p.wt ? "true" : "false", p.unr,
                     p.mt2 ? "true" : "false");
    int rc = launch_chain_wide(p.ci, a, p.nn, p.sn, p.wt, p.unr, p.l.lds, p.l.grid, st);
    if (rc == TTSK_OK) rc = chain_slab_reduce(st, a.slab, p.l, c);
    return rc == TTSK_OK ? 1 : (rc == 1 ? 0 : rc);
}

}  // namespace ttsk

using namespace ttsk;

extern "C" int ttsk_chain_step_wide(int nb, int n, int K1, int A, int A2, int J, const double *const *W, int64_t w_c,
                                    const double *const *X, int64_t x_j, int64_t x_k, int64_t x_c, int64_t x_extent,
                                    const double *E, double *const *T, double *const *Out, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(W && X && E && Out && nb >= 1, "ttsk_chain_step_wide: NULL argument");
    ChainStepArgs c{nb, n, K1, A, A2, J, W, w_c, X, x_j, x_k, x_c, x_extent, E, T, Out};
    const int rc = chain_wide_try(c, stream, st, true);
    if (rc == 0) {
        set_error("ttsk_chain_step_wide: shape (n=%d K1=%d A=%d A2=%d J=%d nb=%d) is not covered by the chunked fused kernel", n, K1,
                  A, A2, J, nb);
        return TTSK_ERR_UNSUPPORTED;
    }
    return rc < 0 ? rc : TTSK_OK;
}
