// Host side of the Psi product kernels (stream_small.h): their instantiations, the launchers that carry out the plans of
// psi_plan.h, and the two C entry points that reach the kernels directly.
#include <cstdlib>
#include "stream_small.h"
#include "prof.h"

namespace ttsk {

static int launch_ss(const StreamSmall &a, int nf, int str, int unr, size_t lds, int grid, hipStream_t st)
{
#define TTSK_SS_CASE(NF, STR) if (nf == NF && str == STR) return launch(unr == 25 ? stream_small_kernel<NF, STR, 5, 25> : stream_small_kernel<NF, STR, 5, 5>, dim3((unsigned)grid), dim3(512), lds, st, a);
    PSI_STREAM_STRUCTURES(TTSK_SS_CASE)
#undef TTSK_SS_CASE
    return 1;
}

int stream_small_try(const StreamSmallArgs &c, int stream, hipStream_t st, int cus)
{
    (void)stream;
    PsiStreamPlan p;
    const int ok = psi_stream_plan(c, cus > 0 ? cus : device_num_cu(), p);
    if (ok != 1) return ok;
    ProfBracket prof(st, PROF_CURRENT, p.l.flops, "%s", p.l.name);
    const int rc = launch_ss(p.a, p.nf, p.str, p.unr, p.l.lds, p.l.grid, st);
    return rc == TTSK_OK ? 1 : (rc == 1 ? 0 : rc);
}

static int launch_sss(const StreamSmallSum &a, int nf, int str, int unr, size_t lds, int grid, hipStream_t st)
{
#define TTSK_SSS_CASE(NF, STR) if (nf == NF && str == STR) return launch(unr == 25 ? stream_small_sum_kernel<NF, STR, 5, 25> : stream_small_sum_kernel<NF, STR, 5, 5>, dim3((unsigned)grid), dim3(512), lds, st, a);
    PSI_STREAM_SUM_STRUCTURES(TTSK_SSS_CASE)
#undef TTSK_SSS_CASE
    return 1;
}

int stream_small_sum_try(const StreamSmallSumArgs &c, int stream, hipStream_t st, int cus)
{
    (void)stream;
    PsiStreamSumPlan p;
    const int ok = psi_stream_sum_plan(c, cus > 0 ? cus : device_num_cu(), p);
    if (ok != 1) return ok;
    ProfBracket prof(st, PROF_CURRENT, p.l.flops, "%s", p.l.name);
    const int rc = launch_sss(p.a, p.nf, p.str, p.unr, p.l.lds, p.l.grid, st);
    return rc == TTSK_OK ? 1 : (rc == 1 ? 0 : rc);
}

}  // namespace ttsk

using namespace ttsk;

extern "C" int ttsk_psi_stream(int nb, int J, int K1, int A, const double *const *S, int64_t s_j, const double *const *W,
                               int64_t w_c, double *const *C, int64_t c_j, int accumulate, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(S && W && C, "ttsk_psi_stream: NULL argument");
    for (int b = 0; b < nb && b < SK_MAXB; ++b) TTSK_ARG(S[b] && W[b] && C[b], "ttsk_psi_stream: NULL operand of problem %d", b);
    const StreamSmallArgs c{nb, J, K1, A, S, s_j, W, w_c, C, c_j, accumulate};
    const int rc = stream_small_try(c, stream, st);
    if (rc == 0) {
        set_error("ttsk_psi_stream: shape (nb=%d J=%d K1=%d A=%d s_j=%lld w_c=%lld c_j=%lld) is not covered by the streamed kernel", nb, J, K1,
                  A, (long long)s_j, (long long)w_c, (long long)c_j);
        return TTSK_ERR_UNSUPPORTED;
    }
    return rc < 0 ? rc : TTSK_OK;
}

extern "C" int ttsk_psi_stream_sum(int nb, int J, int K1, int A, const double *S, int64_t s_j, int64_t s_b, const double *W,
                                   int64_t w_c, int64_t w_b, double *C, int64_t c_j, int accumulate, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(S && W && C, "ttsk_psi_stream_sum: NULL argument");
    const StreamSmallSumArgs c{nb, J, K1, A, S, s_j, s_b, W, w_c, w_b, C, c_j, accumulate};
    const int rc = stream_small_sum_try(c, stream, st);
    if (rc == 0) {
        set_error("ttsk_psi_stream_sum: shape (nb=%d J=%d K1=%d A=%d s_j=%lld s_b=%lld w_c=%lld w_b=%lld c_j=%lld) is not covered by the "
                  "summing streamed kernel", nb, J, K1, A, (long long)s_j, (long long)s_b, (long long)w_c, (long long)w_b, (long long)c_j);
        return TTSK_ERR_UNSUPPORTED;
    }
    return rc < 0 ? rc : TTSK_OK;
}
