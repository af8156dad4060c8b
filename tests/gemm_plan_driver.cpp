// Driver of tests/test_gemm_plan.py: reads calls, one per line, and prints every non-pointer field of what gemm_route and the
// plans of csrc/gemm_plan.h decide, and for pointer tables which of the tables handed in they equal.  Host compiler only.
//
//   <id> route  <n_cu> <desc: 16 extents and strides> <acc> <split_k> <k_scale?> <A> <B> <C> <nb> <tA> <tB> <tC> <alpha>
//   <id> batch  ... the same: nb problems at X + 8 b tX through skinny_r_plan, skinny_s_plan, small_gemm_plan in that order
//   <id> reduce <n_cu> <chunks> <M> <N> <m_tiles> <nprob> <Mtot> <c_m> <c_n> <slab> <C> <tC>
//
// What follows " ;; " on a line are a plan's own intermediate decisions (no launcher before gemm_plan.h showed them).
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "gemm_plan.h"
using namespace ttsk;

static const double *tA[SK_MAXB], *tB[SK_MAXB];
static double *tC[SK_MAXB];
static int t_nb;

template <typename T, typename U> static char which(T *const *got, int n, U *const *a, U *const *b)
{
    bool ia = true, ib = true;
    for (int i = 0; i < SK_MAXB; ++i) {
        ia &= got[i] == (i < n ? a[i] : nullptr);
        ib &= got[i] == (i < n ? b[i] : nullptr);
    }
    return ia ? 'a' : ib ? 'b' : 'x';
}

static void put_reduce(const RReduceArgs &r, int nprob)
{
    const RReducePlan q = r_reduce_plan((const double *)4096, r);
    printf(" red=%d,%d,%d,%d,%d,%lld,%lld,%lld,%.17g,%d redC=%c rvariant=%d rgrid=%u,%u rblock=%d", r.chunks, r.M, r.N, r.m_tiles, r.nprob,
           (long long)r.Mtot, (long long)r.c_m, (long long)r.c_n, r.alpha, r.accumulate, which(r.out.C, nprob, tC, tC), q.variant, q.gx, q.gy,
           q.block);
}

static void put_r(const SkinnyRPlan &p)
{
    const SkinnyR &r = p.r;
    printf(" fam=skinny_r name=skinny_r_kernel<%d,%d,4> unit=%d grid=%d block=%d scratch=%zu work=%.17g nb=%d chunks=%d a_ko=%lld a_ki=%lld b_ko=%lld"
           " b_ki=%lld Ki=%lld K=%lld chunk=%lld a_extent=%lld b_extent=%lld M=%d N=%d m_tiles=%d rebase=%d Mtot=%lld a_gen=%d b_gen=%d a_m=%lld"
           " b_n=%lld tabA=%c tabB=%c slab=%d",
           p.nmt, p.nnt, p.unit, p.grid, p.block, p.scratch_bytes, p.work, r.nb, r.chunks, (long long)r.a_ko, (long long)r.a_ki, (long long)r.b_ko,
           (long long)r.b_ki, (long long)r.Ki, (long long)r.K, (long long)r.chunk, (long long)r.a_extent, (long long)r.b_extent, r.M, r.N, r.m_tiles,
           r.rebase, (long long)r.Mtot, r.a_gen, r.b_gen, (long long)r.a_m, (long long)r.b_n, which(r.A, r.nb, tA, tB), which(r.B, r.nb, tA, tB),
           r.slab != nullptr);
    put_reduce(p.red, r.nb);
    printf(" ;; swap=%d a_pair=%d b_pair=%d gk=%d nsub=%d", p.swap, p.a_pair, p.b_pair, p.gk, p.nsub);
}

static void put_s(const SkinnySPlan &p)
{
    const SkinnyS &s = p.s;
    printf(" fam=skinny_s name=skinny_s_kernel<%d,%d,%d,%d> grid=%d block=%d lds=%zu work=%.17g nb=%d wpp=%d w_k=%lld w_m=%lld s_j=%lld s_k=%lld"
           " s_u=%lld U=%d V=%d nbv=%d tvl=%d c_m=%lld c_j=%lld c_u=%lld J=%lld P=%d K=%d groups=%d s_extent=%lld w_extent=%lld c_extent=%lld"
           " alpha=%.17g acc=%d big=%d tabW=%c tabS=%c tabC=%c",
           p.npt, p.spt, p.dring, p.str, p.grid, p.block, p.lds, p.work, s.nb, s.wpp, (long long)s.w_k, (long long)s.w_m, (long long)s.s_j,
           (long long)s.s_k, (long long)s.s_u, s.U, s.V, s.nbv, s.tvl, (long long)s.c_m, (long long)s.c_j, (long long)s.c_u, (long long)s.J, s.P, s.K,
           s.groups, (long long)s.s_extent, (long long)s.w_extent, (long long)s.c_extent, s.alpha, s.accumulate, s.big, which(s.W, s.nb, tA, tB),
           which(s.S, s.nb, tA, tB), which(s.C, s.nb, tC, tC));
    printf(" ;; a_small=%d", p.a_small);
}

static void put_small(const SmallGemmPlan &p, const ttsk_gemm_desc &d)
{
    const SmallG &g = p.g;
    // a uniformly strided batch: the plan spreads the one triple over the table
    const double *xa[SK_MAXB] = {}, *xb[SK_MAXB] = {};
    double *xc[SK_MAXB] = {};
    for (int b = 0; b < g.nb; ++b) {
        xa[b] = d.batch > 1 ? tA[0] + b * d.a_b : tA[b];
        xb[b] = d.batch > 1 ? tB[0] + b * d.b_b : tB[b];
        xc[b] = d.batch > 1 ? tC[0] + b * d.c_b : tC[b];
    }
    printf(" fam=small name=%s grid=%u block=%d work=%.17g nb=%d M=%d N=%d K=%d tiles_m=%d tiles_n=%d a_m=%lld a_k=%lld b_k=%lld b_n=%lld c_m=%lld"
           " c_n=%lld a_extent=%lld b_extent=%lld c_extent=%lld alpha=%.17g acc=%d tabA=%c tabB=%c tabC=%c",
           p.name, p.grid, p.block, p.work, g.nb, g.M, g.N, g.K, g.tiles_m, g.tiles_n, (long long)g.a_m, (long long)g.a_k, (long long)g.b_k,
           (long long)g.b_n, (long long)g.c_m, (long long)g.c_n, (long long)g.a_extent, (long long)g.b_extent, (long long)g.c_extent, g.alpha,
           g.accumulate, which(g.A, g.nb, xa, xa), which(g.B, g.nb, xb, xb), which(g.C, g.nb, xc, xc));
    printf(" ;; ksplit=%d", p.ksplit);
}

static void put_rows(const RowsLongkPlan &p)
{
    const RightPass &a = p.a;
    printf(" fam=rows_longk name=%s grid=%u block=%d lds=%zu scratch=%zu work=%.17g rows=%lld s_row=%lld b_row=%lld K=%lld N=%d nrb=%d nkc=%d S=%d B=%d"
           " slab=%d",
           p.name, p.grid, p.block, p.lds, p.scratch_bytes, p.work, (long long)a.rows, (long long)a.s_row, (long long)a.b_row, (long long)a.K, a.N,
           a.nrb, a.nkc, a.S == tA[0], a.B == tB[0], a.slab != nullptr);
    put_reduce(p.red, 1);
}

static void put_tiles(const GemmTilePlan &p, const double *A, const double *B, double *C, bool ks)
{
    const GemmLaunch &g = p.g;
    const ttsk_gemm_desc &d = g.d;
    printf(" fam=tiles name=gemm_f64_kernel<%d,%d,%d,%d,%s,%s> grid=%u,%u,%u block=256 lds=%zu scratch=%zu work=%.17g family=%d tiles=%d splits=%d"
           " avec=%d bvec=%d fast_ok=%d kchunk=%lld bm=%d bn=%d a_extent=%lld b_extent=%lld"
           " d=%lld,%lld,%lld,%lld,%lld|%lld,%lld,%lld,%lld|%lld,%lld,%lld,%lld|%lld,%lld,%lld|%.17g,%d,%d ptrs=%d partial=%d",
           p.wm, p.wn, p.tm, p.tn, p.ak ? "true" : "false", p.bk ? "true" : "false", g.gx, g.gy, g.gz, g.lds, p.partial_bytes, p.work, g.family, g.tiles,
           g.splits, g.avec, g.bvec, g.fast_ok, (long long)g.kchunk, g.bm, g.bn, (long long)g.a_extent, (long long)g.b_extent, (long long)d.batch,
           (long long)d.M, (long long)d.N, (long long)d.Ko, (long long)d.Ki, (long long)d.a_b, (long long)d.a_m, (long long)d.a_ko, (long long)d.a_ki,
           (long long)d.b_b, (long long)d.b_ko, (long long)d.b_ki, (long long)d.b_n, (long long)d.c_b, (long long)d.c_m, (long long)d.c_n, d.alpha,
           d.accumulate, d.split_k, g.A == A && g.B == B && g.C == C && (g.ks != nullptr) == ks, g.partial != nullptr);
    if (p.partial_bytes) printf(" sred=%u,%lld,%lld,%d", p.red_grid, (long long)p.tiles_m, (long long)p.tiles_n, p.rota);
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char id[128], kind[16];
    static GemmRoute r;
    while (fscanf(f, "%127s %15s", id, kind) == 2) {
        long long v[32];
        if (!strcmp(kind, "reduce")) {
            for (int i = 0; i < 12; ++i)
                if (fscanf(f, "%lld", &v[i]) != 1) return 3;
            RReduceArgs a{(int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], v[6], v[7], v[8], 1.0, 0, {}};
            for (int b = 0; b < a.nprob; ++b) a.out.C[b] = (double *)(uintptr_t)(v[10] + 8 * b * v[11]);
            const RReducePlan q = r_reduce_plan((const double *)(uintptr_t)v[9], a);
            printf("%s rvariant=%d rgrid=%u,%u rblock=%d |\n", id, q.variant, q.gx, q.gy, q.block);
            continue;
        }
        double alpha;
        for (int i = 0; i < 27; ++i)
            if (fscanf(f, "%lld", &v[i]) != 1) return 3;
        if (fscanf(f, "%lf", &alpha) != 1) return 3;
        const int n_cu = (int)v[0];
        ttsk_gemm_desc d{};
        d.batch = v[1]; d.M = v[2]; d.N = v[3]; d.Ko = v[4]; d.Ki = v[5];
        d.a_b = v[6]; d.a_m = v[7]; d.a_ko = v[8]; d.a_ki = v[9];
        d.b_b = v[10]; d.b_ko = v[11]; d.b_ki = v[12]; d.b_n = v[13];
        d.c_b = v[14]; d.c_m = v[15]; d.c_n = v[16];
        d.accumulate = (int)v[17]; d.split_k = (int)v[18]; d.alpha = alpha;
        const bool ks = v[19] != 0;
        const double *A = (const double *)(uintptr_t)v[20], *B = (const double *)(uintptr_t)v[21];
        double *C = (double *)(uintptr_t)v[22];
        const double *scale = ks ? (const double *)(uintptr_t)4096 : nullptr;
        const int nb = (int)v[23];
        printf("%s", id);
        if (!strcmp(kind, "batch")) {
            const double *Ap[64];
            const double *Bp[64];
            double *Cp[64];
            if (nb > 64) return 3;
            for (int b = 0; b < nb; ++b) { Ap[b] = A + b * v[24]; Bp[b] = B + b * v[25]; Cp[b] = C + b * v[26]; }
            t_nb = nb < SK_MAXB ? nb : SK_MAXB;
            memset(tA, 0, sizeof(tA)); memset(tB, 0, sizeof(tB)); memset(tC, 0, sizeof(tC));
            for (int b = 0; b < t_nb; ++b) { tA[b] = Ap[b]; tB[b] = Bp[b]; tC[b] = Cp[b]; }
            if (skinny_r_plan(d, nb, Ap, Bp, Cp, n_cu, &r.sr) == 1) put_r(r.sr);
            else if (skinny_s_plan(d, nb, Ap, Bp, Cp, n_cu, &r.ss) == 1) put_s(r.ss);
            else if (small_gemm_plan(d, nb, Ap, Bp, Cp, &r.sm) == 1) put_small(r.sm, d);
            else printf(" fam=none");
            printf(" |\n");
            continue;
        }
        const int rc = gemm_route(d, A, B, C, scale, n_cu, &r);
        printf(" rc=%d", rc);
        if (rc) { printf(" | %s\n", r.msg); continue; }
        memset(tA, 0, sizeof(tA)); memset(tB, 0, sizeof(tB)); memset(tC, 0, sizeof(tC));
        tA[0] = A; tB[0] = B; tC[0] = C;
        int launches = 1, fallback = 0;
        if (r.kind == GEMM_LONGK_BATCH) {
            // ttsk_gemm's loop over the slice groups behind the first one: every group must be accepted like the first
            launches = 0;
            for (int64_t b0 = 0; b0 < d.batch && !fallback; b0 += SK_MAXB) {
                const int cnt = (int)(d.batch - b0 < SK_MAXB ? d.batch - b0 : SK_MAXB);
                for (int b = 0; b < cnt; ++b) { tA[b] = A + (b0 + b) * d.a_b; tB[b] = B + (b0 + b) * d.b_b; tC[b] = C + (b0 + b) * d.c_b; }
                for (int b = cnt; b < SK_MAXB; ++b) { tA[b] = tB[b] = nullptr; tC[b] = nullptr; }
                static SkinnyRPlan later;
                static SkinnySPlan later_s;
                if (b0 == 0) { ++launches; continue; }
                if (skinny_r_plan(r.n, cnt, tA, tB, tC, n_cu, &later) == 1 || skinny_s_plan(r.n, cnt, tA, tB, tC, n_cu, &later_s) == 1) ++launches;
                else fallback = 1;
            }
            const int cnt = (int)(d.batch < SK_MAXB ? d.batch : SK_MAXB);
            for (int b = 0; b < SK_MAXB; ++b) {
                tA[b] = b < cnt ? A + b * d.a_b : nullptr; tB[b] = b < cnt ? B + b * d.b_b : nullptr; tC[b] = b < cnt ? C + b * d.c_b : nullptr;
            }
        }
        const char *route[] = {"empty", "k0", "rows_longk", "skinny_r", "skinny_s", "small", "longk_batch", "tiles"};
        printf(" route=%s launches=%d fallback=%d", route[r.kind], r.kind <= GEMM_K0 ? 0 : launches, fallback);
        switch (r.kind) {
        case GEMM_ROWS_LONGK: put_rows(r.rl); break;
        case GEMM_SKINNY_R: case GEMM_LONGK_BATCH: put_r(r.sr); break;
        case GEMM_SKINNY_S: put_s(r.ss); break;
        case GEMM_SMALL: put_small(r.sm, r.n); break;
        case GEMM_TILES: put_tiles(r.g, A, B, C, ks); break;
        default: break;
        }
        printf(" |\n");
    }
    return 0;
}
