"""The host-side plans of the three chain-step kernels (csrc/chain_plan.h, plain C++): a short driver compiled with the host
compiler prints every non-pointer field of what chain_fused_plan / chain_wide_plan / chain_sum_plan decide, and that is
checked here -- before any kernel reads it.

(a) tests/golden/chain_plan_cases.json holds, for a list of calls, what the launchers of the commit before chain_plan.h
    decided (recorded from that commit's own chain_fused.hip / chain_wide.hip / chain_sum.hip, compiled for the host and
    linked against stubs that print what they are handed): verdicts with and without `force`, and for an accepted call the
    kernel-argument struct, the instantiation, LDS, grid, scratch bytes, the arguments of the slab reduce, the profiling
    bracket's name and work.  The plans must give the same, field by field.
(b) On every accepted plan of the edge list below -- the smallest shapes on either side of each branch -- the invariants
    the kernels rely on."""
import json
import os

import pytest

from tests.host_driver import ROOT, compile_driver, run_driver

FIXTURE = os.path.join(ROOT, "tests", "golden", "chain_plan_cases.json")

LIM32 = (1 << 32) - 64
LDS_MAX = 160 * 1024
N_CU = (256, 20)        # 20: fewer compute units than tensors of a batch -- the wpp / nranges clamps
CALL_KEYS = ("nb", "n", "K1", "A", "A2", "J", "w_c", "x_j", "x_k", "x_c", "x_extent", "e_off", "x_off", "t_b", "t_ld", "t_extent")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <type_traits>
#include "chain_plan.h"
using namespace ttsk;

static const ChainStepArgs *g_call;
template <typename A> static int tables_ok(const A &a, const double *E, bool with_t)
{
    int ok = E == g_call->E;
    for (int b = 0; b < SK_MAXB; ++b) {
        const bool in = b < g_call->nb;
        ok &= a.W[b] == (in ? g_call->W[b] : nullptr) && a.X[b] == (in ? g_call->X[b] : nullptr);
        if constexpr (!std::is_same<A, ChainSum>::value) ok &= a.T[b] == (in && with_t ? g_call->T[b] : nullptr);
    }
    return ok;
}
static void put_launch(const ChainLaunch &l)
{
    printf(" lds=%zu grid=%d slab=%lld red=%d,%d,%d flops=%.17g\n", l.lds, l.grid, (long long)l.slab, l.red_chunks, l.red_m, l.red_n, l.flops);
}

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    const int n_cu = atoi(argv[1]);
    FILE *f = fopen(argv[2], "r");
    if (!f) return 2;
#define RECT(R, C) printf(" %d", 16 * R + C);
#define STRIP(R, C) printf(" %d", 128 + 16 * R + C);
    printf("const CF_MAX_DMA=%d CS_NAMAX=%d CS_SRMAX=%d CS_NSMAX=%d CS_DMAMAX=%d CD_WAVES=%d CD_NONE=%d\nbodies", CF_MAX_DMA, CS_NAMAX, CS_SRMAX,
           CS_NSMAX, CS_DMAMAX, CD_WAVES, (int)CD_NONE);
    CS_RECT_BODIES(RECT) CS_STRIP_BODIES(STRIP)
    printf("\ncw");
    for (int i = 0; i < 7; ++i) printf(" %d", 16 * CW_NQ[i] + 4 * CW_SQ[i]);
    printf("\n");
    char id[128];
    long long v[16];
    while (fscanf(f, "%127s", id) == 1) {
        for (int i = 0; i < 16; ++i)
            if (fscanf(f, "%lld", &v[i]) != 1) return 3;
        const int nb = (int)v[0], ntab = nb < 1 ? 1 : (nb > SK_MAXB ? SK_MAXB + 1 : nb);
        const double *W[SK_MAXB + 1], *X[SK_MAXB + 1];
        double *T[SK_MAXB + 1], *Out[SK_MAXB + 1];
        for (int b = 0; b < ntab; ++b) {           // never dereferenced: integers cast to pointers
            W[b] = (const double *)(0x30000000ull + 0x100000ull * b);
            X[b] = (const double *)(0x20000000ull + 0x100000ull * b + (b == ntab - 1 ? v[12] : 0));
            T[b] = (double *)(0x40000000ull + 0x100000ull * b);
            Out[b] = (double *)(0x50000000ull + 0x100000ull * b);
        }
        for (int wt = 0; wt < 2; ++wt)
            for (int force = 0; force < 2; ++force) {
                ChainStepArgs c{nb, (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], W, v[6], X, v[7], v[8], v[9], v[10],
                                (const double *)(0x10000000ull + v[11]), wt ? T : nullptr, Out};
                ChainSumArgs cs{c, wt ? (double *)0x70000000ull : nullptr, wt ? v[13] : 0, wt ? v[14] : 0, wt ? v[15] : 0};
                cs.s.T = nullptr;
                g_call = &c;
                {
                    ChainFusedPlan p;
                    const int rc = chain_fused_plan(c, n_cu, force, p);
                    printf("%s ncu=%d T=%d force=%d fused rc=%d", id, n_cu, wt, force, rc);
                    if (rc) {
                        const ChainStep &a = p.a;
                        printf(" nf=%d str=%d wt=%d ebuf=%d unr=%d waves=%d", p.nq, p.sq, (int)p.wt, p.ebuf, p.unr, p.waves);
                        printf(" a.nb=%d a.wpp=%d a.n=%d a.K1=%d a.A=%d a.A2=%d a.J=%d a.w_c=%lld a.x_j=%lld a.x_k=%lld a.x_c=%lld a.x_extent=%lld"
                               " a.t_extent=%lld", a.nb, a.wpp, a.n, a.K1, a.A, a.A2, a.J, (long long)a.w_c, (long long)a.x_j, (long long)a.x_k,
                               (long long)a.x_c, (long long)a.x_extent, (long long)a.t_extent);
                        printf(" a.AP=%d a.A2P=%d a.ebase=%d a.eunits=%d a.xcd_map=%d a.nload=%d a.diag=%d a.stamps=%d a.slab=%d a.piece=", a.AP, a.A2P,
                               a.ebase, a.eunits, a.xcd_map, a.nload, a.diag, a.stamps != nullptr, a.slab != nullptr);
                        for (int i = 0; i < CD_WAVES; ++i) printf("%s%u", i ? "," : "", a.piece[i]);
                        printf(" tables=%d", tables_ok(a, a.E, p.wt));
                        put_launch(p.l);
                    } else printf("\n");
                }
                {
                    ChainWidePlan p;
                    const int rc = chain_wide_plan(c, n_cu, force, p);
                    printf("%s ncu=%d T=%d force=%d wide rc=%d", id, n_cu, wt, force, rc);
                    if (rc) {
                        const ChainWide &a = p.a;
                        printf(" ci=%d nn=%d sn=%d wt=%d unr=%d mt2=%d", p.ci, p.nn, p.sn, (int)p.wt, p.unr, (int)p.mt2);
                        printf(" a.nb=%d a.wpp=%d a.nac=%d a.n=%d a.K1=%d a.A=%d a.A2=%d a.J=%d a.w_c=%lld a.x_j=%lld a.x_k=%lld a.x_c=%lld"
                               " a.x_extent=%lld a.t_extent=%lld", a.nb, a.wpp, a.nac, a.n, a.K1, a.A, a.A2, a.J, (long long)a.w_c, (long long)a.x_j,
                               (long long)a.x_k, (long long)a.x_c, (long long)a.x_extent, (long long)a.t_extent);
                        printf(" a.ac=%d a.A2P=%d a.ebase=%d a.eunits=%d a.ebuf2=%d a.xcd_map=%d a.loader=%d a.tpw=%d a.wimg=%d a.slab=%d", a.ac, a.A2P,
                               a.ebase, a.eunits, a.ebuf2, a.xcd_map, a.loader, a.tpw, a.wimg, a.slab != nullptr);
                        printf(" a.tile0=");
                        for (int i = 0; i < 8; ++i) printf("%s%d", i ? "," : "", a.tile0[i]);
                        printf(" a.tile1=");
                        for (int i = 0; i < 8; ++i) printf("%s%d", i ? "," : "", a.tile1[i]);
                        printf(" a.slot=");
                        for (int i = 0; i < 8; ++i) printf("%s%d", i ? "," : "", a.slot[i]);
                        printf(" tables=%d", tables_ok(a, a.E, p.wt));
                        put_launch(p.l);
                    } else printf("\n");
                }
                {
                    ChainSumPlan p;
                    const int rc = chain_sum_plan(cs, n_cu, force, p);
                    printf("%s ncu=%d T=%d force=%d sum rc=%d", id, n_cu, wt, force, rc);
                    if (rc) {
                        const ChainSumS &a = p.ka.s;
                        printf(" na_run=%d wt=%d", p.na_run, (int)p.wt);
                        printf(" a.nb=%d a.n=%d a.K1=%d a.A=%d a.A2=%d a.J=%d a.tpw=%d a.ngroups=%d a.nranges=%d a.w_c=%lld a.x_j=%lld a.x_k=%lld"
                               " a.x_c=%lld a.x_extent=%lld", a.nb, a.n, a.K1, a.A, a.A2, a.J, a.tpw, a.ngroups, a.nranges, (long long)a.w_c,
                               (long long)a.x_j, (long long)a.x_k, (long long)a.x_c, (long long)a.x_extent);
                        printf(" a.t_b=%lld a.t_ld=%lld a.t_extent=%lld a.RP=%d a.KB2=%d a.A2P=%d a.NNF=%d a.NS=%d a.ebase=%d a.gbase=%d a.eunits=%d"
                               " a.xcd_map=%d a.c_fast=%d", (long long)a.t_b, (long long)a.t_ld, (long long)a.t_extent, a.RP, a.KB2, a.A2P, a.NNF, a.NS,
                               a.ebase, a.gbase, a.eunits, a.xcd_map, a.c_fast);
                        printf(" a.kbase=%d a.krem=%d a.inv_ng=%d a.wpt=%d a.per=%d a.gu=%d a.w_c8=%u a.x_j8=%u a.x_c8=%u a.t_b8=%u a.t_a8=%u"
                               " a.slab_t8=%u a.slab_r8=%u a.e_inv=%u", a.kbase, a.krem, a.inv_ng, a.wpt, a.per, a.gu, a.w_c8, a.x_j8, a.x_c8, a.t_b8,
                               a.t_a8, a.slab_t8, a.slab_r8, a.e_inv);
                        printf(" a.slab=%d a.T=%d role=", a.slab != nullptr, a.T == cs.Tint);
                        for (int w = 0; w < 8; ++w) {
                            const ChainSumRole &r = p.ka.role[w];
                            printf("%s%d.%d.%d.%d.%d.%d.%d.%d", w ? "," : "", r.term, r.at0, r.na, r.body, r.rt0, r.ct0, r.pad0, r.pad1);
                        }
                        printf(" tables=%d", tables_ok(p.ka, a.E, false));
                        put_launch(p.l);
                    } else printf("\n");
                }
            }
    }
    fclose(f);
    return 0;
}
"""


def call(nb, n, K1, A, A2, J, right, **over):
    """A call as the chain tests make it: X[j][k][c] (right chain) or X[c][k][j] (left), W rows of A, T per term for the
    stacked-terms kernel; `over` replaces single numbers."""
    c = dict(nb=nb, n=n, K1=K1, A=A, A2=A2, J=J, w_c=A, x_extent=J * n * K1, e_off=0, x_off=0, t_b=A * n * J, t_ld=J,
             t_extent=nb * A * n * J)
    c.update(dict(x_j=n * K1, x_k=K1, x_c=1) if right else dict(x_j=1, x_k=J, x_c=n * J))
    c.update(over)
    return [c[k] for k in CALL_KEYS]


def edge_list():
    """(id, call): the smallest shapes on either side of each branch of the three plans"""
    e = []
    # ---- fused
    e += [("ef-J%d" % J, call(16, 40, 100, 100, 100, J, True)) for J in (1, 64, 65, 112, 113)]
    e += [("ef-K%d" % K1, call(2, 40, K1, 50, 50, 100, False)) for K1 in (1, 128, 129)]
    e += [("ef-A%d" % A, call(2, 40, 64, A, A, 40, False)) for A in (48, 52, 53, 54, 56, 57, 58)]     # remainders 0, 4, 5, 6, 8, 9, 10
    e += [("ef-A52-A48", call(2, 40, 64, 52, 48, 40, False)), ("ef-A100-A50", call(2, 40, 64, 100, 50, 40, True)),
          ("ef-A2odd", call(2, 40, 64, 52, 51, 40, False)), ("ef-Eoff8", call(2, 40, 64, 52, 52, 40, False, e_off=8)),
          ("ef-Xoff4", call(2, 40, 64, 52, 52, 40, False, x_off=4))]
    e += [("ef-K%d-A50" % K1, call(2, 40, K1, 50, 50, 20, False)) for K1 in (20, 24, 25)]             # 2 K1 < A, and the first that is not
    e += [("ef-nb%d" % nb, call(nb, 24, 64, 50, 50, 20, False)) for nb in (1, 32, 33)]
    e += [("ef-nb16-n%d" % n, call(16, n, 100, 100, 100, 100, True)) for n in (1, 2, 3, 31, 32)]      # wpp = 16 (256 CUs), 1 (20)
    e += [("ef-nb1-n%d" % n, call(1, n, 100, 100, 100, 100, True)) for n in (39, 40, 511, 512)]       # wpp = 256, 20
    lim = LIM32 // 8 - 100 - 132
    e += [("ef-xext-under", call(2, 40, 100, 100, 100, 100, True, x_extent=lim - 1)), ("ef-xext-over", call(2, 40, 100, 100, 100, 100, True, x_extent=lim))]
    # ---- wide
    e += [("ew-A2-%d" % A2, call(2, 50, 100, 160, A2, 100, True)) for A2 in (144, 148, 152, 153, 156, 160, 161)]
    e += [("ew-J%d-A2-%d" % (J, A2), call(1, 16, 160, 64, A2, J, True)) for J in (112, 113, 176, 177) for A2 in (112, 128)]
    e += [("ew-nb%d-J%d" % (nb, J), call(nb, 24, 20, 100, 100, J, True)) for nb in (1, 2, 8) for J in (20, 48, 49)]
    e += [("ew-A%d" % A, call(1, 100, 150, A, 110, 150, True)) for A in (56, 57, 112, 113, 168, 169)]  # one .. four chunks of at most 56 (two row tiles per wave)
    e += [("ew-lds-A2-%d" % A2, call(1, 100, 150, 64, A2, 100, True)) for A2 in (80, 82)]               # two E images, one
    # ---- sum
    e += [("es-J%d-K%d" % (J, K1), call(8, 24, K1, 100, 100, J, True)) for J, K1 in ((20, 20), (21, 20), (20, 21))]
    e += [("es-A%d" % A, call(8, 24, 20, A, 100, 20, True)) for A in (4, 128, 129)]
    e += [("es-A2-%d" % A2, call(8, 24, 20, 100, A2, 20, False)) for A2 in (48, 52, 53, 54, 56, 58)]
    e += [("es-nb%d" % nb, call(nb, 24, 20, 100, 100, 20, True)) for nb in (3, 4)]
    e += [("es-tpw4", call(8, 24, 20, 100, 100, 20, True)), ("es-tpw2", call(12, 40, 20, 112, 112, 20, True)),
          ("es-tpw1", call(8, 24, 20, 128, 104, 20, True))]
    tb, tld = LIM32 // 8, LIM32 // 8 // 24
    assert 24 * tld * 8 == LIM32
    e += [("es-tb-under", call(8, 24, 20, 100, 100, 20, True, t_b=tb - 1)), ("es-tb-over", call(8, 24, 20, 100, 100, 20, True, t_b=tb)),
          ("es-tld-under", call(8, 24, 20, 100, 100, 20, True, t_ld=tld - 1)), ("es-tld-over", call(8, 24, 20, 100, 100, 20, True, t_ld=tld))]
    return e


def parse(text):
    """driver / recorder output -> {(id, ncu, T, force, launcher): fields}, header lines apart"""
    out, head = {}, {}
    for line in text.splitlines():
        w = line.split()
        if w[0] in ("const", "bodies", "cw"):
            head[w[0]] = w[1:]
            continue
        f = dict(x.split("=", 1) for x in w[5:])
        out[(w[0], int(w[1][4:]), int(w[2][2:]), int(w[3][6:]), w[4])] = f
    return out, head


@pytest.fixture(scope="module")
def fixture_file():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def plans(tmp_path_factory, fixture_file):
    """every case of the fixture and of the edge list through the three plan functions, at both compute-unit counts"""
    exe = compile_driver(tmp_path_factory, "chain_plan", DRIVER)
    cases = exe.parent / "cases.txt"
    todo = {c[0]: c[1] for c in fixture_file["cases"]}
    for name, c in edge_list():
        assert todo.setdefault(name, c) == c, name
    cases.write_text("".join("%s %s\n" % (k, " ".join(str(x) for x in v)) for k, v in todo.items()))
    res, head = {}, None
    for n_cu in N_CU:
        r, head = parse(run_driver(exe, [n_cu, cases]))
        res.update(r)
    return res, head, todo


def route(v):
    """chain_step_try (csrc/tt_fused.hip): the fused kernel where every extent is <= 128, then the stacked-terms kernel,
    then the wide one -- from the three verdicts without `force`"""
    return "fused" if v["fused"] else ("sum" if v["sum"] else ("wide" if v["wide"] else "none"))


def bracket_name(kind, f, head):
    tf = lambda x: "true" if int(x) else "false"
    if kind == "fused":
        return "chain_step_kernel<%s, %s, %s, %s, 5, %s, 1, %s, %s>" % (f["nf"], f["str"], f["nf"], f["str"], tf(f["wt"]), f["ebuf"], f["unr"])
    if kind == "wide":
        ap = int(head["cw"][int(f["ci"])])
        return "chain_wide_kernel<%d, %d, %s, %s, %s, %s, %s>" % (ap // 16, ap % 16 // 4, f["nn"], f["sn"], tf(f["wt"]), f["unr"], tf(f["mt2"]))
    return "chain_sum_kernel<5, 5, NA, %s>" % tf(f["wt"])


def echoes(kind, c, T):
    """What an accepted plan only repeats from its call.  The fixture leaves these out (the recording checked them on the
    launchers it was taken from); here they are checked on every accepted plan."""
    e = {"a." + k: c[k] for k in ("nb", "n", "K1", "A", "A2", "J", "w_c", "x_j", "x_k", "x_c", "x_extent")}
    e.update({"wt": T, "tables": 1, "prof_work": 2.0 * c["nb"] * c["n"] * c["J"] * (c["K1"] * c["A"] + c["A"] * c["A2"])})
    if kind == "fused":
        e.update({"a.diag": 0, "a.stamps": 0})
    if kind == "sum":
        e.update({"a.T": 1, "a.t_b": c["t_b"] * T, "a.t_ld": c["t_ld"] * T, "a.t_extent": c["t_extent"] * T})
    return e


def name_without_wt(kind, name, T):
    """the bracket's name with its WT argument -- true exactly where T is written -- replaced by WT: a record then does not
    differ from the one before it by its name alone"""
    w = name.split(", ")
    i = {"fused": 5, "wide": 4, "sum": 3}[kind]
    assert w[i].rstrip(">") == ("true" if T else "false"), name
    w[i] = w[i].replace("true" if T else "false", "WT")
    return ", ".join(w)


def as_recorded(kind, f, c, T, head):
    """the fields of a plan in the recorder's terms, without those that repeat the call"""
    g = {k: v for k, v in f.items() if k not in ("slab", "red", "flops", "mt2", "na_run", "a.slab")}
    g["scratch"] = str(int(f["slab"]) * 8 + 64)
    g["reduce"] = f["red"]                          # chunks, M, N
    g["prof_work"] = f["flops"]
    g["prof_name"] = name_without_wt(kind, bracket_name(kind, f, head), T)
    if kind == "sum":
        g["na_inst"] = "2" if int(f["na_run"]) <= 2 else "4"
    for k, v in echoes(kind, c, T).items():
        assert float(g.pop(k)) == v, (kind, k)
    return g


def test_plans_equal_the_launchers_they_replace(plans, fixture_file):
    """A case of the fixture: [id, call, verdicts, routes, records].  verdicts: one digit per (compute units, T, launcher,
    force) in that order; routes: one letter per (compute units, T); records: one per accepted (compute units, T, launcher)
    in that order -- the first of a launcher in the file as the list of its fields, every later one as the pairs
    index, value of the fields that differ from the launcher's record before it."""
    res, head, _ = plans
    assert fixture_file["n_cu"] == list(N_CU) and len(fixture_file["cases"]) >= 200
    checked, prev = 0, {}
    for name, call_, verdicts, routes, records in fixture_file["cases"]:
        c, verdicts, records = dict(zip(CALL_KEYS, call_)), [int(x) for x in verdicts], list(records)
        for n_cu in N_CU:
            for T in (0, 1):
                first = {}
                for kind in ("fused", "wide", "sum"):
                    v0, v1 = verdicts.pop(0), verdicts.pop(0)
                    where = (name, n_cu, T, kind)
                    got0, got1 = dict(res[(name, n_cu, T, 0, kind)]), dict(res[(name, n_cu, T, 1, kind)])
                    assert (int(got0.pop("rc")), int(got1.pop("rc"))) == (v0, v1), where
                    first[kind] = v0
                    if v1:
                        r = records.pop(0)
                        if kind in prev:
                            r = [dict(zip(r[::2], r[1::2])).get(i, x) for i, x in enumerate(prev[kind])]
                        prev[kind] = r
                    want = dict(zip(fixture_file["fields"][kind], prev[kind])) if v1 else {}
                    for force, v, got in ((0, v0, got0), (1, v1, got1)):      # `force` changes the verdict, never the plan
                        if not v:
                            assert got == {}, where
                            continue
                        got = as_recorded(kind, got, c, T, head)
                        assert set(got) == set(want), (where, set(got) ^ set(want))
                        for k in want:
                            assert got[k] == str(want[k]), (where, force, k, got[k], want[k])
                        checked += 1
                assert route(first)[0] == routes[0], (name, n_cu, T)
                routes = routes[1:]
        assert not verdicts and not records and not routes, name
    print("accepted plans compared field by field:", checked)
    assert checked >= 1000


def test_fixture_holds_the_edge_list(fixture_file):
    have = {tuple(c[1]) for c in fixture_file["cases"]}
    for name, c in edge_list():
        assert tuple(c) in have, name


def tiles(r):
    """full 16-wide tiles, 4-wide strips of a rank (a remainder of 9..15 is a zero-padded full tile)"""
    nf, rem = divmod(r, 16)
    return (nf, 0) if rem == 0 else (nf, 1) if rem <= 4 else (nf, 2) if rem <= 8 else (nf + 1, 0)


def check_common(f, c, dma_max):
    assert int(f["lds"]) <= LDS_MAX
    assert int(f["a.eunits"]) % 64 == 0 and 1 <= int(f["a.eunits"]) // 64 <= dma_max
    assert int(f["a.ebase"]) % 2 == 0
    assert int(f["tables"]) == 1 and int(f["a.slab"]) == 0
    for k in ("nb", "n", "K1", "A", "A2", "J", "w_c", "x_j", "x_k", "x_c", "x_extent"):
        assert int(f["a." + k]) == c[k], k
    assert float(f["flops"]) == 2.0 * c["nb"] * c["n"] * c["J"] * (c["K1"] * c["A"] + c["A"] * c["A2"])


def check_fused(f, c, T, n_cu, head):
    const = dict(x.split("=") for x in head["const"])
    check_common(f, c, int(const["CF_MAX_DMA"]))
    assert int(f["wt"]) == T and (int(f["nf"]), int(f["str"])) == tiles(c["A"]) == tiles(c["A2"])
    assert (c["x_extent"] + c["x_k"] + 132 * c["x_c"]) * 8 < LIM32 and c["A"] * c["n"] * c["A2"] * 8 < LIM32
    assert int(f["a.t_extent"]) == c["A"] * c["n"] * c["J"]
    if T:
        assert (int(f["a.t_extent"]) + 16 * c["n"] * c["J"]) * 8 < LIM32
    wpp = int(f["a.wpp"])
    assert 1 <= wpp <= c["n"] and wpp == max(1, min(c["n"], n_cu // c["nb"]))
    assert int(f["grid"]) == c["nb"] * wpp and int(f["slab"]) == c["nb"] * wpp * c["J"] * c["A2"]
    assert f["red"] == "%d,%d,%d" % (wpp, c["J"], c["A2"])
    # a levelled workgroup only where it has two slices to earn its fixed cost back; its table: every wave a piece or a loader
    piece, waves, none = [int(x) for x in f["a.piece"].split(",")], int(f["waves"]), int(const["CD_NONE"])
    assert waves in (8, int(const["CD_WAVES"]))
    if waves == 8:
        assert piece == [0] * len(piece) and int(f["a.nload"]) == 0
    else:
        assert c["n"] >= 2 * wpp and c["J"] > 64
        loaders = sorted(p >> 8 & 255 for p in piece if p >> 16 == none)
        assert loaders == list(range(int(f["a.nload"]))) and loaders and piece[-1] >> 16 == none
        rows = {}
        for p in piece:
            if p >> 16 != none:
                rows.setdefault(p & 255, []).append(p >> 16)
        assert sorted(rows) == list(range((c["J"] + 15) // 16))
        assert all(sorted(k) in ([1], [2, 3], [4]) for k in rows.values()), rows      # whole | first + rest | four rows


def check_wide(f, c, T, n_cu, head):
    const = dict(x.split("=") for x in head["const"])
    check_common(f, c, int(const["CF_MAX_DMA"]))
    assert int(f["wt"]) == T and (int(f["nn"]), int(f["sn"])) == tiles(c["A2"])
    unr = int(f["unr"])
    kb1 = ((c["K1"] + 3) // 4 + unr - 1) // unr * unr
    assert unr in (5, 25)
    assert (c["x_extent"] + c["x_k"] + (kb1 * 4 + 32) * c["x_c"]) * 8 < LIM32
    assert int(f["a.t_extent"]) == c["A"] * c["n"] * c["J"]
    if T:
        assert (int(f["a.t_extent"]) + 80 * c["n"] * c["J"]) * 8 < LIM32
    ap, nac, ac, tpw, wpp = int(head["cw"][int(f["ci"])]), int(f["a.nac"]), int(f["a.ac"]), int(f["a.tpw"]), int(f["a.wpp"])
    assert ac % 4 == 0 and ac <= ap and nac * ac >= c["A"] and (nac - 1) * ac < c["A"]
    assert int(f["a.A2P"]) == c["A2"] + c["A2"] % 2 and int(f["a.wimg"]) >= 4 * kb1 * ap and int(f["a.ebase"]) == tpw * int(f["a.wimg"])
    assert int(f["lds"]) == (int(f["a.ebase"]) + int(f["a.eunits"]) * (4 if int(f["a.ebuf2"]) else 2)) * 8
    ng, units = (c["nb"] + tpw - 1) // tpw, wpp * nac
    assert 1 <= wpp <= c["n"] and wpp == max(1, min(c["n"], n_cu // (ng * nac)))
    assert int(f["grid"]) == ng * units and int(f["slab"]) == c["nb"] * units * c["J"] * c["A2"]
    assert f["red"] == "%d,%d,%d" % (units, c["J"], c["A2"])
    # the row tiles, once each per tensor slot, on the waves other than the loader
    t0, t1, slot = ([int(x) for x in f[k].split(",")] for k in ("a.tile0", "a.tile1", "a.slot"))
    loader, nt = int(f["a.loader"]), (c["J"] + 15) // 16
    assert t0[loader] == -1 and t1[loader] == -1 and 1 <= tpw <= min(7, c["nb"])
    seen = sorted((slot[w], t) for w in range(8) if w != loader for t in (t0[w], t1[w]) if t >= 0)
    assert seen == [(s, t) for s in range(tpw) for t in range(nt)]
    assert all(t1[w] < 0 or t0[w] >= 0 for w in range(8))
    if not int(f["mt2"]):
        assert t1 == [-1] * 8


def check_sum(f, c, T, n_cu, head):
    const = dict(x.split("=") for x in head["const"])
    check_common(f, c, 8 * int(const["CS_DMAMAX"]))
    assert int(f["wt"]) == T and int(f["a.T"]) == 1
    assert (int(f["a.NNF"]), int(f["a.NS"])) == tiles(c["A2"]) and int(f["a.NS"]) <= int(const["CS_NSMAX"])
    tpw, ng, nr = int(f["a.tpw"]), int(f["a.ngroups"]), int(f["a.nranges"])
    # 32-bit byte offsets, and the strides the kernel reads as 32-bit numbers
    assert (c["x_extent"] + c["x_k"]) * 8 < LIM32 and c["A"] * c["n"] * c["A2"] * 8 < LIM32
    assert ((c["K1"] - 1) * c["w_c"] + c["A"]) * 8 < LIM32 and c["nb"] * nr * c["J"] * c["A2"] * 8 < LIM32
    assert int(f["a.w_c8"]) == c["w_c"] * 8 < LIM32
    assert int(f["a.x_j8"]) == (c["x_j"] * 8 if c["J"] > 1 else 0) < LIM32 and int(f["a.x_c8"]) == (c["x_c"] * 8 if c["K1"] > 1 else 0) < LIM32
    if T:
        assert c["t_extent"] * 8 < LIM32
        assert int(f["a.t_b8"]) == (c["t_b"] * 8 if c["nb"] > 1 else 0) < LIM32
        assert int(f["a.t_a8"]) == (c["n"] * c["t_ld"] * 8 if c["A"] > 1 else 0) < LIM32
    assert int(f["a.slab_r8"]) == c["J"] * c["A2"] * 8 and int(f["a.slab_t8"]) == nr * c["J"] * c["A2"] * 8
    # grid, slab, slice ranges
    assert tpw in (1, 2, 4) and ng == (c["nb"] + tpw - 1) // tpw and 1 <= nr <= c["n"] and nr <= max(1, 3 * n_cu // 4 // ng)
    assert int(f["grid"]) == ng * nr and int(f["slab"]) == c["nb"] * nr * c["J"] * c["A2"] and f["red"] == "%d,%d,%d" % (nr, c["J"], c["A2"])
    assert int(f["a.kbase"]) * nr + int(f["a.krem"]) == c["n"] and 0 <= int(f["a.krem"]) < nr
    assert ng * nr * ng < 1 << 20 and all(i // ng == i * int(f["a.inv_ng"]) >> 20 for i in range(ng * nr))
    a2p = int(f["a.A2P"])
    assert a2p % 2 == 0 and a2p >= max(c["A2"], 16 * int(f["a.NNF"]) + 4 * int(f["a.NS"])) and int(f["a.e_inv"]) == -(-(1 << 32) // a2p)
    assert int(f["a.KB2"]) == (c["A"] + 3) // 4 and int(f["a.wpt"]) == 8 // tpw
    # phase B: the roles tile the NRT x NNF rectangle once, the strip column is one wave's, every body one the kernel has
    roles = [[int(x) for x in r.split(".")] for r in f["role"].split(",")]
    nrt, nnf, ns = (tpw * 20 + 15) // 16, int(f["a.NNF"]), int(f["a.NS"])
    assert int(f["a.RP"]) >= 16 * nrt
    bodies, cells, strips = {int(x) for x in head["bodies"]}, [], 0
    for term, at0, na, body, rt0, ct0, pad0, pad1 in roles:
        assert pad0 == pad1 == 0
        if body == 0:
            continue
        assert body in bodies, body
        if body >= 128:
            assert ((body - 128) // 16, body % 16) == (nrt, ns) and nrt <= int(const["CS_SRMAX"])
            strips += 1
        else:
            cells += [(r, q) for r in range(rt0, rt0 + body // 16) for q in range(ct0, ct0 + body % 16)]
    assert sorted(cells) == [(r, q) for r in range(nrt) for q in range(nnf)] and strips == (1 if ns else 0)
    # phase A: the a-tiles of every local term once
    nat = (c["A"] + 15) // 16
    for t in range(tpw):
        got = sorted(a for term, at0, na, *_ in roles if term == t for a in range(at0, at0 + na))
        assert got == list(range(nat)), (t, got)
    assert all(term < tpw and na <= int(f["na_run"]) <= int(const["CS_NAMAX"]) for term, at0, na, *_ in roles)


def test_invariants_at_the_dispatch_edges(plans):
    res, head, todo = plans
    accepted = {"fused": 0, "wide": 0, "sum": 0}
    for name, c in edge_list():
        c = dict(zip(CALL_KEYS, c))
        for n_cu in N_CU:
            for T in (0, 1):
                for force in (0, 1):
                    for kind, check in (("fused", check_fused), ("wide", check_wide), ("sum", check_sum)):
                        f = dict(res[(name, n_cu, T, force, kind)])
                        if int(f.pop("rc")):
                            try:
                                check(f, c, T, n_cu, head)
                            except AssertionError as e:
                                raise AssertionError((name, n_cu, T, force, kind, f)) from e
                            accepted[kind] += 1
    print("accepted plans of the edge list:", accepted)
    assert min(accepted.values()) >= 100


def verdict(res, name, kind, force=1, T=0, n_cu=256):
    return int(res[(name, n_cu, T, force, kind)]["rc"])


def test_the_edges_fall_on_the_sides_they_are_named_for(plans):
    """each pair of the edge list straddles its branch: one side covered, the other not (or another structure)"""
    res, _, _ = plans
    v = lambda *a, **k: verdict(res, *a, **k)
    assert [v("ef-J%d" % J, "fused") for J in (1, 64, 65, 112, 113)] == [1, 1, 1, 1, 0]
    assert (res[("ef-J64", 256, 0, 1, "fused")]["waves"], res[("ef-J65", 256, 0, 1, "fused")]["waves"]) == ("8", "12")
    assert [v("ef-K%d" % K, "fused") for K in (1, 128, 129)] == [1, 1, 0] and v("ef-K1", "fused", force=0) == 0
    assert [v("ef-A%d" % A, "fused") for A in (48, 52, 53, 54, 56, 57, 58)] == [1, 1, 0, 1, 1, 0, 1]
    assert [v(n, "fused") for n in ("ef-A52-A48", "ef-A100-A50", "ef-A2odd", "ef-Eoff8", "ef-Xoff4")] == [0] * 5
    assert [(v("ef-K%d-A50" % K, "fused", force=0), v("ef-K%d-A50" % K, "fused")) for K in (20, 24, 25)] == [(0, 1), (0, 1), (1, 1)]
    assert [v("ef-nb%d" % nb, "fused") for nb in (1, 32, 33)] == [1, 1, 0]
    assert [res[("ef-nb16-n%d" % n, 256, 0, 1, "fused")]["waves"] for n in (1, 31, 32)] == ["8", "8", "12"]
    assert [res[("ef-nb16-n%d" % n, 20, 0, 1, "fused")]["waves"] for n in (1, 2, 3)] == ["8", "12", "12"]
    assert [res[("ef-nb1-n%d" % n, 256, 0, 1, "fused")]["waves"] for n in (511, 512)] == ["8", "12"]
    assert [res[("ef-nb1-n%d" % n, 20, 0, 1, "fused")]["waves"] for n in (39, 40)] == ["8", "12"]
    assert (v("ef-xext-under", "fused"), v("ef-xext-over", "fused")) == (1, 0)
    assert [v("ew-A2-%d" % A2, "wide") for A2 in (144, 148, 152, 153, 156, 160, 161)] == [1, 1, 1, 1, 1, 1, 0]
    assert [[v("ew-J%d-A2-%d" % (J, A2), "wide") for A2 in (112, 128)] for J in (112, 113, 176, 177)] == [[1, 1], [1, 0], [1, 0], [0, 0]]
    assert [res[("ew-nb%d-J20" % nb, 256, 0, 1, "wide")]["a.tpw"] for nb in (1, 2, 8)] == ["1", "2", "7"]
    assert [res[("ew-nb8-J%d" % J, 256, 0, 1, "wide")]["a.tpw"] for J in (20, 48, 49)] == ["7", "3", "1"]
    assert [res[("ew-A%d" % A, 256, 0, 1, "wide")]["a.nac"] for A in (56, 57, 112, 113, 168, 169)] == ["1", "2", "2", "3", "3", "4"]
    assert [res[("ew-lds-A2-%d" % A2, 256, 0, 1, "wide")]["a.ebuf2"] for A2 in (80, 82)] == ["1", "0"]
    assert [v("es-J%d-K%d" % jk, "sum") for jk in ((20, 20), (21, 20), (20, 21))] == [1, 0, 0]
    assert [v("es-A%d" % A, "sum") for A in (4, 128, 129)] == [1, 1, 0]
    assert [v("es-A2-%d" % A2, "sum") for A2 in (48, 52, 53, 54, 56, 58)] == [1, 1, 0, 1, 1, 1]
    assert [(v("es-nb%d" % nb, "sum", force=0), v("es-nb%d" % nb, "sum")) for nb in (3, 4)] == [(0, 1), (1, 1)]
    assert [res[("es-tpw%d" % t, 256, 0, 1, "sum")]["a.tpw"] for t in (4, 2, 1)] == ["4", "2", "1"]
    assert [v(n, "sum", T=1) for n in ("es-tb-under", "es-tb-over", "es-tld-under", "es-tld-over")] == [1, 0, 1, 0]
    assert [v(n, "sum", T=0) for n in ("es-tb-under", "es-tb-over", "es-tld-under", "es-tld-over")] == [1, 1, 1, 1]
