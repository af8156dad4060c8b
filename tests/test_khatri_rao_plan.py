"""The host-side plans of the Khatri-Rao kernels (plain C++, compiled by the host compiler alone): csrc/khatri_rao_plan.h
(ttsk_kr_rows, ttsk_kr_step: checks and grids) and csrc/sparse_plan.h with kind-5 factors of ttsk_sg_factor -- a kind-4
chain whose steps are diagonal.  Whatever sg_plan decides for a kind-5 factor it must decide for the kind-4 factor of the same
ranks, apart from the flag SgPlanCh::diag."""
import pytest

from tests.host_driver import compile_driver, run_driver

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "sparse_plan.h"
#include "khatri_rao_plan.h"
using namespace ttsk;
static double dummy;
// a factor from argv: kind w lo | for kinds 4 and 5: rows steps null_core (n)*steps (rank)*(steps + 1)
static char **factor(char **v, ttsk_sg_factor &f, ttsk_sg_chain &c)
{
    f.kind = atoi(v[0]); f.w = atoi(v[1]); f.rank_min = atoi(v[2]);
    v += 3;
    if (f.kind != 4 && f.kind != 5) return v;
    c.rows = strtoull(v[0], nullptr, 10); c.steps = atoi(v[1]);
    const int null_core = atoi(v[2]);
    v += 3;
    for (int s = 0; s < c.steps; ++s, ++v)
        if (s < TTSK_SG_CHAIN_MAX) { c.core[s] = s == null_core ? nullptr : &dummy; c.n[s] = atoll(v[0]); }
    for (int s = 0; s <= c.steps; ++s, ++v)
        if (s <= TTSK_SG_CHAIN_MAX) c.rank[s] = atoi(v[0]);
    f.chain = &c;
    if (c.rows) f.table = &dummy;
    return v;
}
static void *ptr(const char *s) { return atoi(s) ? (void *)&dummy : nullptr; }
int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "rows")) {          // rows prev P g n w out
        KrPlan p;
        const int rc = kr_rows_plan((double *)ptr(argv[2]), atoll(argv[3]), (double *)ptr(argv[4]), atoll(argv[5]), atoll(argv[6]),
                                    (double *)ptr(argv[7]), &p);
        printf("rc %d\nmsg %s\nkr %lld %lld %lld\nconst %d %lld\n", rc, p.msg, (long long)p.rows, (long long)p.total, (long long)p.blocks,
               KR_THREADS, (long long)KR_BLOCKS_MAX);
        return 0;
    }
    if (argc >= 2 && !strcmp(argv[1], "step")) {          // step v g n w idx N out
        KrPlan p;
        const int rc = kr_step_plan((double *)ptr(argv[2]), (double *)ptr(argv[3]), atoll(argv[4]), atoll(argv[5]), (int64_t *)ptr(argv[6]),
                                    (size_t)strtoull(argv[7], nullptr, 10), (double *)ptr(argv[8]), &p);
        printf("rc %d\nmsg %s\nkr %lld %lld %lld\nconst %d %lld\n", rc, p.msg, (long long)p.rows, (long long)p.total, (long long)p.blocks,
               KR_THREADS, (long long)KR_BLOCKS_MAX);
        return 0;
    }
    ttsk_sg_factor f[3] = {};
    ttsk_sg_chain c[3] = {};
    const ttsk_sg_factor *fp[3];
    char **v = argv + 1;
    for (int i = 0; i < 3; ++i) { v = factor(v, f[i], c[i]); fp[i] = f[i].kind < 0 ? nullptr : &f[i]; }
    const int c_left = atoi(v[0]), w32 = atoi(v[3]);
    SgPlan p;
    const int rc = sg_plan(fp[0], fp[1], fp[2], c_left, (size_t)atoll(v[1]), (size_t)atoll(v[2]), &p, w32);
    printf("rc %d\nmsg %s\n", rc, p.msg);
    if (rc) return 0;
    for (int i = 0; i < 3; ++i) {
        const SgPlanCh &h = p.ch[i];
        printf("f%d %d %d %d %d %d\n", i, p.f[i].kind, p.f[i].w, p.f[i].off, p.f[i].units, p.f[i].rcp);
        printf("ch%d %d %d %d %d %d %d %u", i, h.steps, h.has_table, h.lo, h.toff, h.doff, h.gsh, h.rows);
        for (int s = 0; s < h.steps; ++s) printf(" %u %u %d", h.n[s], h.dn[s].mul, h.dn[s].sh);
        for (int s = 0; s <= h.steps; ++s) printf(" %d", h.rank[s]);
        printf("\ndiag%d %d\n", i, h.diag);
    }
    printf("tile %d %d %d\ninst %d %d %d\nchain %d %d %d\n", p.tcols, p.tab, p.qcols, p.NT, p.NS, p.T, p.has_chain, p.digits, p.chain);
    printf("grid %zu %zu %zu %zu %zu\n", p.lds, p.wg_per_cu, p.chunk, p.waves, p.blocks);
    printf("out %d %d %zu %zu %zu %zu\n", p.cellsP, p.cellsO, p.psi_off, p.om_off, p.j_off, p.scratch);
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "khatri_rao_plan", DRIVER)
    return lambda args: run_driver(exe, args).splitlines()


def _parse(out):
    p = dict(rc=int(out[0].split()[1]), msg=out[1][4:])
    for line in out[2:]:
        key, *v = line.split()
        p[key] = [int(x) for x in v]
    return p


# ------------------------------------------------------------------ khatri_rao_plan.h
def rows_plan(driver, prev=1, P=1, g=1, n=1, w=1, out=1):
    return _parse(driver(["rows", prev, P, g, n, w, out]))


def step_plan(driver, v=1, g=1, n=1, w=1, idx=1, N=1, out=1):
    return _parse(driver(["step", v, g, n, w, idx, N, out]))


def _blocks(total):
    return min(-(-total // 256), 8192)


def test_kr_rows_grids(driver):
    for P, n, w in [(1, 1, 1), (1, 37, 17), (200, 150, 15), (30000, 100, 32), (2 ** 20, 2 ** 10, 32)]:
        for prev in ((0, 1) if P == 1 else (1,)):
            p = rows_plan(driver, prev=prev, P=P, n=n, w=w)
            assert p["rc"] == 0 and p["kr"] == [n * P, n * P * w, _blocks(n * P * w)], p
            assert p["const"] == [256, 8192]
    assert rows_plan(driver, P=1, n=16, w=16)["kr"][2] == 1 and rows_plan(driver, P=1, n=257, w=1)["kr"][2] == 2


def test_kr_rows_refusals(driver):
    refused = {
        "ttsk_kr_rows: NULL g or out": [dict(g=0), dict(out=0)],
        "ttsk_kr_rows: n = 0, w = 3, P = 2 must be positive": [dict(n=0, w=3, P=2)],
        "ttsk_kr_rows: n = 4, w = 0, P = 2 must be positive": [dict(n=4, w=0, P=2)],
        "ttsk_kr_rows: n = 4, w = 3, P = -1 must be positive": [dict(n=4, w=3, P=-1)],
        "ttsk_kr_rows: NULL prev means P = 1, not 2": [dict(prev=0, P=2)],
    }
    for msg, cases in refused.items():
        for kw in cases:
            p = rows_plan(driver, **kw)
            assert p["rc"] == -2 and p["msg"] == msg and p["kr"] == [0, 0, 0], (kw, p)
    p = rows_plan(driver, P=2 ** 40, n=2 ** 40, w=1)
    assert p["rc"] == -3 and p["msg"] == "ttsk_kr_rows: n * P does not fit in int64_t"
    p = rows_plan(driver, P=2 ** 31, n=2 ** 31, w=2)
    assert p["rc"] == -3 and "one grid stride do not fit in int64_t" in p["msg"]


def test_kr_step_grids(driver):
    for N in (1, 31, 32, 33, 2049, 10 ** 7):
        for w in (1, 15, 16, 17, 32):
            for idx in (0, 1):
                p = step_plan(driver, n=N if not idx else 37, w=w, idx=idx, N=N)
                assert p["rc"] == 0 and p["kr"] == [N, N * w, _blocks(N * w)], p
    for v in (0, 1):                                       # nothing to do: no launch, whatever the pointers are
        assert step_plan(driver, v=v, g=0, idx=0, N=0, out=0)["kr"] == [0, 0, 0]


def test_kr_step_refusals(driver):
    refused = {
        "ttsk_kr_step: NULL g or out": [dict(g=0), dict(out=0)],
        "ttsk_kr_step: n = 0, w = 3 must be positive": [dict(n=0, w=3)],
        "ttsk_kr_step: n = 4, w = -2 must be positive": [dict(n=4, w=-2)],
        "ttsk_kr_step: without an index 5 rows are read from a g of 4": [dict(idx=0, n=4, N=5)],
    }
    for msg, cases in refused.items():
        for kw in cases:
            p = step_plan(driver, **kw)
            assert p["rc"] == -2 and p["msg"] == msg and p["kr"] == [0, 0, 0], (kw, p)
    assert step_plan(driver, idx=0, n=4, N=4)["rc"] == 0
    assert step_plan(driver, n=1, w=32, N=2 ** 62)["rc"] == -3


# ------------------------------------------------------------------ kind 5 in sg_plan
ABSENT = [-1, 0, 0]
TABLE = lambda w: [1, w, 0]


def chain_args(kind, w, lo, rows, ns, ranks, null_core=-1):
    assert len(ranks) == len(ns) + 1
    return [kind, w, lo, rows, len(ns), null_core] + list(ns) + list(ranks)


def plan(driver, A, B, C, c_left=0, N=1281, n_cu=256, w32=1):
    return _parse(driver(A + B + C + [c_left, N, n_cu, w32]))


def _same_but_for_the_flag(p5, p4, where):
    assert p5["rc"] == 0 and p4["rc"] == 0, (where, p5, p4)
    keys5 = {k: v for k, v in p5.items() if not k.startswith("diag")}
    keys4 = {k: v for k, v in p4.items() if not k.startswith("diag")}
    assert keys5 == keys4, (where, keys5, keys4)


@pytest.mark.parametrize("position", ["A", "B", "C"])
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("steps", [0, 1, 8])
def test_kind_5_plans_as_kind_4_of_the_same_ranks(driver, position, table, steps):
    """widths 1, 16, 17 and 32, 0 / 1 / 8 steps, with and without a start table, in each position beside two table factors, and
    a rank slice.  Without a table a kind-4 chain starts from the vector (1), so its rank 0 is 1 where kind 5 has w ones: the
    plan of kind 4 is then taken at ranks (1, w, ..., w), which differ in that entry alone."""
    i = "ABC".index(position)
    for w, lo, rho in ((1, 0, 1), (16, 0, 16), (17, 0, 17), (32, 0, 32), (5, 3, 9)):
        ns = [7] * steps
        rows = 35 if table else 0
        ranks = [rho] * (steps + 1)

        def beside(ch):
            return {"A": (ch, TABLE(w), TABLE(5)), "B": (TABLE(w), ch, TABLE(5)), "C": (TABLE(5), TABLE(w), ch)}[position]
        p5 = plan(driver, *beside(chain_args(5, w, lo, rows, ns, ranks)))
        if not table and steps == 0:
            assert p5["rc"] == -2 and p5["msg"].endswith("chain with neither a table nor a core"), p5
            continue
        p4 = plan(driver, *beside(chain_args(4, w, lo, rows, ns, ranks if table else [1] + ranks[1:])))
        if p5["rc"]:                                       # (three wide factors and 8 rows of digits: the LDS may not hold them)
            assert p5["rc"] == p4["rc"] == -3 and p5["msg"] == p4["msg"] and "does not fit the LDS" in p5["msg"], (p5, p4)
            continue
        if not table:
            assert p5["ch%d" % i][-(steps + 1):] == ranks and p4["ch%d" % i][-(steps + 1):] == [1] + ranks[1:]
            p5["ch%d" % i][-(steps + 1)] = p4["ch%d" % i][-(steps + 1)] = 0
        _same_but_for_the_flag(p5, p4, (position, table, steps, w))
        assert [p5["diag%d" % k] for k in range(3)] == [[int(k == i)] for k in range(3)]
        assert [p4["diag%d" % k] for k in range(3)] == [[0]] * 3
        assert p5["f%d" % i][0] == 4 and p5["inst"][0] == (2 if max(rho, w) > 16 else 1)
        assert p5["ch%d" % i][:3] == [steps, int(table), lo]


def test_kind_5_in_all_three_positions_and_streams_lengths(driver):
    ch = lambda kind, w: chain_args(kind, w, 0, 35, [7, 3], [w] * 3)
    for w in (1, 16, 17, 32):
        for N in (1, 31, 32, 33, 2049, 10 ** 7):
            for c_left in (0, 1):
                _same_but_for_the_flag(plan(driver, ch(5, w), ch(5, w), ch(5, w), c_left=c_left, N=N),
                                       plan(driver, ch(4, w), ch(4, w), ch(4, w), c_left=c_left, N=N), (w, N, c_left))


def test_kind_5_refusals_each_with_its_own_message(driver):
    ok = TABLE(4)
    head = "ttsk_sparse_gauss_pass: factor 0: "
    refused = {
        "a diagonal chain of ranks 4 and 5, it has one rank throughout": (chain_args(5, 2, 0, 0, [5], [4, 5]), -2, 1),
        "a diagonal chain of ranks 4 and 3, it has one rank throughout": (chain_args(5, 2, 0, 9, [5, 6], [4, 4, 3]), -2, 1),
        "chain rank 0 is 33, up to 32 are covered": (chain_args(5, 2, 0, 0, [5], [33, 33]), -3, 1),
        "chain of 9 steps, up to 8 are covered": (chain_args(5, 2, 0, 0, [5] * 9, [4] * 10), -3, 1),
        "a chain factor takes the 32-bit streams only": (chain_args(5, 2, 0, 0, [5], [4, 4]), -3, 0),
        "chain core 0 is NULL": (chain_args(5, 2, 0, 0, [5], [4, 4], null_core=0), -2, 1),
        "chain core 1 is NULL": (chain_args(5, 2, 0, 9, [5, 6], [4, 4, 4], null_core=1), -2, 1),
        "chain with neither a table nor a core": (chain_args(5, 2, 0, 0, [], [4]), -2, 1),
        "columns [3, 5) of a chain that ends in rank 4": (chain_args(5, 2, 3, 0, [5], [4, 4]), -2, 1),
        "chain rank 0 is 0": (chain_args(5, 1, 0, 0, [5], [0, 0]), -2, 1),
        "kind 5, width 33": (chain_args(5, 33, 0, 0, [5], [33, 33]), -2, 1),
        "kind 6, width 2": ([6, 2, 0], -2, 1),
    }
    for msg, (A, rc, w32) in refused.items():
        p = plan(driver, A, ok, ABSENT, w32=w32)
        assert p["rc"] == rc and p["msg"] == head + msg, (msg, p)
    assert plan(driver, chain_args(5, 2, 2, 0, [5], [4, 4]), ok, ABSENT)["rc"] == 0
