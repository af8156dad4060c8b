"""The host-side plan of a sparse pass with chain factors (kind 4 of ttsk_sg_factor; csrc/sparse_plan.h, plain C++): a driver
compiled with the host compiler prints the plan and the digits sg_chain_digits extracts, and both are checked here -- the LDS
layout before any kernel reads it, the multiply-shift division against Python's divmod.  Plans without a chain factor are
tests/test_sparse_plan.py's."""

import pytest

from tests import sparse_chain_ref as ref
from tests.host_driver import compile_driver, run_driver

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "sparse_plan.h"
using namespace ttsk;
static double dummy;
// a factor from argv: kind w lo | for kind 4: rows steps rank0 (n rank)*steps
static char **factor(char **v, ttsk_sg_factor &f, ttsk_sg_chain &c)
{
    f.kind = atoi(v[0]); f.w = atoi(v[1]); f.rank_min = atoi(v[2]);
    v += 3;
    if (f.kind != 4) return v;
    c.rows = strtoull(v[0], nullptr, 10); c.steps = atoi(v[1]); c.rank[0] = atoi(v[2]);
    v += 3;
    for (int s = 0; s < c.steps; ++s, v += 2)
        if (s < TTSK_SG_CHAIN_MAX) { c.core[s] = &dummy; c.n[s] = atoll(v[0]); c.rank[s + 1] = atoi(v[1]); }
    f.chain = &c;
    if (c.rows) f.table = &dummy;
    return v;
}
int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "digits")) {   // digits j_last rows steps n... : then flat indices (and j) on stdin
        ttsk_sg_factor f = {};
        ttsk_sg_chain c = {};
        f.kind = 4; f.w = 1; f.chain = &c;
        const int j_last = atoi(argv[2]);
        c.rows = strtoull(argv[3], nullptr, 10); c.steps = atoi(argv[4]); c.rank[0] = 1;
        for (int s = 0; s < c.steps; ++s) { c.core[s] = &dummy; c.n[s] = atoll(argv[5 + s]); c.rank[s + 1] = 1; }
        SgPlan p;
        if (sg_plan(&f, nullptr, nullptr, 0, 1, 256, &p, 1)) { printf("refused %s\n", p.msg); return 1; }
        unsigned long long flat, j;
        while (scanf("%llu %llu", &flat, &j) == 2) {
            uint32_t dg[TTSK_SG_CHAIN_MAX] = {};
            const uint32_t row = sg_chain_digits(p.ch[0], (uint32_t)flat, j_last != 0, (uint32_t)j, dg, 1);
            printf("%u", row);
            for (int s = 0; s < c.steps; ++s) printf(" %u", dg[s]);
            printf("\n");
        }
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
    for (int i = 0; i < 3; ++i)
        printf("f%d %d %d %d %d %d %d %d %d %d %d\n", i, p.f[i].kind, p.f[i].w, p.f[i].off, p.f[i].units, p.f[i].rcp, p.ch[i].steps,
               p.ch[i].has_table, p.ch[i].toff, p.ch[i].doff, 1 << p.ch[i].gsh);
    printf("tile %d %d %d\ninst %d %d %d\nchain %d %d %d\n", p.tcols, p.tab, p.qcols, p.NT, p.NS, p.T, p.has_chain, p.digits, p.chain);
    printf("grid %zu %zu %zu %zu %zu\n", p.lds, p.wg_per_cu, p.chunk, p.waves, p.blocks);
    const SgLds L = sg_lds_layout(p.tcols, p.tab, p.qcols, p.T, p.chain);
    printf("lds %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", L.tile, L.tabs, L.ro, L.rv, L.rj, L.q, L.cv, L.cd, L.total);
    printf("const %zu %zu %zu %d %d %d\n", SG_LDS_BUDGET, sg_salt_bytes(p.NT), SG_STATIC_SLACK, SG_CHAIN_GROUPS, SG_CHAIN_RANK, SG_CHAIN_MAX);
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "sparse_chain_plan", DRIVER)
    return lambda args, stdin="": run_driver(exe, args, stdin=stdin).splitlines()


def chain_args(w, lo, rows, rank0, steps):
    return [4, w, lo, rows, len(steps), rank0] + [x for n, r in steps for x in (n, r)]


ABSENT = [-1, 0, 0]
TABLE = lambda w: [1, w, 0]


def plan(driver, A, B, C, c_left=0, N=1281, n_cu=256, w32=1):
    out = driver(A + B + C + [c_left, N, n_cu, w32])
    p = dict(rc=int(out[0].split()[1]), msg=out[1][4:])
    for line in out[2:]:
        key, *v = line.split()
        p[key] = [int(x) for x in v]
    return p


def check_layout(p):
    (tcols, tab, qcols), (NT, NS, T), (has_chain, digits, chain) = p["tile"], p["inst"], p["chain"]
    tile, tabs, ro, rv, rj, q, cv, cd, total = p["lds"]
    budget, salt, slack, groups, rank, _ = p["const"]
    assert has_chain == 1
    # the regions in order, each as long as its contents: the layout of a pass without chain factors, then the running
    # vectors (two per group of lanes, of the widest rank), then one row of T ints per digit
    regions = [(tile, T * tcols), (tabs, tab), (ro, 3 * T), (rv, T), (rj, T // 2), (q, (T * qcols + 3) // 4), (cv, groups * 2 * rank),
               (cd, (digits * T + 1) // 2)]
    for (b0, n0), (b1, _) in zip(regions, regions[1:]):
        assert b0 + n0 == b1, regions
    assert cd + (digits * T + 1) // 2 == total and chain == total - cv
    assert (total - cd) * 8 >= digits * T * 4
    lds, wg = p["grid"][:2]
    assert lds == total * 4 * 8
    assert 1 <= wg <= (3 if NT == 1 else 2) and wg * (lds + salt + slack) <= budget
    doffs = []
    for kind, w, off, units, rcp, steps, has_table, toff, doff, G in (p["f0"], p["f1"], p["f2"]):
        if kind == 4:
            assert off + w <= tcols and G in (16, 32) and 64 // G <= groups
            doffs.append((doff, steps))
            if has_table:                       # the block of its start rows: T rows of 2 units doubles inside the table region
                assert toff % T == 0 and toff + 2 * units * T <= tab
        elif kind == 1:
            assert off % T == 0 and off + 2 * units * T <= tab
    # the digit rows of the chain factors: disjoint, together all of them
    doffs.sort()
    assert doffs[0][0] == 0 and all(a + s == b for (a, s), (b, _) in zip(doffs, doffs[1:])) and doffs[-1][0] + doffs[-1][1] == digits


@pytest.mark.parametrize("position", ["A", "B", "C"])
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("steps", [0, 1, 3])
def test_lds_layout_of_a_chain_factor(driver, position, table, steps):
    """ranks 1 .. 32 on every inner and outer bond, no core (table only) / the first core only / three cores, in each
    position beside two table factors: regions disjoint and inside the budget, or a refusal with its own message"""
    for rank in (1, 2, 15, 16, 17, 32):
        if not table and steps == 0:
            core_steps, rank0 = [(7, rank)], 1                     # "steps 0" without a table: the first core only
        else:
            core_steps, rank0 = [(7, rank)] * steps, rank if table else 1
        ch = chain_args(rank, 0, 35 if table else 0, rank0, core_steps)
        A, B, C = {"A": (ch, TABLE(rank), TABLE(5)), "B": (TABLE(rank), ch, TABLE(5)), "C": (TABLE(5), TABLE(rank), ch)}[position]
        p = plan(driver, A, B, C, c_left=0)
        if p["rc"]:
            assert p["rc"] == -3 and "does not fit the LDS" in p["msg"], p
            continue
        G = p["f%d" % "ABC".index(position)][-1]
        assert G == (16 if rank <= 16 else 32)
        assert p["inst"][0] == (2 if rank > 16 else 1)
        check_layout(p)


def test_three_wide_chains_take_the_16_record_tile(driver):
    ch = chain_args(32, 0, 35, 32, [(7, 32)])
    p = plan(driver, ch, ch, ch, c_left=1)
    assert p["rc"] == 0 and p["inst"] == [2, 0, 16], p
    check_layout(p)
    p = plan(driver, chain_args(32, 0, 35, 32, [(7, 32)]), TABLE(32), TABLE(32))
    assert p["rc"] == 0 and p["inst"] == [2, 0, 16], p
    check_layout(p)


def test_plan_without_a_chain_has_no_chain_region(driver):
    p = plan(driver, TABLE(16), TABLE(16), TABLE(16), c_left=1)
    assert p["rc"] == 0 and p["chain"] == [0, 0, 0]
    tile, tabs, ro, rv, rj, q, cv, cd, total = p["lds"]
    assert cv == cd == total == 32 * 1 + 32 * 3 * 16 + 4 * 32 + 16


def test_refusals_each_with_its_own_message(driver):
    ok = TABLE(4)
    head = "ttsk_sparse_gauss_pass: factor 0: "
    refused = {
        "chain rank 1 is 33, up to 32 are covered": (chain_args(2, 0, 0, 1, [(5, 33)]), -3, 1),
        "chain rank 0 is 33, up to 32 are covered": (chain_args(2, 0, 9, 33, [(5, 4)]), -3, 1),
        "chain with neither a table nor a core": (chain_args(1, 0, 0, 1, []), -2, 1),
        "a chain factor takes the 32-bit streams only": (chain_args(2, 0, 0, 1, [(5, 4)]), -3, 0),
        "chain of 9 steps, up to 8 are covered": (chain_args(2, 0, 0, 1, [(5, 4)] * 9), -3, 1),
        "chain from the first core with rank 2 in front of it": (chain_args(2, 0, 0, 2, [(5, 4)]), -2, 1),
        "columns [3, 5) of a chain that ends in rank 4": (chain_args(2, 3, 0, 1, [(5, 4)]), -2, 1),
        "chain mode 0 has size 0": (chain_args(2, 0, 0, 1, [(0, 4)]), -2, 1),
        "chain mode 0 of size 2147483648, below 2^31 is covered": (chain_args(2, 0, 0, 1, [(2 ** 31, 4)]), -3, 1),
        "chain table of 2147483648 rows, below 2^31 is covered": (chain_args(2, 0, 2 ** 31, 2, [(5, 4)]), -3, 1),
        "kind 4, width 33": (chain_args(33, 0, 0, 1, [(5, 33)]), -2, 1),
    }
    for msg, (A, rc, w32) in refused.items():
        p = plan(driver, A, ok, ABSENT, w32=w32)
        assert p["rc"] == rc and p["msg"] == head + msg, (msg, p)
    assert plan(driver, chain_args(2, 2, 0, 1, [(5, 4)]), ok, ABSENT)["rc"] == 0


def _digits(driver, rows, ns, flats, js=None):
    lines = "".join(f"{f} {0 if js is None else j}\n" for f, j in zip(flats, js if js is not None else flats))
    out = driver(["digits", int(js is not None), rows, len(ns)] + list(ns), stdin=lines)
    return [[int(x) for x in line.split()] for line in out]


def _want(rows, ns, flats, js=None):
    row, idx = ref.digits(flats, rows, ns, js)
    return [[int(row[e])] + [int(i[e]) for i in idx] for e in range(len(flats))]


@pytest.mark.parametrize("rows", [0, 1, 3, 7])
def test_digits_exhaustively_for_small_extents(driver, rows):
    import itertools
    for m in (1, 2, 3):
        for ns in itertools.product((1, 2, 3, 7), repeat=m):
            extent = max(rows, 1)
            for n in ns:
                extent *= n
            flats = list(range(extent))
            assert _digits(driver, rows, ns, flats) == _want(rows, ns, flats), (rows, ns)
    # the mode index as the last digit: it takes no part in the flat index
    ns, flats = (3, 7, 2), list(range(max(rows, 1) * 21))
    js = [f % 2 for f in flats]
    assert _digits(driver, rows, ns, flats, js) == _want(rows, ns, flats, js)


@pytest.mark.parametrize("rows, ns", [(0, (32768, 32767, 2)), (0, (46340, 46340)), (32768, (32767, 2)), (46340, (46340,)),
                                      (0, (2 ** 31 - 1,)), (2 ** 31 - 1, ()), (1, (2 ** 31 - 1, 1)), (0, (1, 65536, 32767)),
                                      (0, (3, 715827882)), (715827882, (3,))])
def test_digits_of_flat_indices_up_to_2_31(driver, rows, ns):
    import numpy as np
    extent = max(rows, 1)
    for n in ns:
        extent *= n
    assert 2 ** 31 - 2 ** 17 < extent < 2 ** 31
    rng = np.random.default_rng(extent % 1000)
    edges = [0, 1, extent - 1, extent - 2, extent // 2]
    for d in (rows,) + tuple(ns):                         # around the multiples of every divisor
        if d > 1:
            edges += [d - 1, d, d + 1, (extent // d) * d - 1, (extent // d - 1) * d]
    flats = [f for f in edges if 0 <= f < extent] + [int(x) for x in rng.integers(0, extent, 20000)]
    assert _digits(driver, rows, ns, flats) == _want(rows, ns, flats), (rows, ns)
