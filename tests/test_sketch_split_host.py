"""The CU budgets of the one-call TT sketch (csrc/sketch_split.h) on the host: the policy's invariants over device sizes and
batch sizes, its full-width cases, the committed split, and that every budget it hands out is one the plan functions of the
kernels it goes to (chain_fused_plan, psi_stream_plan) accept with a grid inside the budget.  No GPU.

The calls the budgets are fed to: the benchmark's C3 call (d = 6, n = 200, TT rank 100, l = 50 / r = 100), the same with
r = 52 (the chains' work nearly equal) and the small calls of tests/test_gpu_sketch_split.py.  The driver asks the policy
with at most SK_MAXB tensors (larger batches are sliced first), so the plans are fed for nb <= SK_MAXB; the policy's own
invariants are checked for every nb.  A budget of 0 stands for the whole device (the Psi products always get it: no budget
for them paid when it was measured), so the bounds below are those of the budgets that are not 0."""
import pytest

from tests.host_driver import compile_driver, run_driver

N_CUS = (20, 64, 256, 304)
NBS = (1, 2, 3, 16, 32, 48)
# (n_cu, nb, call) -> (right, left, psi): the split measured at C3 (DESIGN.md "CU budgets") and what the rule makes of it at r = 52
COMMITTED_SPLIT = {(256, 32, "c3"): (160, 64, 0), (256, 32, "r52"): (128, 96, 0)}

# name, interior mode size, TT rank, left DRM rank, right DRM rank
CALLS = (("c3", 200, 100, 50, 100), ("r52", 200, 100, 50, 52), ("small_a", 5, 68, 36, 68), ("small_a7", 7, 68, 36, 68), ("small_b", 4, 100, 50, 100))
MODE_SIZE = {c[0]: c[1] for c in CALLS}

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "sketch_split.h"
#include "chain_plan.h"
#include "psi_plan.h"
using namespace ttsk;

static const double *W[SK_MAXB], *X[SK_MAXB], *S[SK_MAXB];
static double *T[SK_MAXB], *Out[SK_MAXB];

// an interior chain step of TT rank s on DRM rank a, mode size n, as tt_fused.hip describes it (right: the transposed core)
static int chain(int nb, int n, int s, int a, bool left, int cus, int &grid, int &wpp)
{
    const ChainStepArgs c = left ? ChainStepArgs{nb, n, s, a, a, s, W, a, X, 1, s, (int64_t)n * s, (int64_t)s * n * s, (const double *)0x10000000ull, T, Out}
                                 : ChainStepArgs{nb, n, s, a, a, s, W, a, X, (int64_t)n * s, s, 1, (int64_t)s * n * s, (const double *)0x10000000ull, nullptr, Out};
    ChainFusedPlan p;
    const int rc = chain_fused_plan(c, cus, false, p);
    grid = rc == 1 ? p.l.grid : 0; wpp = rc == 1 ? p.a.wpp : 0;
    return rc;
}

static int psi(int nb, int J, int s, int r, int cus, int &grid, int &wpp)
{
    const StreamSmallArgs c{nb, J, s, r, S, s, W, r, Out, r, 0};
    PsiStreamPlan p;
    const int rc = psi_stream_plan(c, cus, p);
    grid = rc == 1 ? p.l.grid : 0; wpp = rc == 1 ? p.a.wpp : 0;
    return rc;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const int n_cu = atoi(argv[1]), nb = atoi(argv[2]);
    for (int b = 0; b < SK_MAXB; ++b) {            // never dereferenced: integers cast to pointers
        W[b] = (const double *)(0x30000000ull + 0x100000ull * b); X[b] = (const double *)(0x20000000ull + 0x100000ull * b);
        S[b] = (const double *)(0x60000000ull + 0x100000ull * b);
        T[b] = (double *)(0x40000000ull + 0x100000ull * b); Out[b] = (double *)(0x50000000ull + 0x100000ull * b);
    }
    printf("const min_nb=%d min_wpp=%d maxb=%d\n", SPLIT_MIN_NB, SPLIT_MIN_WPP, SK_MAXB);
    // argv[3..] = name n s l r, five words per call: a d = 6 sketch of that signature in every mode
    for (int i = 3; i + 4 < argc; i += 5) {
        const char *name = argv[i];
        const int n = atoi(argv[i + 1]), s = atoi(argv[i + 2]), l = atoi(argv[i + 3]), r = atoi(argv[i + 4]);
        const int64_t nn[6] = {n, n, n, n, n, n}, ss[7] = {1, s, s, s, s, s, 1}, lt[6] = {1, l, l, l, l, l}, rt[6] = {1, r, r, r, r, r};
        // the policy: (two streams, pipelined, family) variants
        for (int two = 0; two < 2; ++two)
            for (int pipe = 0; pipe < 2; ++pipe)
                for (int fam = 0; fam < 2; ++fam) {
                    const SketchSplit sp = sketch_split_policy(SketchSplitIn{n_cu, nb, 6, nn, ss, lt, rt, two != 0, pipe != 0, fam ? SKETCH_OTHER : SKETCH_FUSED});
                    printf("policy %s n=%d two=%d pipe=%d fam=%d right=%d left=%d psi=%d\n", name, n, two, pipe, fam, sp.right, sp.left, sp.psi);
                }
        const SketchSplitIn in{n_cu, nb, 6, nn, ss, lt, rt, true, true, SKETCH_FUSED};
        const SketchSplit sp = sketch_split_policy(in);
        double wr, wl;
        sketch_chain_work(in, wr, wl);
        printf("work %s right=%.17g left=%.17g\n", name, wr, wl);
        // resolve: a process-wide setting over the policy
        const int sets[4][3] = {{-1, -1, -1}, {0, 0, 0}, {7, -1, 100000}, {-1, 0, 5}};
        for (const auto &st : sets) {
            const SketchSplit rs = sketch_split_resolve(in, st);
            printf("resolve %s set=%d,%d,%d right=%d left=%d psi=%d pol=%d,%d,%d\n", name, st[0], st[1], st[2], rs.right, rs.left, rs.psi, sp.right, sp.left, sp.psi);
        }
        if (nb > SK_MAXB) continue;
        // the plans under the policy's budgets
        int g, w, g0, w0;
        int rc = chain(nb, n, s, r, false, sp.right ? sp.right : n_cu, g, w), rc0 = chain(nb, n, s, r, false, n_cu, g0, w0);
        printf("plan %s right budget=%d rc=%d grid=%d wpp=%d rc_full=%d grid_full=%d\n", name, sp.right, rc, g, w, rc0, g0);
        rc = chain(nb, n, s, l, true, sp.left ? sp.left : n_cu, g, w), rc0 = chain(nb, n, s, l, true, n_cu, g0, w0);
        printf("plan %s left budget=%d rc=%d grid=%d wpp=%d rc_full=%d grid_full=%d\n", name, sp.left, rc, g, w, rc0, g0);
        rc = psi(nb, l * n, s, r, sp.psi ? sp.psi : n_cu, g, w), rc0 = psi(nb, l * n, s, r, n_cu, g0, w0);
        printf("plan %s psi budget=%d rc=%d grid=%d wpp=%d rc_full=%d grid_full=%d\n", name, sp.psi, rc, g, w, rc0, g0);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """{(n_cu, nb): {kind: rows}} -- every row a dict of the driver's fields, `call` the name of the call it is about"""
    exe = compile_driver(tmp_path_factory, "sketch_split", DRIVER)
    calls = [str(x) for c in CALLS for x in c]
    out = {}
    for n_cu in N_CUS:
        for nb in NBS:
            rows = {"const": [], "policy": [], "work": [], "resolve": [], "plan": []}
            for line in run_driver(exe, [n_cu, nb] + calls).splitlines():
                w = line.split()
                f = dict(x.split("=", 1) for x in w[1:] if "=" in x)
                if w[0] != "const":
                    f["call"] = w[1]
                if w[0] == "plan":
                    f["cls"] = w[2]
                rows[w[0]].append(f)
            out[(n_cu, nb)] = rows
    return out


def budgets(row):
    return int(row["right"]), int(row["left"]), int(row["psi"])


def wpp_full(n_cu, nb, row):
    """workgroups per tensor at full width: the device's share, at most one per slice"""
    return min(n_cu // nb, MODE_SIZE[row["call"]])


def test_every_budget_is_whole_workgroups_per_tensor_within_the_device(answers):
    seen_split = 0
    for (n_cu, nb), rows in answers.items():
        for row in rows["policy"]:
            b = budgets(row)
            assert (b[0] == 0) == (b[1] == 0), (n_cu, nb, row)               # the two chains are split together or not at all
            if b[0] == 0:
                assert b == (0, 0, 0), (n_cu, nb, row)
                continue
            seen_split += 1
            for x in b:
                if x:
                    assert nb <= x <= n_cu, (n_cu, nb, row)
                    assert x % nb == 0 and x // nb >= 1, (n_cu, nb, row)      # budget / nb is the plan's wpp, nothing left over
            assert b[0] + b[1] <= n_cu, (n_cu, nb, row)                      # the two chains side by side
            assert b[0] // nb + b[1] // nb == wpp_full(n_cu, nb, row) - 1, (n_cu, nb, row)   # one workgroup per tensor stays free
    assert seen_split > 0


def test_full_width_in_each_stated_case(answers):
    for (n_cu, nb), rows in answers.items():
        min_nb, min_wpp = int(rows["const"][0]["min_nb"]), int(rows["const"][0]["min_wpp"])
        for row in rows["policy"]:
            full = budgets(row) == (0, 0, 0)
            reasons = [row["two"] == "0",                         # TTSK_SINGLE_STREAM=1, or one chain only
                       row["pipe"] == "0",                        # one step in flight: a split only lengthens it
                       row["fam"] == "1",                         # a step that is not on the fused kernel
                       nb == 1, nb < min_nb,                      # a single tensor; few tensors
                       wpp_full(n_cu, nb, row) < min_wpp]         # a budget would fall below nb
            assert full == any(reasons), (n_cu, nb, row)          # ... and a split everywhere else


def test_the_split_follows_the_work_of_the_chains(answers):
    for (n_cu, nb), rows in answers.items():
        work = {w["call"]: (float(w["right"]), float(w["left"])) for w in rows["work"]}
        for row in rows["policy"]:
            b = budgets(row)
            if b[0] == 0:
                continue
            wr, wl = work[row["call"]]
            share = wpp_full(n_cu, nb, row) - 1
            ideal = share * wr / (wr + wl)
            got = b[0] // nb
            assert abs(got - ideal) <= 0.5 + 1e-9 or got in (1, share - 1), (n_cu, nb, row, ideal)
    # C3: the right chain has 8 / 3 of the left chain's work
    wr, wl = next((float(w["right"]), float(w["left"])) for w in answers[(256, 32)]["work"] if w["call"] == "c3")
    assert wr / wl == pytest.approx((100 * 100 + 100 * 100) / (100 * 50 + 50 * 50))


def test_the_committed_split(answers):
    for (n_cu, nb, call), want in COMMITTED_SPLIT.items():
        got = [budgets(r) for r in answers[(n_cu, nb)]["policy"] if r["call"] == call and r["two"] == r["pipe"] == "1" and r["fam"] == "0"]
        assert got == [want]


def test_a_setting_goes_over_the_policy_per_class(answers):
    for (n_cu, nb), rows in answers.items():
        for row in rows["resolve"]:
            pol = tuple(int(x) for x in row["pol"].split(","))
            want = tuple(p if s < 0 else min(s, n_cu) for s, p in zip((int(x) for x in row["set"].split(",")), pol))
            assert budgets(row) == want, (n_cu, nb, row)


def test_the_plans_accept_every_budget_with_a_grid_inside_it(answers):
    fed = 0
    for (n_cu, nb), rows in answers.items():
        for row in rows["plan"]:
            budget, rc, rc_full, grid = (int(row[k]) for k in ("budget", "rc", "rc_full", "grid"))
            assert rc == rc_full, (n_cu, nb, row)                  # a budget never changes whether a kernel covers the call
            if row["cls"] != "psi" or row["call"] in ("c3", "r52"):
                assert rc == 1, (n_cu, nb, row)                     # (the small calls' Psi products, l n < 1024 rows, are not on the streamed kernel)
            if budget and rc == 1:
                fed += 1
                assert 0 < grid <= budget, (n_cu, nb, row)
                if row["cls"] != "psi":
                    assert int(row["wpp"]) == min(budget // nb, MODE_SIZE[row["call"]]), (n_cu, nb, row)
            if not budget and rc == 1:
                assert grid == int(row["grid_full"])
    assert fed > 0
