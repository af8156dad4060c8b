"""The host side of the inner products with a CP tensor, on the CPU: the plan of ttsk_cp_gram (csrc/cp_gram_plan.h, plain
C++) compiled with the host compiler and checked before any kernel reads it -- the tile map covers every pair (j, j') with
total weight N M, the grid, partial and tile counts are those tests/cp_gram_ref.py restates, every refusal is listed; that
float64 NumPy stays inside the derived bounds of that module against np.longdouble (so the bounds can be relied on in the
GPU test); the host paths of ``CPTensor.dot`` / ``norm`` against dense evaluations and against runs of the reference."""

import numpy as np
import pytest

from tests import cp_gram_ref as cr
from tests.host_driver import compile_driver, run_driver

ARG, UNSUPPORTED = -2, -3

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "cp_gram_plan.h"
using namespace ttsk;
// plan <variant> d N M sym n_cu pad_a pad_b shape...   |   tile tn tm sym t...
int main(int argc, char **argv)
{
    if (argc >= 5 && !strcmp(argv[1], "tile")) {
        const int tn = atoi(argv[2]), tm = atoi(argv[3]), sym = atoi(argv[4]);
        for (int i = 5; i < argc; ++i) {
            const CpGramTile T = cp_gram_tile(tn, tm, sym, atoll(argv[i]));
            printf("tile %d %d %d\n", T.ti, T.tj, T.weight);
        }
        return 0;
    }
    if (argc < 10 || strcmp(argv[1], "plan")) return 2;
    const char *variant = argv[2];
    const int d = atoi(argv[3]);
    const int64_t N = atoll(argv[4]), M = atoll(argv[5]);
    const int sym = atoi(argv[6]), n_cu = atoi(argv[7]);
    const int64_t pad_a = atoll(argv[8]), pad_b = atoll(argv[9]);
    const int dd = d > 0 ? d : 0;
    if (argc != 10 + dd) return 2;
    std::vector<int64_t> shape, lda(dd, N + pad_a), ldb(dd, M + pad_b);
    for (int i = 0; i < dd; ++i) shape.push_back(atoll(argv[10 + i]));
    // addresses that are never read: factor k of a at 4096 (k + 1), of b behind them (sym: the same)
    std::vector<const double *> a, b;
    for (int k = 0; k < dd; ++k) {
        a.push_back((const double *)(uintptr_t)(4096 * (k + 1)));
        b.push_back(sym ? a.back() : (const double *)(uintptr_t)(4096 * (k + 1 + dd)));
    }
    double *out = (double *)(uintptr_t)8;
    const double *const *pa = a.data(), *const *pb = b.data();
    const int64_t *plda = lda.data(), *pldb = ldb.data(), *pshape = shape.data();
    if (!strcmp(variant, "null_a")) pa = nullptr;
    if (!strcmp(variant, "null_lda")) plda = nullptr;
    if (!strcmp(variant, "null_b")) pb = nullptr;
    if (!strcmp(variant, "null_ldb")) pldb = nullptr;
    if (!strcmp(variant, "null_shape")) pshape = nullptr;
    if (!strcmp(variant, "null_out")) out = nullptr;
    if (!strcmp(variant, "null_factor_a")) a[dd - 1] = nullptr;
    if (!strcmp(variant, "null_factor_b")) b[0] = nullptr;
    if (!strcmp(variant, "sym_other_ptr")) b[dd - 1] = a[dd - 1] + 1;
    if (!strcmp(variant, "sym_other_ld")) ldb[0] += 1;
    CpGramPlan p;
    const int rc = cp_gram_plan(pa, plda, N, pb, pldb, M, pshape, d, sym, out, n_cu, &p);
    printf("rc %d\nmsg %s\n", rc, p.msg);
    if (rc) return 0;
    printf("top %u %lld %lld %d %d %.17g %lld %zu %lld\n", p.grid, (long long)p.run, (long long)p.a.tiles, p.a.tn, p.a.tm, p.flops, (long long)p.depth,
           p.scratch, (long long)p.a.steps);
    printf("const %d %d %d %d %d %d %d %zu\n", CPG_TILE, CPG_KC, CPG_WG_PER_CU, CPG_TILE_SUMS, CPG_CLOSE_SUMS, CPG_MAX_MODES, CPG_PITCH, CPG_LDS);
    printf("args %d %d %d %d\n", p.a.d, p.a.sym, p.a.N, p.a.M);
    for (int k = 0; k < d; ++k)
        printf("mode %d %lld %lld %d %d\n", p.a.n[k], (long long)p.a.lda[k], (long long)p.a.ldb[k], p.a.a[k] == a[k], p.a.b[k] == b[k]);
    if (p.a.tiles <= 4096)
        for (int64_t t = 0; t < p.a.tiles; ++t) {
            const CpGramTile T = cp_gram_tile(p.a.tn, p.a.tm, p.a.sym, t);
            printf("tile %d %d %d\n", T.ti, T.tj, T.weight);
        }
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "cp_gram_plan", DRIVER)

    def run(*args):
        return run_driver(exe, args).splitlines()
    return run


def plan(driver, shape, N, M, sym, n_cu, pad_a=0, pad_b=0, variant="ok", d=None):
    out = driver("plan", variant, len(shape) if d is None else d, N, M, int(sym), n_cu, pad_a, pad_b, *shape)
    p = dict(rc=int(out[0].split()[1]), msg=out[1][4:], modes=[], tiles=[])
    for line in out[2:]:
        key, *v = line.split()
        if key == "tile":
            p["tiles"].append(tuple(int(x) for x in v))
        elif key == "mode":
            p["modes"].append([int(x) for x in v])
        else:
            p[key] = [float(x) if "." in x or "e" in x else int(x) for x in v]
    return p


def check_plan(p, case, n_cu):
    sym = case.M is None
    N, M = case.N, case.N if sym else case.M
    assert p["rc"] == 0, p["msg"]
    grid, run, tiles, tn, tm, flops, depth, scratch, steps = p["top"]
    assert steps == sum(-(-n // cr.KC) for n in case.shape)                        # the slabs of one tile through LDS
    assert p["const"][:6] == [cr.TILE, cr.KC, cr.WG_PER_CU, cr.TILE_SUMS, cr.CLOSE_SUMS, cr.MAX_MODES]
    pitch, lds = p["const"][6:]
    assert pitch >= cr.TILE and pitch % 16 == 0 and (2 * pitch) % 64 == 32          # the two rows of a half-wave read: disjoint banks
    assert lds == 2 * 2 * cr.KC * pitch * 8 <= 64 * 1024                           # static LDS of a workgroup
    assert p["args"] == [len(case.shape), int(sym), N, M]
    assert p["modes"] == [[n, N + case.pad_a, M + (case.pad_a if sym else case.pad_b), 1, 1] for n in case.shape]
    # ---- grid, partials, tiles, depth: the restatement's
    assert (tn, tm) == (-(-N // cr.TILE), -(-M // cr.TILE))
    assert tiles == cr.tiles(N, M, sym) and grid == cr.grid(N, M, sym, n_cu) and run == cr.run(N, M, sym, n_cu)
    assert 1 <= grid <= min(tiles, cr.WG_PER_CU * n_cu) and (grid == tiles or grid == cr.WG_PER_CU * n_cu)
    assert run == max(len(range(g, tiles, grid)) for g in range(grid))             # workgroup g owns g, g + grid, ...
    assert scratch == 8 * grid
    assert depth == cr.depth(case.shape, N, M, sym, n_cu)
    pairs = N * (N + 1) / 2 if sym else N * M
    assert flops == 2.0 * sum(case.shape) * pairs
    # ---- every (j, j') is covered, with total weight exactly N M
    assert len(p["tiles"]) == tiles and len(set(p["tiles"])) == tiles
    assert p["tiles"] == [cr.tile_of(tn, tm, sym, t) for t in range(tiles)]
    cover = np.zeros((tn, tm), dtype=np.int64)
    weight = 0
    for ti, tj, w in p["tiles"]:
        assert 0 <= ti < tn and 0 <= tj < tm
        rows, cols = min(cr.TILE, N - cr.TILE * ti), min(cr.TILE, M - cr.TILE * tj)
        assert rows >= 1 and cols >= 1
        weight += w * rows * cols
        cover[ti, tj] += 1
        if sym:
            assert ti <= tj and w == (2 if tj > ti else 1)
            if tj > ti:
                cover[tj, ti] += 1                                                  # the mirrored tile, counted by the weight
        else:
            assert w == 1
    assert (cover == 1).all() and weight == N * M


@pytest.mark.parametrize("n_cu", [1, 3, 256])
@pytest.mark.parametrize("case", cr.CASES, ids=lambda c: c.name)
def test_plan_of_every_gpu_case(driver, case, n_cu):
    sym = case.M is None
    check_plan(plan(driver, case.shape, case.N, case.N if sym else case.M, sym, n_cu, case.pad_a, case.pad_a if sym else case.pad_b), case, n_cu)


def test_cases_reach_their_edges():
    ns = {c.N for c in cr.CASES} | {c.M for c in cr.CASES if c.M is not None}
    assert {1, 15, 16, 17, 63, 64, 65, 129} <= ns
    assert {1, 3, 4, 5, 12} <= {n for c in cr.CASES for n in c.shape}
    assert any(n > cr.KC and n % cr.KC for c in cr.CASES for n in c.shape)           # a mode of more than one step, ragged
    assert {1, 2, 5, 8} <= {len(c.shape) for c in cr.CASES}
    assert any(c.pad_a and c.pad_b for c in cr.CASES)
    assert {16, 65, 129} <= {c.N for c in cr.CASES if c.M is None}
    assert all(c.M != c.N for c in cr.CASES if c.M is not None and c.N > 1)
    for sym in (False, True):
        over = [c for c in cr.CASES if (c.M is None) == sym and cr.run(c.N, c.N if sym else c.M, sym, cr.CHIP_CUS) >= 2]
        assert over and all(c.shape == (2, 2) for c in over)


def test_tile_map_of_the_widest_triangle(driver):
    """tn = 2^25 tile rows (N just below 2^31): first, last and middle tiles of chosen rows, where the square root of the
    map is at its least exact"""
    tn = 2 ** 25
    start = lambda ti: ti * tn - ti * (ti - 1) // 2
    rows = [0, 1, 2, 12345, 2 ** 24, tn - 3, tn - 2, tn - 1]
    ts, want = [], []
    for ti in rows:
        for off in sorted({0, 1, (tn - ti) // 2, tn - ti - 1}):
            if off < tn - ti:
                ts.append(start(ti) + off)
                want.append((ti, ti + off, 2 if off else 1))
    assert ts[-1] == tn * (tn + 1) // 2 - 1
    got = [tuple(int(x) for x in line.split()[1:]) for line in driver("tile", tn, tn, 1, *ts)]
    assert got == want
    got = [tuple(int(x) for x in line.split()[1:]) for line in driver("tile", tn, 7, 0, 0, 6, 7, 7 * tn - 1)]
    assert got == [(0, 0, 1), (0, 6, 1), (1, 0, 1), (tn - 1, 6, 1)]


def test_every_refusal(driver):
    shape = (3, 4)
    ok = plan(driver, shape, 5, 6, False, 256)
    assert ok["rc"] == 0
    for variant in ("null_a", "null_lda", "null_b", "null_ldb", "null_shape", "null_out", "null_factor_a", "null_factor_b"):
        p = plan(driver, shape, 5, 6, False, 256, variant=variant)
        assert p["rc"] == ARG and "NULL" in p["msg"], variant
    assert plan(driver, (), 5, 6, False, 256)["rc"] == ARG                                   # d = 0
    assert plan(driver, (), 5, 6, False, 256, d=-1)["rc"] == ARG
    for N, M, sh in ((0, 6, shape), (5, 0, shape), (5, 6, (3, 0)), (-1, 6, shape), (5, 6, (-2, 4))):
        assert plan(driver, sh, N, M, False, 256)["rc"] == ARG, (N, M, sh)
    assert plan(driver, shape, 5, 6, False, 256, pad_a=-1)["rc"] == ARG                      # lda = N - 1
    assert plan(driver, shape, 5, 6, False, 256, pad_b=-1)["rc"] == ARG
    assert plan(driver, shape, 5, 5, True, 256)["rc"] == 0
    assert plan(driver, shape, 5, 6, True, 256, pad_a=1)["rc"] == ARG                        # sym with M != N
    assert plan(driver, shape, 5, 5, True, 256, variant="sym_other_ptr")["rc"] == ARG
    assert plan(driver, shape, 5, 5, True, 256, variant="sym_other_ld")["rc"] == ARG
    # ---- the cover
    assert plan(driver, (2,) * 32, 5, 6, False, 256)["rc"] == 0
    p = plan(driver, (2,) * 33, 5, 6, False, 256)
    assert p["rc"] == UNSUPPORTED and "33 modes" in p["msg"]
    big = 2 ** 31
    assert plan(driver, shape, big - 1, 6, False, 256)["rc"] == 0 and plan(driver, shape, 5, big - 1, False, 256)["rc"] == 0
    assert plan(driver, (3, big - 1), 5, 6, False, 256)["rc"] == 0
    assert plan(driver, shape, big - 1, big - 1, True, 256)["rc"] == 0
    for N, M, sh in ((big, 6, shape), (5, big, shape), (5, 6, (big, 4)), (5, 6, (3, 2 ** 40))):
        assert plan(driver, sh, N, M, False, 256)["rc"] == UNSUPPORTED, (N, M, sh)
    assert plan(driver, shape, big, big, True, 256)["rc"] == UNSUPPORTED
    # a refusal of the arguments comes before one of the cover, except for d itself
    assert plan(driver, (big, 0), 5, 6, False, 256)["rc"] == ARG


@pytest.mark.parametrize("case", cr.CASES, ids=lambda c: c.name)
def test_float64_gram_is_inside_the_bound_of_longdouble(case):
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("np.longdouble is no wider than float64 on this host: the bound cannot be checked")
    sym = case.M is None
    A, B = cr.operands(case, *cr.case_factors(case))
    G, ref = cr.gram(A, B), cr.gram(A, B, dtype=np.longdouble)
    neg = np.signbit(np.concatenate([x.ravel() for x in A + B]))
    assert neg.size < 8 or (neg.any() and not neg.all())                            # entries of both signs
    for n_cu in (1, 256):
        tol = cr.bound(A, B, sym, n_cu)
        assert abs(G - ref) <= tol, (case.name, abs(G - ref) / tol)
    assert cr.gram(A, B, absolute=True) >= abs(G)


TT_CP_SHAPES = [((7,), (), 5), ((3, 4), (1,), 1), ((4, 1, 5), (16, 17), 33), ((2, 3, 2, 3, 2), (3, 9, 9, 2), 65)]


@pytest.mark.parametrize("spec", TT_CP_SHAPES, ids=lambda s: f"d{len(s[0])}_N{s[2]}")
def test_tt_cp_restatement_against_dense_and_longdouble(spec):
    shape, ranks, N = spec
    rng = np.random.default_rng(N)
    cores, V = cr.random_tt(rng, shape, ranks), [rng.standard_normal((n, N)) for n in shape]
    import tt_sketch_amd as tsa
    tt, cp = tsa.TensorTrain(cores), tsa.CPTensor(V)
    dense = float(np.dot(tt.to_numpy().ravel(), cp.to_numpy().ravel()))
    got, ref = cr.tt_cp_dot(cores, V), cr.tt_cp_dot(cores, V, dtype=np.longdouble)
    tol = cr.tt_cp_bound(cores, V)
    assert abs(got - ref) <= tol
    assert abs(dense - ref) <= 1e-12 * float(cr.tt_cp_dot(cores, V, absolute=True))
    # two host objects keep the NumPy path, bit for bit, and upload nothing
    assert cp.dot(tt) == dense == tt.dot(cp)
    assert cp._dev is None and tt._dev is None
    assert cp.norm() == float(np.sqrt(abs(np.dot(cp.to_numpy().ravel(), cp.to_numpy().ravel()))))
    assert cp._dev is None


@pytest.mark.parametrize("case", cr.load_cases(), ids=lambda c: c["name"])
def test_restatement_and_host_paths_against_reference_runs(case):
    import tt_sketch_amd as tsa
    A, B, cores = case["factors_a"], case["factors_b"], case["cores"]
    assert abs(cr.gram(A, A) - case["norm_a"] ** 2) <= 1e-12 * float(cr.gram(A, A, absolute=True))
    assert abs(cr.gram(B, B) - case["norm_b"] ** 2) <= 1e-12 * float(cr.gram(B, B, absolute=True))
    assert abs(cr.gram(A, B) - case["dot_ab"]) <= 1e-12 * float(cr.gram(A, B, absolute=True))
    assert abs(cr.tt_cp_dot(cores, A) - case["dot_tt_a"]) <= 1e-12 * float(cr.tt_cp_dot(cores, A, absolute=True))
    assert case["dot_a_tt"] == case["dot_tt_a"] or abs(case["dot_a_tt"] - case["dot_tt_a"]) <= 1e-12 * abs(case["dot_tt_a"])
    want = cr.fast_error(case["norm_tt"], case["norm_a"], case["dot_tt_a"], relative=True)
    assert abs(want - case["error_tt_a"]) <= 1e-12 * want
    # the host objects of the package: the reference's dense path
    a, b, tt = tsa.CPTensor(A), tsa.CPTensor(B), tsa.TensorTrain(cores)
    assert abs(a.norm() - case["norm_a"]) <= 1e-12 * case["norm_a"]
    assert abs(a.dot(b) - case["dot_ab"]) <= 1e-12 * float(cr.gram(A, B, absolute=True))
    assert abs(tt.dot(a) - case["dot_tt_a"]) <= 1e-12 * float(cr.tt_cp_dot(cores, A, absolute=True))
    assert abs(tt.error(a, fast=True, relative=True) - case["error_tt_a"]) <= 1e-9 * case["error_tt_a"]
    assert abs(a.error(tt, fast=True, relative=True) - case["error_a_tt"]) <= 1e-9 * case["error_a_tt"]
    assert a._dev is None and b._dev is None and tt._dev is None


def test_cp_gram_checks_its_arguments_before_the_device():
    import tt_sketch_amd as tsa
    rng = np.random.default_rng(0)
    a = tsa.CPTensor([rng.standard_normal((n, 3)) for n in (4, 5)])
    b = tsa.CPTensor([rng.standard_normal((n, 2)) for n in (4, 6)])
    tt = tsa.TensorTrain(cr.random_tt(rng, (4, 5), (2,)))
    with pytest.raises(TypeError):
        tsa.cp_gram(tt)
    with pytest.raises(TypeError):
        tsa.cp_gram(a, tt)
    with pytest.raises(ValueError):
        tsa.cp_gram(a, b)
    assert a._dev is None and b._dev is None and tt._dev is None
    assert "cp_gram" in tsa.__all__
