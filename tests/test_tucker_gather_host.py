"""The host side of the Tucker arithmetic, on the CPU: the plan of ttsk_tucker_gather (csrc/tucker_gather_plan.h, plain
C++) compiled with the host compiler and held against the restatement of tests/tucker_ref.py -- the split of the modes,
the chunks, the LDS bytes, the grid as a function of N and the CU count, every refusal, a table of tags that reaches every
branch; that float64 NumPy stays inside the derived bars of that module against np.longdouble (so the bars can be relied
on in the GPU test); the restatement against runs of the reference; and what the Python layer does before it touches the
device."""

import numpy as np
import pytest

from tests import tucker_ref as tr
from tests.host_driver import compile_driver, run_driver

ARG, UNSUPPORTED = -2, -3

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "tucker_gather_plan.h"
using namespace ttsk;
// plan <variant> d N n_cu stride_pad reverse ranks... shape...
int main(int argc, char **argv)
{
    if (argc < 8 || strcmp(argv[1], "plan")) return 2;
    const char *variant = argv[2];
    const int d = atoi(argv[3]);
    const size_t N = (size_t)atoll(argv[4]);
    const int n_cu = atoi(argv[5]);
    const long long pad = atoll(argv[6]);
    const int reverse = atoi(argv[7]);
    const int dd = d > 0 ? d : 0;
    if (argc != 8 + 2 * dd) return 2;
    std::vector<int64_t> ranks, shape;
    for (int i = 0; i < dd; ++i) ranks.push_back(atoll(argv[8 + i]));
    for (int i = 0; i < dd; ++i) shape.push_back(atoll(argv[8 + dd + i]));
    // addresses that are never read
    std::vector<const void *> fac;
    std::vector<int> order;
    for (int k = 0; k < dd; ++k) {
        fac.push_back((const void *)(uintptr_t)(4096 * (k + 1)));
        order.push_back(reverse ? dd - 1 - k : k);
    }
    const void *core = (const void *)(uintptr_t)64, *idx = (const void *)(uintptr_t)128, *val = (const void *)(uintptr_t)192;
    const void *out = (const void *)(uintptr_t)256, *stats = (const void *)(uintptr_t)320;
    const void *const *pfac = fac.data();
    const int64_t *pranks = ranks.data(), *pshape = shape.data();
    const int *porder = reverse ? order.data() : nullptr;
    if (!strcmp(variant, "null_core")) core = nullptr;
    if (!strcmp(variant, "null_factors")) pfac = nullptr;
    if (!strcmp(variant, "null_ranks")) pranks = nullptr;
    if (!strcmp(variant, "null_shape")) pshape = nullptr;
    if (!strcmp(variant, "null_factor")) fac[dd - 1] = nullptr;
    if (!strcmp(variant, "null_idx")) idx = nullptr;
    if (!strcmp(variant, "no_output")) out = stats = nullptr;
    if (!strcmp(variant, "stats_without_val")) val = nullptr;
    if (!strcmp(variant, "out_only")) { stats = nullptr; val = nullptr; }
    if (!strcmp(variant, "bad_order")) { order[0] = -1; porder = order.data(); }
    TuckerGatherPlan p;
    const int rc = tucker_gather_plan(core, pfac, pranks, pshape, d, idx, (int64_t)N + pad, porder, N, val, out, stats, n_cu, &p);
    printf("rc %d\nmsg %s\n", rc, p.msg);
    if (rc) return 0;
    printf("top %d %d %d %d %d %zu %u %lld %lld %lld %.17g\n", p.a.m, p.a.P, p.a.Q, p.ct, p.chunks, p.lds, p.grid, (long long)p.run,
           (long long)p.depth, (long long)p.stat_depth, p.flops);
    printf("const %d %lld %d %d %d %d %d %d %zu %d %d\n", TKG_MAX_MODES, (long long)TKG_MAX_CORE, TKG_TILES, TKG_BATCH, TKG_MAX_CT, TKG_KC,
           TKG_A_PITCH, TKG_WG_PER_CU, TKG_LDS_LIMIT, TKG_TAIL_SUMS, TKG_BLOCK_SUMS);
    printf("pitch %d %d %d\n", tkg_b_pitch(1), tkg_b_pitch(2), tkg_b_pitch(4));
    printf("args %d %d\n", p.a.d, p.a.core == core);
    for (int k = 0; k < d; ++k) printf("mode %d %lld %d %d\n", p.a.s[k], (long long)p.a.n[k], p.a.fac[k] == fac[k], p.row[k]);
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "tucker_gather_plan", DRIVER)

    def run(*args):
        return run_driver(exe, args).splitlines()
    return run


def plan(driver, ranks, shape, N, n_cu=tr.CHIP_CUS, pad=0, reverse=False, variant="ok", d=None):
    out = driver("plan", variant, len(ranks) if d is None else d, N, n_cu, pad, int(reverse), *ranks, *shape)
    p = dict(rc=int(out[0].split()[1]), msg=out[1][4:], modes=[])
    for line in out[2:]:
        key, *v = line.split()
        vals = [float(x) if "." in x or "e" in x else int(x) for x in v]
        if key == "mode":
            p["modes"].append(vals)
        else:
            p[key] = vals
    return p


def check_plan(p, ranks, shape, N, n_cu, reverse=False):
    assert p["rc"] == 0, p["msg"]
    want = tr.plan(ranks, N, n_cu)
    m, P, Q, ct, chunks, lds, grid, run, depth, stat_depth, flops = p["top"]
    assert dict(m=m, P=P, Q=Q, ct=ct, chunks=chunks, lds=lds, grid=grid, run=run, depth=depth, stat_depth=stat_depth,
                flops=flops) == want
    assert p["const"] == [tr.MAX_MODES, tr.MAX_CORE, tr.TILES, tr.BATCH, tr.MAX_CT, tr.KC, tr.A_PITCH, tr.WG_PER_CU, tr.LDS_LIMIT,
                          tr.TAIL_SUMS, tr.BLOCK_SUMS]
    d = len(ranks)
    # ---- the split: the leading modes are the rows, the trailing ones the columns, in at most four column tiles
    assert 1 <= m <= d and P == tr.prod(ranks[:m]) and Q == tr.prod(ranks[m:]) and P * Q == tr.prod(ranks)
    assert Q <= 16 * tr.MAX_CT and ct in (1, 2, 4) and 16 * ct >= Q
    assert all(tr.split_cost(tr.prod(ranks[:m]), Q, d, m) <= tr.split_cost(tr.prod(ranks[:mm]), tr.prod(ranks[mm:]), d, mm)
               for mm in range(1, d + 1) if tr.prod(ranks[mm:]) <= 16 * tr.MAX_CT)
    # ---- the chunks and the LDS: conflict-free pitches, the workgroup's bytes inside the limit, a wave's 64 tuples per row of A
    assert chunks == -(-P // tr.KC) and tr.KC % 4 == 0
    assert p["pitch"] == [tr.b_pitch(c) for c in (1, 2, 4)]
    for c, pitch in zip((1, 2, 4), p["pitch"]):
        assert pitch >= 16 * c and pitch % 32 == 16
    assert tr.A_PITCH >= 16 * tr.TILES and tr.A_PITCH % 32 == 16 and tr.BATCH == 4 * 16 * tr.TILES
    assert lds == (tr.KC * tr.b_pitch(ct) + 4 * tr.KC * tr.A_PITCH + 256) * 8 + 4 * d * 64 * 4 <= tr.LDS_LIMIT < 64 * 1024
    # ---- the grid: a function of N and the CU count alone
    batches = -(-N // tr.BATCH)
    assert grid == min(batches, tr.WG_PER_CU * n_cu)
    assert run == (max(len(range(g, batches, grid)) for g in range(grid)) if grid else 0)
    assert flops == 2.0 * tr.prod(ranks) * N
    assert depth == d + 4 * -(-P // 4) + tr.TAIL_SUMS
    assert p["args"] == [d, 1]
    order = list(range(d))[::-1] if reverse else list(range(d))
    assert p["modes"] == [[s, n, 1, order[k]] for k, (s, n) in enumerate(zip(ranks, shape))]


@pytest.mark.parametrize("n_cu", [1, 3, 256])
@pytest.mark.parametrize("case", tr.CASES, ids=lambda c: c[0])
def test_plan_of_every_gpu_case(driver, case, n_cu):
    tag, ranks, shape, N, reverse, pad = case
    check_plan(plan(driver, ranks, shape, N, n_cu, pad, reverse), ranks, shape, N, n_cu, reverse)


def test_grid_depends_on_n_and_cus_alone(driver):
    for N in (0, 1, 255, 256, 257, 768 * 256, 768 * 256 + 1, 10 ** 7):
        a = plan(driver, (16, 16, 16), (200, 200, 200), N)
        b = plan(driver, (2, 3), (5, 2 ** 31 - 1), N, reverse=True, pad=11, variant="out_only")
        assert a["rc"] == b["rc"] == 0
        assert a["top"][6:8] == b["top"][6:8] == [tr.plan((2, 3), N)["grid"], tr.plan((2, 3), N)["run"]]
    assert plan(driver, (4,), (4,), 0)["top"][6] == 0
    assert plan(driver, (4,), (4,), 10 ** 7, n_cu=256)["top"][6] == 256 * tr.WG_PER_CU and plan(driver, (4,), (4,), 10 ** 7, n_cu=0)["top"][6] == tr.WG_PER_CU


# tag -> the branch of the plan it reaches, as the restatement sees it
BRANCHES = {
    "d1_q1": lambda p, r: len(r) == 1 and p["Q"] == 1 and p["chunks"] == 1,
    "d1_two_chunks": lambda p, r: len(r) == 1 and p["chunks"] == 2 and p["P"] % 4,
    "d2_rank1": lambda p, r: p["P"] * p["Q"] == 1,
    "d2_ct1_full": lambda p, r: p["Q"] == 16 and p["ct"] == 1 and p["P"] == tr.KC,
    "d2_ct2": lambda p, r: p["ct"] == 2 and p["Q"] % 16,
    "d2_ct3_as_4": lambda p, r: -(-p["Q"] // 16) == 3 and p["ct"] == 4,
    "d2_ct4": lambda p, r: p["Q"] == 64 and p["ct"] == 4,
    "d2_q_over_64": lambda p, r: r[-1] > 64 and p["m"] == len(r) and p["Q"] == 1,
    "d3_chunks": lambda p, r: p["chunks"] > 2 and p["ct"] == 4 and -(-p["Q"] // 16) == 3,
    "d3_unit_mode": lambda p, r: 1 in r,
    "d3_mixed": lambda p, r: p["m"] == 2 and p["ct"] == 1 and p["chunks"] == 17,
    "d5_r4": lambda p, r: 1 < p["m"] < len(r) - 1,
    "d5_mixed": lambda p, r: len(r) == 5 and r[0] == 1,
    "d8_r2": lambda p, r: len(r) == 8 and p["m"] >= 3,
    "d8_slow_odometer": lambda p, r: len(r) == 8 and p["m"] >= 4 and 1 in r[:p["m"] - 1],
}


def test_cases_reach_every_branch():
    assert set(BRANCHES) == {c[0] for c in tr.CASES}
    for tag, ranks, shape, N, reverse, pad in tr.CASES:
        assert BRANCHES[tag](tr.plan(ranks, N), ranks), (tag, tr.plan(ranks, N))
    assert {1, 2, 3, 5, 8} <= {len(c[1]) for c in tr.CASES}
    assert {1, 3, 4, 5, 16, 17} <= {s for c in tr.CASES for s in c[1]}
    assert {1, 15, 16, 17, 63, 64, 65} <= {c[3] for c in tr.CASES}
    assert any(c[3] < tr.BATCH and c[3] > 65 for c in tr.CASES) and any(c[3] > 2 * tr.BATCH and c[3] % tr.BATCH for c in tr.CASES)
    assert any(1 in c[2] for c in tr.CASES) and any(c[4] and c[5] for c in tr.CASES)
    assert {1, 2, 4} <= {tr.plan(c[1], c[3])["ct"] for c in tr.CASES}


def test_every_refusal(driver):
    ranks, shape = (3, 4), (5, 6)
    assert plan(driver, ranks, shape, 10)["rc"] == 0
    assert plan(driver, ranks, shape, 10, variant="out_only")["rc"] == 0
    for variant in ("null_core", "null_factors", "null_ranks", "null_shape", "null_factor", "null_idx"):
        p = plan(driver, ranks, shape, 10, variant=variant)
        assert p["rc"] == ARG and "NULL" in p["msg"], variant
    assert plan(driver, ranks, shape, 0, variant="null_idx")["rc"] == 0              # an empty list needs no index matrix
    assert plan(driver, ranks, shape, 10, variant="no_output")["rc"] == ARG
    p = plan(driver, ranks, shape, 10, variant="stats_without_val")
    assert p["rc"] == ARG and "dev_val" in p["msg"]
    assert plan(driver, ranks, shape, 10, variant="bad_order")["rc"] == ARG
    assert plan(driver, (), (), 10)["rc"] == ARG                                      # d = 0
    assert plan(driver, (), (), 10, d=-1)["rc"] == ARG
    assert plan(driver, ranks, shape, 10, pad=-1)["rc"] == ARG                        # row_stride below N
    for rk, sh in (((0, 4), shape), ((3, -1), shape), (ranks, (0, 6)), (ranks, (5, -2))):
        assert plan(driver, rk, sh, 10)["rc"] == ARG, (rk, sh)
    # ---- the cover: d <= 8, a core of up to 2^20 entries, any mode below 2^31
    assert plan(driver, (2,) * 8, (3,) * 8, 10)["rc"] == 0
    p = plan(driver, (2,) * 9, (3,) * 9, 10)
    assert p["rc"] == UNSUPPORTED and "9 modes" in p["msg"]
    big = 2 ** 31
    assert plan(driver, ranks, (5, big - 1), 10)["rc"] == 0
    assert plan(driver, ranks, (big, 6), 10)["rc"] == UNSUPPORTED
    for rk in ((2 ** 20,), (1024, 1024), (4,) * 8, (5,) * 8, (32, 32, 32, 32), (2 ** 10, 2 ** 5, 2 ** 5)):
        sh = tuple(max(r, 2) for r in rk)
        assert plan(driver, rk, sh, 10)["rc"] == 0, rk
        check_plan(plan(driver, rk, sh, 10 ** 6), rk, sh, 10 ** 6, tr.CHIP_CUS)
    for rk in ((2 ** 20 + 1,), (1024, 1025), (2 ** 40, 2 ** 40), (2 ** 62, 4), (6,) * 8, (2 ** 21, 1)):
        p = plan(driver, rk, (7,) * len(rk), 10)
        assert p["rc"] == UNSUPPORTED and "2^20" in p["msg"], rk
    # a refusal of the arguments comes before one of the cover, except for d itself
    assert plan(driver, (2 ** 21, 0), (5, 6), 10)["rc"] == ARG
    assert plan(driver, (2,) * 9, (0,) * 9, 10)["rc"] == UNSUPPORTED


def _longdouble_is_wider():
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("np.longdouble is no wider than float64 on this host: the bars cannot be checked")


@pytest.mark.parametrize("case", tr.CASES, ids=lambda c: c[0])
def test_float64_gather_is_inside_the_bar_of_longdouble(case):
    _longdouble_is_wider()
    tag, ranks, shape, N, _, _ = case
    factors, core, idx, val = tr.case_data(tag, ranks, shape, N)
    t, truth = tr.gather(factors, core, idx), tr.gather(factors, core, idx, dtype=np.longdouble)
    bar = tr.entry_bar(factors, core, idx)
    assert (np.abs(t - truth) <= bar).all(), float(np.max(np.abs(t - truth) / bar))
    assert (N == 1 or (idx[:, 0] == 0).all()) and (idx[:, -1] == np.asarray(shape) - 1).all()
    s_true = tr.stats(truth, val.astype(np.longdouble))
    assert (np.abs(tr.stats(t, val) - s_true) <= tr.stats_bar(truth, val, bar)).all()
    # the integer data of the exact check stay exact in float64
    fi, ci, ii, _ = tr.case_data(tag, ranks, shape, N, integer=True)
    ti = tr.gather(fi, ci, ii)
    assert (ti == np.round(ti)).all() and np.max(np.abs(tr.gather(fi, ci, ii, absolute=True))) < 2 ** 50
    dense = np.einsum(ci.astype(np.int64), list(range(len(ranks))), *sum(([f.astype(np.int64), [k, 10 + k]] for k, f in enumerate(fi)), []),
                      [10 + k for k in range(len(ranks))]) if tr.prod(shape) <= 10 ** 6 else None
    if dense is not None:
        assert (ti == dense[tuple(ii)]).all()


@pytest.mark.parametrize("ranks", [(2, 33), (33, 2, 5), (7, 3, 2, 9), (2, 3, 4, 5, 6)], ids=str)
def test_float64_inner_products_are_inside_their_bars(ranks):
    _longdouble_is_wider()
    rng = np.random.default_rng(sum(ranks))
    shape = tuple(s + 3 for s in ranks)
    d = len(ranks)
    fa, ca = [rng.standard_normal((s, n)) for s, n in zip(ranks, shape)], rng.standard_normal(ranks)
    rb = ranks[::-1]
    fb, cb = [rng.standard_normal((s, n)) for s, n in zip(rb, shape)], rng.standard_normal(rb)
    cores = tr.random_tt(rng, shape, (3,) * (d - 1))
    A = [rng.standard_normal((n, 6)) for n in shape]
    ld = np.longdouble
    assert abs(tr.tucker_dot(fa, ca, fb, cb) - tr.tucker_dot(fa, ca, fb, cb, dtype=ld)) <= tr.tucker_dot_bar(fa, ca, fb, cb)
    assert abs(tr.tucker_dot(fa, ca, fa, ca) - tr.tucker_dot(fa, ca, fa, ca, dtype=ld)) <= tr.tucker_dot_bar(fa, ca, fa, ca)
    assert abs(tr.tucker_tt_dot(fa, ca, cores) - tr.tucker_tt_dot(fa, ca, cores, dtype=ld)) <= tr.tucker_tt_dot_bar(fa, ca, cores)
    assert abs(tr.tucker_cp_dot(fa, ca, A) - tr.tucker_cp_dot(fa, ca, A, dtype=ld)) <= tr.tucker_cp_dot_bar(fa, ca, A)
    # the restatements against the dense evaluation
    import tt_sketch_amd as tsa
    a, b, tt, cp = tsa.TuckerTensor(fa, ca), tsa.TuckerTensor(fb, cb), tsa.TensorTrain(cores), tsa.CPTensor(A)
    X = a.to_numpy().ravel()
    for got, other, scale in ((tr.tucker_dot(fa, ca, fb, cb), b, tr.tucker_dot(fa, ca, fb, cb, absolute=True)),
                              (tr.tucker_tt_dot(fa, ca, cores), tt, tr.tucker_tt_dot(fa, ca, cores, absolute=True)),
                              (tr.tucker_cp_dot(fa, ca, A), cp, tr.tucker_cp_dot(fa, ca, A, absolute=True))):
        assert abs(got - float(X @ other.to_numpy().ravel())) <= 1e-12 * float(scale)


@pytest.mark.parametrize("case", tr.load_cases(), ids=lambda c: c["name"])
def test_restatement_and_host_paths_against_reference_runs(case):
    import tt_sketch_amd as tsa
    f, c, fb, cb, cores, cp = case["factors"], case["core"], case["factors_b"], case["core_b"], case["cores"], case["cp"]
    idx, x = case["idx"], case["entries"]
    # the reference forms the dense array mode by mode: its own rounding is of the order of the bar
    t = tr.gather(f, c, idx)
    assert (np.abs(t - case["gather"]) <= 2 * tr.entry_bar(f, c, idx)).all()
    rel = 1e-12
    assert abs(tr.tucker_dot(f, c, f, c) - case["norm"] ** 2) <= rel * float(tr.tucker_dot(f, c, f, c, absolute=True))
    assert abs(tr.tucker_dot(fb, cb, fb, cb) - case["norm_b"] ** 2) <= rel * float(tr.tucker_dot(fb, cb, fb, cb, absolute=True))
    assert abs(tr.tucker_dot(f, c, fb, cb) - case["dot_tucker"]) <= rel * float(tr.tucker_dot(f, c, fb, cb, absolute=True))
    for key in ("dot_tt", "dot_tt_rev"):
        assert abs(tr.tucker_tt_dot(f, c, cores) - case[key]) <= rel * float(tr.tucker_tt_dot(f, c, cores, absolute=True))
    for key in ("dot_cp", "dot_cp_rev"):
        assert abs(tr.tucker_cp_dot(f, c, cp) - case[key]) <= rel * float(tr.tucker_cp_dot(f, c, cp, absolute=True))
    assert abs(float(t @ x) - case["dot_sparse"]) <= rel * float(np.abs(t) @ np.abs(x))
    for key, na, nb, dot in (("error_tt", case["norm_tt"], case["norm"], case["dot_tt"]),
                             ("error_cp", case["norm_cp"], case["norm"], case["dot_cp"]),
                             ("error_tucker", case["norm_b"], case["norm"], case["dot_tucker"]),
                             ("error_self_tt", case["norm"], case["norm_tt"], case["dot_tt"])):
        want = tr.fast_error(na, nb, dot, relative=True)
        assert abs(want - case[key]) <= 1e-12 * want, key
    # the host objects of the package: two host operands keep the reference's dense path and upload nothing
    a, b, tt, cpt = tsa.TuckerTensor(f, c), tsa.TuckerTensor(fb, cb), tsa.TensorTrain(cores), tsa.CPTensor(cp)
    assert not a.resident()
    assert abs(a.norm() - case["norm"]) <= 1e-12 * case["norm"]
    assert abs(a.dot(b) - case["dot_tucker"]) <= rel * float(tr.tucker_dot(f, c, fb, cb, absolute=True))
    assert abs(a.dot(tt) - case["dot_tt"]) <= rel * float(tr.tucker_tt_dot(f, c, cores, absolute=True))
    assert abs(cpt.dot(a) - case["dot_cp_rev"]) <= rel * float(tr.tucker_cp_dot(f, c, cp, absolute=True))
    assert abs(tt.error(a, fast=True, relative=True) - case["error_tt"]) <= 1e-9 * case["error_tt"]
    assert abs(a.error(tt, fast=True, relative=True) - case["error_self_tt"]) <= 1e-9 * case["error_self_tt"]
    sp = tsa.SparseTensor(case["shape"], idx, x)
    assert abs(sp.dot(a) - case["dot_sparse"]) <= rel * float(np.abs(t) @ np.abs(x))
    assert abs(a.dot(sp) - case["dot_sparse"]) <= rel * float(np.abs(t) @ np.abs(x))
    assert a._dev is None and b._dev is None and tt._dev is None and cpt._dev is None and sp._dev is None


@pytest.mark.parametrize("case", tr.CASES[:11], ids=lambda c: c[0])
def test_host_gather_equals_to_numpy(case):
    import tt_sketch_amd as tsa
    tag, ranks, shape, N, _, _ = case
    factors, core, idx, _ = tr.case_data(tag, ranks, shape, N)
    a = tsa.TuckerTensor(factors, core)
    X = a.to_numpy()
    bar = 2 * tr.entry_bar(factors, core, idx)
    for arg in (idx, tuple(idx), list(idx)):
        got = a.gather(arg)
        assert got.shape == (N,) and got.dtype == np.float64
        assert (np.abs(got - X[tuple(idx)]) <= bar).all()
    assert (np.abs(a.T.gather(idx[::-1]) - X[tuple(idx)]) <= bar).all()
    assert a._dev is None
    fi, ci, ii, _ = tr.case_data(tag, ranks, shape, N, integer=True)
    ai = tsa.TuckerTensor(fi, ci)
    assert (ai.gather(ii) == ai.to_numpy()[tuple(ii)]).all()


def test_python_layer_raises_before_the_device(monkeypatch):
    import tt_sketch_amd as tsa
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd import tensor_tucker as tk
    from tt_sketch_amd.device import DevArray

    def closed(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(nat, "call", closed)
    monkeypatch.setattr(DevArray, "from_host", classmethod(closed))
    a = tsa.TuckerTensor.random((4, 5, 6), 2, seed=1)
    sp = tsa.SparseTensor.random((4, 5, 7), 10, seed=2)
    with pytest.raises(ValueError):
        a.gather_dev(sp)
    with pytest.raises(ValueError):
        a.support_error(sp)
    with pytest.raises(ValueError):
        a.gather_dev(np.zeros((2, 5), dtype=np.int64))
    with pytest.raises(ValueError):
        a.gather(np.zeros((2, 5), dtype=np.int64))
    with pytest.raises(IndexError):
        a.gather_dev(np.array([[0, 4], [0, 0], [0, 0]]))
    with pytest.raises(IndexError):
        a.gather_dev((np.array([0]), np.array([-1]), np.array([0])))
    with pytest.raises(ValueError):
        a.gather_dev(np.zeros((3, 5), dtype=np.int64), route="fused")
    other = tsa.TuckerTensor.random((4, 5, 7), 2, seed=3)
    with pytest.raises(ValueError):
        tk.tucker_dot(a, other)
    with pytest.raises(ValueError):
        tk.tucker_tt_dot(a, tsa.TensorTrain.random((4, 5, 7), 2, seed=1))
    with pytest.raises(ValueError):
        tk.tucker_cp_dot(a, tsa.CPTensor.random((4, 5, 7), 2, seed=1))
    with pytest.raises(TypeError):
        tk.tucker_dot(a, tsa.CPTensor.random((4, 5, 6), 2, seed=1))
    with pytest.raises(TypeError):
        tk.tucker_tt_dot(tsa.CPTensor.random((4, 5, 6), 2, seed=1), a)
    assert a._dev is None and sp._dev is None
    assert not hasattr(tk, "_host") and "tensor_tucker" not in tsa.__all__
