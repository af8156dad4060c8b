"""The host side of the sorted-key join of sparse tensors, on the CPU: the plan (csrc/sparse_join_plan.h, plain C++) compiled
with the host compiler and checked before any kernel reads it -- stride, splitter count, step counts, grid and every
refusal; the restated two-level search (tests/sparse_join_ref.py) against np.searchsorted on every case the GPU test runs;
the float64 dot in the stated order inside the derived bound of the long-double truth; the restatement and the host paths
of ``SparseTensor.dot`` / ``gather`` against runs of the reference; the argument checks that come before any device call."""
import os
import subprocess

import numpy as np
import pytest

from tests import sparse_join_ref as sj
from tests.host_driver import ROOT, compile_driver, run_driver

ARG, UNSUPPORTED = -2, -3

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "sparse_join_plan.h"
using namespace ttsk;
// const  |  index <variant> N max_split stride_pad d shape...  |  join <variant> dense N_table Nq max_split n_cu stride_pad d shape...
int main(int argc, char **argv)
{
    if (argc >= 2 && !strcmp(argv[1], "const")) {
        printf("%d %d %d %d %d %d %d %d\n", SJ_MAX_SPLIT, SJ_SPLIT_LIMIT, SJ_THREADS, SJ_QPT, SJ_WG_PER_CU, SJ_BLOCK_SUMS, SJ_CLOSE_SUMS, SJ_MAX_MODES);
        return 0;
    }
    if (argc < 3) return 2;
    const char *variant = argv[2];
    const void *some = (const void *)(uintptr_t)4096;        // addresses that are never read
    const bool index = !strcmp(argv[1], "index");
    int a = 3;
    const int dense = index ? 0 : atoi(argv[a++]);
    const uint64_t N = strtoull(argv[a++], nullptr, 10);
    const uint64_t Nq = index ? 0 : strtoull(argv[a++], nullptr, 10);
    const int max_split = atoi(argv[a++]);
    const int n_cu = index ? 0 : atoi(argv[a++]);
    const long long pad = atoll(argv[a++]);
    const int d = atoi(argv[a++]);
    const int dd = d > 0 ? d : 0;
    if (argc != a + dd) return 2;
    std::vector<int64_t> shape;
    std::vector<int> rows;
    for (int i = 0; i < dd; ++i) { shape.push_back(atoll(argv[a + i])); rows.push_back(dd - 1 - i); }
    const int64_t *pshape = shape.data();
    const int *prow = !strcmp(variant, "rows_reversed") ? rows.data() : nullptr;
    if (!strcmp(variant, "bad_row") && dd) { rows[0] = -1; prow = rows.data(); }
    if (!strcmp(variant, "null_shape")) pshape = nullptr;
    const void *idx = !strcmp(variant, "null_idx") ? nullptr : some, *val = !strcmp(variant, "null_val") ? nullptr : some;
    const void *keys = !strcmp(variant, "null_keys") ? nullptr : some, *vals = !strcmp(variant, "null_vals") ? nullptr : some;
    const void *spl = !strcmp(variant, "null_split") ? nullptr : some;
    const void *out = !strcmp(variant, "null_out") || !strcmp(variant, "null_both") ? nullptr : some;
    const void *dot = !strcmp(variant, "null_dot") || !strcmp(variant, "null_both") ? nullptr : some;
    int rc;
    if (index) {
        SjIndexPlan p;
        rc = sparse_key_index_plan(pshape, d, idx, (int64_t)N + pad, prow, N, val, max_split, keys, vals, spl, &p);
        printf("rc %d\nmsg %s\n", rc, p.msg);
        if (rc) return 0;
        printf("top %d %lld %lld %lld %lld %d\n", p.bits, (long long)p.stride, (long long)p.n_split, (long long)p.km.total, (long long)p.km.row_stride, p.km.d);
        for (int k = 0; k < d; ++k) printf("mode %lld %d\n", (long long)p.km.mult[k], p.km.row[k]);
        return 0;
    }
    SjJoinPlan p;
    rc = sparse_join_plan(dense, keys, vals, spl, N, max_split, pshape, d, idx, (int64_t)Nq + pad, prow, Nq, val, out, dot, n_cu, &p);
    printf("rc %d\nmsg %s\n", rc, p.msg);
    if (rc) return 0;
    printf("top %lld %lld %d %d %u %lld %lld %zu %zu %lld\n", (long long)p.stride, (long long)p.n_split, p.lds_steps, p.seg_steps, p.grid, (long long)p.run,
           (long long)p.depth, p.lds, p.scratch, (long long)p.km.total);
    for (int k = 0; k < d; ++k) printf("mode %lld %d\n", (long long)p.km.mult[k], p.km.row[k]);
    return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "sparse_join_plan", DRIVER)

    def run(*args):
        return run_driver(exe, args).splitlines()
    return run


@pytest.fixture(scope="module")
def consts(driver):
    names = ("max_split", "split_limit", "threads", "qpt", "wg_per_cu", "block_sums", "close_sums", "max_modes")
    return dict(zip(names, (int(x) for x in driver("const")[0].split())))


def _parse(out):
    p = dict(rc=int(out[0].split()[1]), msg=out[1][4:], modes=[])
    for line in out[2:]:
        key, *v = line.split()
        if key == "mode":
            p["modes"].append(tuple(int(x) for x in v))
        else:
            p[key] = [int(x) for x in v]
    return p


def index_plan(driver, shape, N, max_split=0, pad=0, variant="ok", d=None):
    return _parse(driver("index", variant, N, max_split, pad, len(shape) if d is None else d, *shape))


def join_plan(driver, shape, N_table, Nq, max_split=0, n_cu=sj.CHIP_CUS, pad=0, variant="ok", dense=0, d=None):
    return _parse(driver("join", variant, dense, N_table, Nq, max_split, n_cu, pad, len(shape) if d is None else d, *shape))


def test_constants_are_the_restatement_s(consts):
    assert consts["max_split"] in (8192, 16384) and consts["max_split"] <= consts["split_limit"] == 16384
    assert (consts["threads"], consts["wg_per_cu"], consts["block_sums"], consts["close_sums"]) == (sj.THREADS, sj.WG_PER_CU, sj.BLOCK_SUMS,
                                                                                                  sj.CLOSE_SUMS)
    assert consts["qpt"] == sj.QPT >= 2                        # several queries of a thread in flight
    assert consts["split_limit"] * 8 + 64 <= 160 * 1024        # the splitter image and block_total's words fit one workgroup's LDS


def _sizes(ms):
    return sj.table_sizes(ms) + [10 ** 7, 2 ** 31 - 1]


def test_stride_splitters_and_steps_at_every_edge(driver, consts):
    ms = consts["max_split"]
    shape = (2 ** 20, 2 ** 20, 8)
    for cap, arg in ((ms, 0), (16384, 16384), (8192, 8192), (4, 4), (1, 1)):
        for N in _sizes(cap) + _sizes(ms):
            pi, pj = index_plan(driver, shape, N, arg), join_plan(driver, shape, N, 1000, arg)
            assert pi["rc"] == 0 and pj["rc"] == 0, (N, cap, pi["msg"], pj["msg"])
            bits, stride, n_split, total, row_stride, d = pi["top"]
            want = sj.layout(N, 1000, cap)
            assert (stride, n_split) == (want["stride"], want["n_split"]) == tuple(pj["top"][:2]), (N, cap)
            assert pj["top"][2:4] == [want["lds_steps"], want["seg_steps"]]
            # what the kernel relies on: the splitters fit, they cover the table, the last segment is not empty
            assert n_split <= cap and stride >= 1
            if N:
                assert (n_split - 1) * stride < N <= n_split * stride
                assert stride == -(-N // cap)
                assert 2 ** pj["top"][2] >= n_split > (2 ** pj["top"][2]) // 2 and 2 ** pj["top"][3] >= stride > (2 ** pj["top"][3]) // 2
            else:
                assert (stride, n_split) == (1, 0)
            assert pj["top"][7] == 8 * n_split
            assert (bits, total, row_stride, d) == (43, 2 ** 43, N, 3)
    ragged = 12 * ms + 7
    assert ragged % sj.split(ragged, ms)[0] != 0                # the large size of the cases has a ragged last segment


def test_grid_run_and_depth(driver):
    for n_cu in (1, 3, 256, 0):
        cap = sj.WG_PER_CU * max(n_cu, 1)
        for Nq in (0, 1, 255, 256, 257, 256 * cap - 1, 256 * cap, 256 * cap + 1, 10 ** 7 + 3):
            p = join_plan(driver, (5, 6), 100, Nq, 0, n_cu)
            assert p["rc"] == 0
            stride, n_split, lds_steps, seg_steps, grid, run, depth, lds, scratch, total = p["top"]
            want = sj.layout(100, Nq, 8192, n_cu)
            assert (grid, run, depth) == (want["grid"], want["run"], want["depth"])
            assert grid == min(-(-Nq // 256), cap) and scratch == 8 * grid
            assert grid * run >= Nq and (grid == 0 or grid * (run - 1) < Nq)     # the runs cover the list, none is longer than needed
            assert depth == -(-run // 256) + sj.BLOCK_SUMS + -(-grid // 256) + sj.CLOSE_SUMS
    # the dense pass: no splitters, no LDS
    p = join_plan(driver, (5, 6), 0, 1000, dense=1)
    assert p["rc"] == 0 and p["top"][:4] == [1, 0, 0, 0] and p["top"][7] == 0


def test_key_map_and_sort_bits(driver):
    for shape in [(7,), (1,), (3, 4, 5), (1, 300, 1, 1, 200), sj.BIG_SHAPE, (2,) * 32, (2 ** 62, 1, 1), (2 ** 63 - 1,)]:
        m, total = sj.mults(shape)
        for variant in ("ok", "rows_reversed"):
            p = index_plan(driver, shape, 10, variant=variant, pad=3)
            assert p["rc"] == 0, p["msg"]
            rows = list(range(len(shape)))[::-1] if variant == "rows_reversed" else list(range(len(shape)))
            assert p["modes"] == list(zip(m, rows))
            assert p["top"][0] == sj.sort_bits(shape) and p["top"][3] == total and p["top"][4] == 13
            assert total - 1 < 2 ** p["top"][0] and (p["top"][0] == 1 or total - 1 >= 2 ** (p["top"][0] - 1))
            assert join_plan(driver, shape, 10, 10, variant=variant)["modes"] == p["modes"]


def test_every_refusal(driver, consts):
    shape = (4, 5, 6)
    for variant in ("null_shape", "null_idx", "null_val", "null_keys", "null_vals", "null_split"):
        p = index_plan(driver, shape, 10, variant=variant)
        assert p["rc"] == ARG and "NULL" in p["msg"], variant
    for variant in ("null_shape", "null_idx", "null_val", "null_keys", "null_vals", "null_split", "null_both"):
        p = join_plan(driver, shape, 10, 10, variant=variant)
        assert p["rc"] == ARG and any(w in p["msg"] for w in ("NULL", "dev_qval", "neither")), variant
    assert join_plan(driver, shape, 10, 10, variant="null_out")["rc"] == 0
    assert join_plan(driver, shape, 10, 10, variant="null_dot")["rc"] == 0
    p = join_plan(driver, shape, 10, 10, dense=1, variant="null_keys")
    assert p["rc"] == ARG and "ttsk_dense_join" in p["msg"]
    # an empty table or list needs no arrays
    assert index_plan(driver, shape, 0, variant="null_idx")["rc"] == 0 and index_plan(driver, shape, 0, variant="null_keys")["rc"] == 0
    assert join_plan(driver, shape, 0, 10, variant="null_keys")["rc"] == 0 and join_plan(driver, shape, 10, 0, variant="null_idx")["rc"] == 0
    for plan in (lambda **k: index_plan(driver, k.pop("shape", shape), 10, **k), lambda **k: join_plan(driver, k.pop("shape", shape), 10, 10, **k)):
        assert plan(shape=(), d=0)["rc"] == ARG and plan(shape=(), d=-1)["rc"] == ARG
        assert plan(shape=(4, 0, 6))["rc"] == ARG and plan(shape=(4, -5, 6))["rc"] == ARG
        p = plan(pad=-1)
        assert p["rc"] == ARG and "row_stride" in p["msg"]
        assert plan(pad=-11)["rc"] == ARG                       # a negative stride
        assert plan(variant="bad_row")["rc"] == ARG
        assert plan(max_split=-1)["rc"] == ARG and plan(max_split=consts["split_limit"] + 1)["rc"] == ARG
        assert plan(max_split=consts["split_limit"])["rc"] == 0
        # ---- the cover
        assert plan(shape=(2,) * 32)["rc"] == 0
        p = plan(shape=(2,) * 33)
        assert p["rc"] == UNSUPPORTED and "33 modes" in p["msg"]
        assert plan(shape=(2 ** 63 - 1,))["rc"] == 0 and plan(shape=(2 ** 31, 2 ** 31 - 1, 2))["rc"] == 0
        assert plan(shape=(2 ** 63 - 1, 1))["rc"] == 0
        for big in ((2 ** 31, 2 ** 31, 2), (2 ** 62, 2), (3, 2 ** 62), (2 ** 40, 2 ** 40)):        # 2^63 and beyond
            p = plan(shape=big)
            assert p["rc"] == UNSUPPORTED and "2^63" in p["msg"], big
    big_n = 2 ** 31
    assert index_plan(driver, shape, big_n - 1)["rc"] == 0 and join_plan(driver, shape, big_n - 1, 10)["rc"] == 0
    for p in (index_plan(driver, shape, big_n), join_plan(driver, shape, big_n, 10), index_plan(driver, shape, big_n, variant="null_idx")):
        assert p["rc"] == UNSUPPORTED and "2^31" in p["msg"]
    assert join_plan(driver, shape, 10, 2 ** 33)["rc"] == 0       # the list of queries has no such limit


def _cases(ms):
    return [sj.make_case(spec) for spec in sj.case_list(ms)]


def test_restated_search_against_searchsorted_and_dict(consts):
    ms = consts["max_split"]
    names = set()
    for case in _cases(ms):
        shape = case["shape"]
        for cap in (ms, 16384 if ms == 8192 else 8192):
            index = sj.build_index(case["tidx"], case["tval"], shape, cap)
            ks = index["keys"]
            assert (np.diff(ks) >= 0).all() and len(index["splitters"]) == sj.split(len(ks), cap)[1]
            if cap != ms:
                continue
            qidx, qval = sj.case_queries(case, index)
            q = sj.keys_of(qidx, shape)
            assert len(q) == case["Nq"] and (sj.unravel(q, shape) == qidx).all()
            assert (qidx >= 0).all() and (qidx < np.array(shape, dtype=np.int64)[:, None]).all()
            got = sj.join(index, q)
            # the reference's semantics, independently: a dict filled in storage order (the last entry wins), every query looked up
            table = {}
            for k, v in zip(sj.keys_of(case["tidx"], shape).tolist(), case["tval"].tolist()):
                table[k] = v
            assert np.array_equal(got, np.array([table.get(k, 0.0) for k in q.tolist()])), case["name"]
            if len(ks):
                ub = np.searchsorted(ks, q, side="right")
                pos = sj.search(index, q)
                assert np.array_equal(pos, np.maximum(ub - 1, 0)), case["name"]
                hit = ks[pos] == q
                if case["kind"] != "near_top" and len(q) > 100:
                    assert hit.any() and not hit.all()
                if case["kind"] in ("run", "all_equal") and len(q) > 100:
                    rep = ks[1]
                    assert (q == rep).any() and index["stride"] >= 2
                    last = np.nonzero(sj.keys_of(case["tidx"], shape) == rep)[0][-1]
                    assert (got[q == rep] == case["tval"][last]).all()
        names.add(case["name"])
    assert set(sj.SIZE_NAMES) | {"big_shape", "nq_beyond_grid"} <= names


def test_cases_reach_their_edges(consts):
    ms = consts["max_split"]
    specs = sj.case_list(ms)
    assert {0, 1, 255, 256, 257} <= {s[4] for s in specs}
    assert any(sj.layout(s[2], s[4], ms)["run"] > sj.THREADS * sj.QPT and sj.layout(s[2], s[4], ms)["grid"] == sj.WG_PER_CU * sj.CHIP_CUS for s in specs)
    assert {1, 3, 5} <= {len(s[1]) for s in specs}
    big = sj.make_case(next(s for s in specs if s[0] == "big_shape"))
    k = sj.keys_of(big["tidx"], big["shape"])
    assert sj.sort_bits(big["shape"]) == 63 and (k >= 2 ** 62 - 10 ** 6).all() and (k >= 2 ** 62).any() and k.max() >= sj.mults(big["shape"])[1] - 10 ** 6
    assert (big["tidx"][0] >= 2 ** 30 - 1).all() and (sj.unravel(k, big["shape"]) == big["tidx"]).all()
    run = sj.make_case(next(s for s in specs if s[0] == "run_over_splitters"))
    index = sj.build_index(run["tidx"], run["tval"], run["shape"], ms)
    assert index["stride"] == 3 and (index["keys"][1:8] == index["keys"][1]).all() and index["keys"][8] != index["keys"][1]
    assert (index["splitters"][1:3] == index["keys"][1]).all()           # the run holds two splitters


def test_float64_dot_in_the_stated_order_is_inside_the_bound():
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("np.longdouble is no wider than float64 on this host: the bound cannot be checked")
    rng = np.random.default_rng(5)
    for Nq in (0, 1, 255, 256, 257, 1000, 70001, sj.WG_PER_CU * sj.CHIP_CUS * sj.THREADS + 300, 10 ** 6 + 1):
        for n_cu in (1, 256):
            qv, tv = rng.standard_normal(Nq), rng.standard_normal(Nq) * (rng.random(Nq) < 0.6)
            got = sj.dot_ordered(qv, tv, n_cu)
            truth, abs_sum = sj.dot_truth(qv, tv)
            tol = sj.bound(sj.layout(0, Nq, 1, n_cu)["depth"], abs_sum)
            assert abs(got - truth) <= tol, (Nq, n_cu, float(abs(got - truth)), tol)
    assert sj.dot_ordered(np.ones(5), np.arange(5.0)) == 10.0


@pytest.mark.parametrize("case", sj.load_cases(), ids=lambda c: c["name"])
def test_restatement_and_host_paths_against_reference_runs(case, consts):
    import tt_sketch_amd as tsa
    shape = case["shape"]
    ia, va, ib, vb, X = case["idx_a"], case["val_a"], case["idx_b"], case["val_b"], case["dense"]
    tol = lambda *terms: 1e-12 * float(np.sum(np.abs(np.multiply(*terms)))) + 1e-300
    for cap in (consts["max_split"], 64, 7):                    # small caps: several segments even on these small tables
        b_index, a_index = sj.build_index(ib, vb, shape, cap), sj.build_index(ia, va, shape, cap)
        at_a, at_b = sj.join(b_index, sj.keys_of(ia, shape)), sj.join(a_index, sj.keys_of(ib, shape))
        assert abs(sj.dot_ordered(va, at_a) - case["dot_ab"]) <= tol(va, at_a)
        assert abs(sj.dot_ordered(vb, at_b) - case["dot_ba"]) <= tol(vb, at_b)
        assert np.array_equal(sj.join(b_index, sj.keys_of(case["gather_idx"], shape)), case["gather_b"])
        # the .T views: reversed rows in the reversed shape
        bT = sj.build_index(ib[::-1], vb, shape[::-1], cap)
        at_aT = sj.join(bT, sj.keys_of(ia[::-1], shape[::-1]))
        assert abs(sj.dot_ordered(va, at_aT) - case["dot_abT"]) <= tol(va, at_aT)
    # against a dense tensor the reference densifies `a` (of a repeated index the last entry stays); the join counts every
    # nonzero, as the gathers of the other formats do: the two agree where `a` repeats no index
    at_dense = X.ravel()[sj.keys_of(ia, shape)]
    assert np.array_equal(at_dense, X.T.ravel()[sj.keys_of(ia[::-1], shape[::-1])])
    if case["dup_a"] == 0:
        for name in ("dot_a_dense", "dot_dense_a", "dot_aT_denseT"):
            assert abs(sj.dot_ordered(va, at_dense) - case[name]) <= tol(va, at_dense), name
    # the host objects of the package keep the reference's paths, and upload nothing
    a, b, dense = tsa.SparseTensor(shape, ia, va), tsa.SparseTensor(shape, ib, vb), tsa.DenseTensor(X)
    assert abs(a.dot(b) - case["dot_ab"]) <= tol(va, at_a) and abs(b.dot(a) - case["dot_ba"]) <= tol(vb, at_b)
    assert abs(a.T.dot(b.T) - case["dot_abT"]) <= tol(va, at_a)
    assert np.array_equal(b.gather(tuple(case["gather_idx"])), case["gather_b"])
    assert abs(a.dot(dense) - case["dot_a_dense"]) <= 1e-12 * float(np.sum(np.abs(X)) * np.abs(va).max())
    assert abs(dense.dot(a) - case["dot_dense_a"]) <= 1e-12 * float(np.sum(np.abs(X)) * np.abs(va).max())
    assert a._dev is None and b._dev is None and dense._dev is None


def test_fixture_holds_every_kind_of_case():
    cases = {c["name"]: c for c in sj.load_cases()}
    dup = lambda idx, shape: len(np.unique(sj.keys_of(idx, shape))) < idx.shape[1]
    kinds = {(dup(c["idx_a"], c["shape"]), dup(c["idx_b"], c["shape"])) for c in cases.values()}
    assert kinds == {(False, False), (True, False), (False, True), (True, True)}
    assert all(100 <= c["idx_a"].shape[1] <= 400 and 100 <= c["idx_b"].shape[1] <= 400 for c in cases.values())
    assert any(c["dot_ab"] != c["dot_ba"] for c in cases.values())          # duplicates: the orientation matters
    assert any(c["dot_ab"] == 0.0 for c in cases.values()) and {1, 2, 3, 4, 5} <= {len(c["shape"]) for c in cases.values()}


def test_module_is_importable_first_and_has_no_host_copy():
    import sys
    code = ("import tt_sketch_amd.tensor_sparse as m, tt_sketch_amd.tensor as t; "
            "assert not hasattr(m, '_host'); assert m.SparseTensor is t.SparseTensor; "
            "assert hasattr(t.SparseTensor, 'gather_dev')")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
    src = open(os.path.join(ROOT, "tt_sketch_amd", "tensor_sparse.py")).read()
    assert "_host" not in src and ".to_numpy(" not in src and ".dict" not in src


def test_arguments_are_checked_before_the_device(monkeypatch):
    import tt_sketch_amd as tsa
    from tt_sketch_amd import _native as nat, tensor_sparse as ts
    from tt_sketch_amd.device import DevArray

    def closed(*a, **k):
        raise AssertionError("a device call before the arguments were checked")
    monkeypatch.setattr(nat, "call", closed)
    rng = np.random.default_rng(0)
    shape = (4, 5, 6)
    idx = np.stack([rng.integers(0, n, 20) for n in shape])
    a, b = tsa.SparseTensor(shape, idx, rng.standard_normal(20)), tsa.SparseTensor((4, 5, 7), idx, rng.standard_normal(20))
    dense = tsa.DenseTensor(rng.standard_normal((4, 5, 7)))
    fake = (object(), object(), {})                             # "uploaded": the device branch is taken, nothing is touched
    monkeypatch.setattr(a, "_dev", fake)
    from tt_sketch_amd import paths
    with paths.forced("kernel"):                               # the device route whatever the size: its checks are the ones meant
        with pytest.raises(ValueError):
            a.dot(b)                                                # shapes differ
        with pytest.raises(ValueError):
            a.dot(dense)
        with pytest.raises(ValueError):
            a.gather_dev(b)
        with pytest.raises(ValueError):
            a.gather(idx[:2])                                       # two index rows for three modes
        bad = idx.copy()
        bad[1, 3] = 5
        with pytest.raises(IndexError):
            a.gather(bad)                                           # outside the shape
        bad[1, 3] = -1
        with pytest.raises(IndexError):
            a.gather_dev(tuple(bad))
        with pytest.raises(TypeError):
            ts._dense_join(tsa.DenseTensor(np.zeros(shape, dtype=np.float32)), idx, True, False)
    assert "gather_dev" not in tsa.__all__ and not [n for n in tsa.__all__ if "join" in n.lower()]
    assert DevArray is not None


def test_route_rule_and_switch(monkeypatch):
    """The rule of tensor_sparse is arithmetic on the sizes and on what is cached already; ``route`` / ``paths.forced``
    override it, ``"composed"`` being the host path."""
    import tt_sketch_amd as tsa
    from tt_sketch_amd import _native as nat, paths, tensor_sparse as ts

    def closed(*a, **k):
        raise AssertionError("device")
    monkeypatch.setattr(nat, "call", closed)
    rng = np.random.default_rng(1)
    shape = (30, 40)
    flat = rng.choice(1200, 60, replace=False)
    mk = lambda f: tsa.SparseTensor(shape, np.stack(np.unravel_index(f, shape)), rng.standard_normal(len(f)))
    a, b = mk(flat[:40]), mk(flat[20:])
    want = mk(flat[:1]).__class__(shape, a.indices, a.entries).dot(tsa.SparseTensor(shape, b.indices, b.entries))     # two host tensors: the host path
    monkeypatch.setattr(a, "_dev", (object(), object(), {}))    # "uploaded": the device branch is open
    monkeypatch.setattr(b, "_dev", (object(), object(), {}))
    kernel, host = ts._join_route_ms(b, a.nnz)
    assert kernel == ts._JOIN_CALL_MS + ts._JOIN_INDEX_MS and host == ts._HOST_QUERY_MS * 40 + ts._HOST_TABLE_MS * 40
    assert host < kernel and not ts._join_routed(b, a.nnz, None)
    b._dev[2][("key_index", b.dev_row_order)] = (None, None, None)
    assert ts._join_route_ms(b, a.nnz)[0] == ts._JOIN_CALL_MS
    assert ("key_index", b.T.dev_row_order) not in b._dev[2] and ts._join_route_ms(b.T, a.nnz)[0] == kernel
    b._dev[2].clear()
    a.dot(b)                                                    # small: the rule keeps the host path, which caches the dict
    assert ts._join_route_ms(b, a.nnz)[1] == ts._HOST_QUERY_MS * 40
    big = tsa.SparseTensor((1000, 1000), np.zeros((2, 10 ** 6), dtype=np.int64), np.zeros(10 ** 6))
    monkeypatch.setattr(big, "_dev", (object(), object(), {}))
    assert ts._join_routed(big, 10 ** 6, None) and ts._join_routed(big, 10, None)
    assert not ts._join_routed(big, 10 ** 6, "composed") and ts._join_routed(b, 1, "kernel")
    with paths.forced("composed"):
        assert not ts._join_routed(big, 10 ** 6, None) and ts._join_routed(big, 10 ** 6, "kernel")
    with paths.forced("kernel"):
        assert ts._join_routed(b, 1, None)
        with pytest.raises(AssertionError, match="device"):
            a.dot(b)
    assert a.dot(b, route="composed") == a.dot(b) == want
    assert np.array_equal(b.gather(a.indices, route="composed"), b.gather(a.indices))
    with pytest.raises(AssertionError, match="device"):
        b.gather(a.indices, route="kernel")
    with pytest.raises(ValueError):
        a.dot(b, route="bogus")
