"""The host-side plan of the Gram pass of tensor trains (csrc/tt_gram_plan.h, plain C++): a few lines of driver compiled
with the host compiler print what ttsk_tt_gram (csrc/tt_gram.hip) launches its kernels with, and that is checked here --
before any kernel reads it.  Also held here: the chunk rule tests/tt_gram_ref.py restates, and that float64 NumPy stays
inside the derived bound of that module against np.longdouble (so the bound can be relied on in the GPU test)."""

import numpy as np
import pytest

from tests import tt_gram_ref as gr
from tests.host_driver import compile_driver, run_driver

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "tt_gram_plan.h"
using namespace ttsk;
int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const int d = atoi(argv[1]), K = atoi(argv[2]), M = atoi(argv[3]), n_cu = atoi(argv[4]);
    if (d < 0 || K < 0 || M < 0 || argc != 5 + d + (K + M) * (d + 1)) return 2;
    std::vector<int64_t> shape, ra, rb;
    char **v = argv + 5;
    for (int i = 0; i < d; ++i) shape.push_back(atoll(*v++));
    for (int i = 0; i < K * (d + 1); ++i) ra.push_back(atoll(*v++));
    for (int i = 0; i < M * (d + 1); ++i) rb.push_back(atoll(*v++));
    GramPlan p;
    const int rc = gram_plan(ra.data(), rb.data(), shape.data(), d, K, M, n_cu, &p);
    printf("rc %d\nmsg %s\n", rc, p.msg);
    if (rc) return 0;
    printf("top %d %d %zu %lld\n", p.launches, p.fold_last, p.scratch, (long long)p.pairs);
    printf("const %zu %d %d %d %d %d\n", GRAM_LDS_BUDGET, GRAM_MAX_RANK, GRAM_MAX_CHUNKS, GRAM_MAX_STAGE_TILES, GRAM_FMA_CELLS, GRAM_MAX_TRAINS);
    for (int k = 0; k < d; ++k) {
        const GramModePlan &m = p.m[k];
        printf("mode %d %d %d %d %d %d %d %zu %zu %zu %zu %zu %d %d %d %d %lld %lld\n", m.chunks, m.body, m.S, m.TA, m.pitch, m.acc_rows, m.t_rows,
               m.acc_doubles, m.t_doubles, m.lds, m.slab_off, m.slab_bytes, m.ra, m.rb, m.ra1, m.rb1, (long long)m.sum_a1, (long long)m.sum_b1);
    }
    return 0;
}
"""

MODE_KEYS = ("chunks", "body", "S", "TA", "pitch", "acc_rows", "t_rows", "acc_doubles", "t_doubles", "lds", "slab_off", "slab_bytes",
             "ra", "rb", "ra1", "rb1", "sum_a1", "sum_b1")


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "tt_gram_plan", DRIVER)

    def run(shape, ranks_a, ranks_b, n_cu):
        """ranks_*: full rank rows (d + 1 numbers) of each train"""
        args = [len(shape), len(ranks_a), len(ranks_b), n_cu, *shape, *[r for row in ranks_a for r in row], *[r for row in ranks_b for r in row]]
        out = run_driver(exe, args).splitlines()
        p = dict(rc=int(out[0].split()[1]), msg=out[1][4:], modes=[])
        for line in out[2:]:
            key, *v = line.split()
            if key == "mode":
                p["modes"].append(dict(zip(MODE_KEYS, (int(x) for x in v))))
            else:
                p[key] = [int(x) for x in v]
        return p
    return run


def full(ranks):
    return [(1,) + tuple(r) + (1,) for r in ranks]


def check_plan(p, shape, ra, rb, n_cu):
    d, K, M = len(shape), len(ra), len(rb)
    assert p["rc"] == 0, p["msg"]
    launches, fold, scratch, pairs = p["top"]
    budget, max_rank, max_chunks, stage_tiles, fma_cells, _ = p["const"]
    assert pairs == K * M and len(p["modes"]) == d
    assert launches == d + 1 - fold and launches <= d + 1
    assert fold == (p["modes"][-1]["chunks"] == 1)
    assert [m["chunks"] for m in p["modes"]] == gr.chunks(shape, K * M, n_cu)          # the rule tests/tt_gram_ref.py restates
    assert (max_rank, max_chunks) == (gr.MAX_RANK, gr.MAX_CHUNKS)
    for k, m in enumerate(p["modes"]):
        n = shape[k]
        assert 1 <= m["chunks"] <= n
        assert (m["ra"], m["ra1"]) == (max(r[k] for r in ra), max(r[k + 1] for r in ra))
        assert (m["rb"], m["rb1"]) == (max(r[k] for r in rb), max(r[k + 1] for r in rb))
        assert (m["sum_a1"], m["sum_b1"]) == (sum(r[k + 1] for r in ra), sum(r[k + 1] for r in rb))
        # ---- LDS: acc, then T, inside the budget; what the kernels index stays inside each region
        assert m["lds"] == 8 * (m["acc_doubles"] + m["t_doubles"]) <= budget
        assert m["acc_doubles"] == m["acc_rows"] * m["pitch"]
        assert 1 <= m["S"] <= -(-n // m["chunks"])
        if m["body"] == 1:
            assert m["ra1"] >= 16 and max(m["rb"], m["rb1"]) >= 16
            assert 1 <= m["TA"] and m["S"] * m["TA"] <= stage_tiles
            assert m["acc_rows"] == -(-m["ra"] // 4) * 4 and m["t_rows"] == -(-m["rb"] // 16) * 16 and m["pitch"] >= m["t_rows"]
            assert m["t_doubles"] == m["S"] * m["TA"] * m["t_rows"] * 16
        else:
            assert m["ra1"] < 16 or max(m["rb"], m["rb1"]) < 16
            assert m["ra1"] * m["rb1"] <= fma_cells                                    # eight sums per thread
            assert m["acc_rows"] == m["ra"] and m["pitch"] == m["rb"] and m["t_doubles"] == m["S"] * m["rb"] * m["ra1"]
        # ---- slab: every (pair, chunk) block inside it, blocks of different pairs disjoint
        assert m["slab_bytes"] == 8 * m["chunks"] * m["sum_a1"] * m["sum_b1"]
        assert m["slab_off"] % 8 == 0 and m["slab_off"] + m["slab_bytes"] <= scratch
        blocks, pre_a = [], 0
        for a in ra:
            pre_b = 0
            for b in rb:
                lo = m["chunks"] * (pre_a * m["sum_b1"] + a[k + 1] * pre_b)             # the kernel's offset of the pair
                blocks.append((lo, lo + m["chunks"] * a[k + 1] * b[k + 1]))
                pre_b += b[k + 1]
            pre_a += a[k + 1]
        blocks.sort()
        assert blocks[0][0] == 0 and 8 * blocks[-1][1] <= m["slab_bytes"]
        assert all(e0 <= b1 for (_, e0), (b1, _) in zip(blocks, blocks[1:]))
    # the slabs of consecutive modes are live together: disjoint
    for m0, m1 in zip(p["modes"], p["modes"][1:]):
        assert m0["slab_off"] + m0["slab_bytes"] <= m1["slab_off"] or m1["slab_off"] + m1["slab_bytes"] <= m0["slab_off"]
    if fold:
        assert K * M * 8 == p["modes"][-1]["slab_bytes"]                               # the last slab IS G


@pytest.mark.parametrize("n_cu", [1, 256])
@pytest.mark.parametrize("case", gr.CASES, ids=lambda c: c.name)
def test_plan_of_every_gpu_case(plan, case, n_cu):
    ra = full(case.ranks_a)
    rb = ra if case.ranks_b is None else full(case.ranks_b)
    check_plan(plan(case.shape, ra, rb, n_cu), case.shape, ra, rb, n_cu)


@pytest.mark.parametrize("n_cu", [1, 256])
@pytest.mark.parametrize("KM", [(1, 1), (3, 2), (16, 16)], ids=lambda km: f"KM{km[0] * km[1]}")
def test_plan_over_batch_sizes(plan, KM, n_cu):
    K, M = KM
    for shape, r in (((200,) * 6, (50, 100)), ((20,) * 8, (20, 20)), ((3, 1, 40), (128, 128)), ((5,) * 32, (7, 9))):
        d = len(shape)
        ra = [(1,) + (max(1, r[0] - p),) * (d - 1) + (1,) for p in range(K)]
        rb = [(1,) + (max(1, r[1] - q),) * (d - 1) + (1,) for q in range(M)]
        check_plan(plan(shape, ra, rb, n_cu), shape, ra, rb, n_cu)


def test_widest_acc_fits_without_its_padding(plan):
    p = plan((4, 4, 4), [(1, 128, 128, 1)], [(1, 128, 128, 1)], 256)
    assert p["rc"] == 0
    m = p["modes"][1]
    assert (m["body"], m["S"], m["TA"], m["pitch"]) == (1, 1, 1, 128) and m["lds"] == 8 * (128 * 128 + 128 * 16)
    m = plan((4, 4, 4), [(1, 50, 50, 1)], [(1, 100, 100, 1)], 256)["modes"][1]
    assert m["pitch"] % 32 == 16 and m["TA"] == 4                                      # room for the conflict-free pitch


def test_cover_and_argument_errors(plan):
    ok = [(1, 128, 1)]
    assert plan((3, 3), ok, ok, 256)["rc"] == 0
    for ra, rb in (([(1, 129, 1)], ok), (ok, [(1, 129, 1)])):
        p = plan((3, 3), ra, rb, 256)
        assert p["rc"] == -3 and "rank 129" in p["msg"]
    assert plan((3, 2 ** 31), ok, ok, 256)["rc"] == -3
    assert plan((3, 2 ** 31 - 1), ok, ok, 256)["rc"] == 0
    assert plan((2,) * 33, [(1,) * 34], [(1,) * 34], 256)["rc"] == -3
    assert plan((2,) * 32, [(1,) * 33], [(1,) * 33], 256)["rc"] == 0
    assert plan((2, 2), ok * 64, ok * 64, 256)["rc"] == 0 and plan((2, 2), ok * 65, ok * 64, 256)["rc"] == -3
    for ra, rb, shape in (([(2, 3, 1)], ok, (3, 3)), (ok, [(1, 3, 2)], (3, 3)), ([(1, 0, 1)], ok, (3, 3)), (ok, ok, (3, 0))):
        assert plan(shape, ra, rb, 256)["rc"] == -2
    assert plan((3, 3), [], ok, 256)["rc"] == -2 and plan((3, 3), ok, [], 256)["rc"] == -2 and plan((), [(1,)], [(1,)], 256)["rc"] == -2


@pytest.mark.parametrize("case", gr.CASES, ids=lambda c: c.name)
def test_float64_chain_is_inside_the_bound_of_longdouble(case):
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("np.longdouble is no wider than float64 on this host: the bound cannot be checked")
    A, B = gr.case_cores(case)
    G, ref = gr.gram(A, B), gr.gram(A, B, dtype=np.longdouble)
    for n_cu in (1, 256):
        tol = gr.bound(A, B, n_cu)
        assert (np.abs(G - ref) <= tol).all(), (case.name, np.max(np.abs(G - ref) / tol))
    assert (gr.gram(A, B, absolute=True) >= np.abs(G)).all()
