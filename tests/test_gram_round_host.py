"""Gram-SVD rounding on the CPU: the NumPy restatement of DESIGN section 18 (tests/gram_round_ref.py) against
``TensorTrain.round`` and against the dense truths of a bond, with the figures the GPU test takes its tolerances from; the
plan of ttsk_gram_round_bonds (csrc/gram_round_plan.h, plain C++) compiled with the host compiler and driven over the edges
of the working set; and what ``method="gram"`` does before it reaches a device."""
import typing

import numpy as np
import pytest

from tests import gram_round_ref as gr
from tests.host_driver import ROOT, compile_driver, run_driver

ARG, UNSUPPORTED = -2, -3


# ---------------------------------------------------------------- the restatement
def _round_both(case):
    import tt_sketch_amd as tsa
    from tt_sketch_amd.utils import process_tt_rank
    cores = gr.random_tt(case.shape, case.ranks, case.seed)
    x = tsa.TensorTrain(cores)
    a = x.round(max_rank=case.max_rank)
    caps = process_tt_rank(x.rank if case.max_rank is None else case.max_rank, x.shape, trim=True)
    g = tsa.TensorTrain(gr.round_gram(cores, 0.0, caps)[0])
    return x, a, g


@pytest.mark.parametrize("case", gr.ROUND_CASES, ids=lambda c: c.name)
def test_restatement_against_round(case):
    """ranks equal; where `round` truncates, the error against the input is within ERROR_RATIO_CAP of its error"""
    x, a, g = _round_both(case)
    assert g.rank == a.rank
    ea, eg = a.error(x, relative=True), g.error(x, relative=True)
    print(f"{case.name}: round {ea:.6e} gram {eg:.6e} ratio {eg / max(ea, 1e-300):.5f}")
    if ea > 1e-8:
        assert eg <= gr.ERROR_RATIO_CAP * ea
    else:
        assert eg <= 1e-12


def test_restatement_recovers_an_untruncated_train():
    x, a, g = _round_both(gr.EXACT_CASE)
    assert g.rank == a.rank == gr.EXACT_CASE.ranks
    assert g.error(x, relative=True) <= 1e-12


def test_restatement_on_rank_deficient_sums():
    import tt_sketch_amd as tsa
    xs = gr.random_tt((10, 12, 11, 9), (6, 7, 5), 31)
    ys = gr.random_tt((10, 12, 11, 9), (3, 4, 2), 32)
    X = gr.dense(xs)
    # x + x at eps = 1e-6: the ranks of x
    g, _ = gr.round_gram(gr.add(xs, xs), 1e-6)
    assert tuple(c.shape[0] for c in g[1:]) == (6, 7, 5) and gr.rel_error(gr.dense(g), 2 * X) <= 1e-12
    # a zero summand: exact zero eigenvalues
    g, _ = gr.round_gram(gr.add(xs, gr.scale(ys, 0.0)), 1e-6)
    assert tuple(c.shape[0] for c in g[1:]) == (6, 7, 5) and gr.rel_error(gr.dense(g), X) <= 1e-12
    # a small summand below eps: dropped, at an error of its size
    s = gr.add(xs, gr.scale(ys, 1e-5))
    g, _ = gr.round_gram(s, 1e-3)
    small = np.linalg.norm(gr.dense(ys)) * 1e-5 / np.linalg.norm(X)
    assert tuple(c.shape[0] for c in g[1:]) == (6, 7, 5) and gr.rel_error(gr.dense(g), gr.dense(s)) <= 2 * small
    assert tsa.TensorTrain(s).round(eps=1e-3).rank == (6, 7, 5)


@pytest.mark.parametrize("case", gr.BOND_CASES, ids=lambda c: c.name)
def test_restatement_of_a_bond_is_inside_its_recorded_deviation(case):
    """The deviations recorded beside each case are what this restatement shows here, to a factor of two for another BLAS;
    tests/test_gpu_gram_round.py allows the kernel 16 times the recorded figure."""
    cores = gr.case_cores(case)
    GL, GR = gr.grams(cores)
    worst = [0.0, 0.0, 0.0]
    for b, r in enumerate(case.ranks):
        A, B = gr.parts(cores, b + 1)
        assert A.shape[1] == B.shape[1] == r and A.shape[0] * B.shape[0] <= 10 ** 5
        np.testing.assert_allclose(A.T @ A, GL[b], rtol=0, atol=1e-13 * np.abs(GL[b]).max())
        np.testing.assert_allclose(B.T @ B, GR[b], rtol=0, atol=1e-13 * np.abs(GR[b]).max())
        P, Q, S, rho = gr.bond_solve(GL[b], GR[b], case.eps, case.caps[b])
        assert rho == gr.expected_rank(A, B, case.eps, case.caps[b])
        worst = [max(w, v) for w, v in zip(worst, gr.bond_deviation(A, B, P, Q, S, rho))]
    print(case.name, " ".join(f"{w:.2e}" for w in worst))
    for w, rec in zip(worst, case.dev):
        assert w <= 2.0 * rec


def test_bond_cases_reach_their_edges():
    ranks = {r for c in gr.BOND_CASES for r in c.ranks}
    assert {1, 2, 16, 17, 100, 101, 142, 143, 300} <= ranks
    assert any(len(c.ranks) == 1 for c in gr.BOND_CASES) and any(len(set(c.ranks)) > 2 for c in gr.BOND_CASES)
    assert any(cap < r for c in gr.BOND_CASES for cap, r in zip(c.caps, c.ranks)) and any(c.eps > 0 for c in gr.BOND_CASES)


# ---------------------------------------------------------------- the plan header
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "gram_round_plan.h"
using namespace ttsk;
// plan <variant> eps rank cap [rank cap ...]
int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const char *variant = argv[1];
    const double eps = atof(argv[2]);
    std::vector<int64_t> ranks, caps;
    for (int i = 3; i + 1 < argc; i += 2) { ranks.push_back(atoll(argv[i])); caps.push_back(atoll(argv[i + 1])); }
    int count = (int)ranks.size();
    // addresses that are never read
    std::vector<const double *> gl, gr;
    std::vector<double *> pt, q, sg;
    for (int b = 0; b < count; ++b) {
        gl.push_back((const double *)(uintptr_t)(4096 * (5 * b + 1)));
        gr.push_back((const double *)(uintptr_t)(4096 * (5 * b + 2)));
        pt.push_back((double *)(uintptr_t)(4096 * (5 * b + 3)));
        q.push_back((double *)(uintptr_t)(4096 * (5 * b + 4)));
        sg.push_back((double *)(uintptr_t)(4096 * (5 * b + 5)));
    }
    int *rank_out = (int *)(uintptr_t)8;
    const double *const *pgl = gl.data(), *const *pgr = gr.data();
    double *const *ppt = pt.data(), *const *pq = q.data(), *const *psg = sg.data();
    const int64_t *pranks = ranks.data(), *pcaps = caps.data();
    if (!strcmp(variant, "null_gl")) pgl = nullptr;
    if (!strcmp(variant, "null_gr")) pgr = nullptr;
    if (!strcmp(variant, "null_ranks")) pranks = nullptr;
    if (!strcmp(variant, "null_caps")) pcaps = nullptr;
    if (!strcmp(variant, "null_pt")) ppt = nullptr;
    if (!strcmp(variant, "null_q")) pq = nullptr;
    if (!strcmp(variant, "null_sigma")) psg = nullptr;
    if (!strcmp(variant, "null_rank_out")) rank_out = nullptr;
    if (!strcmp(variant, "null_one_gl")) gl[count - 1] = nullptr;
    if (!strcmp(variant, "null_one_q")) q[0] = nullptr;
    if (!strcmp(variant, "count0")) count = 0;
    static GramRoundPlan p;
    const int rc = gram_round_plan(pgl, pgr, pranks, pcaps, count, eps, ppt, pq, psg, rank_out, &p);
    printf("rc %d\nmsg %s\n", rc, p.msg);
    if (rc) return 0;
    printf("top %u %u %zu %zu %d %.17g\n", p.grid_eig, p.grid_bond, p.lds, p.scratch, p.a.count, p.a.eps);
    printf("const %d %d %d %zu %zu\n", GRB_MAX_BONDS, GRB_MAX_RANK, GRB_THREADS, GRB_LDS_CAP, sizeof(GramRoundArgs));
    for (int b = 0; b < count; ++b) {
        const GrbBond &B = p.a.b[b];
        size_t bytes = 0;
        const int place = grb_place(B.r, &bytes);
        const GrbLayout L = grb_layout(B.r, place);
        printf("bond %d %d %d %d %zu %lld %d\n", B.r, B.cap, p.place[b], place, bytes, (long long)B.ws,
               B.gl == gl[b] && B.gr == gr[b] && B.pt == pt[b] && B.q == q[b] && B.sigma == sg[b]);
        printf("layout %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)L.v_l, (long long)L.v_r, (long long)L.lam_l,
               (long long)L.lam_r, (long long)L.ord_l, (long long)L.ord_r, (long long)L.kept, (long long)L.qa, (long long)L.u, (long long)L.w_l, (long long)L.w_r,
               (long long)L.total);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "gram_round_plan", DRIVER)

    def run(bonds, eps=0.0, variant="ok"):
        args = [variant, repr(float(eps))] + [str(v) for rc in bonds for v in rc]
        out = run_driver(exe, args).splitlines()
        p = dict(rc=int(out[0].split()[1]), msg=out[1][4:], bonds=[], layouts=[])
        for line in out[2:]:
            key, *v = line.split()
            vals = [float(x) if "." in x or "e" in x else int(x) for x in v]
            if key == "bond":
                p["bonds"].append(vals)
            elif key == "layout":
                p["layouts"].append(vals)
            else:
                p[key] = vals
        return p
    return run


LDS_CAP = 160 * 1024 - 256


def _place(r):
    """the rule of jacobi.hip for a square working set: (place, dynamic LDS bytes)"""
    small, mat = (r + (r + 1) // 2) * 8, r * r * 8
    if small + 2 * mat <= LDS_CAP:
        return 2, small + 2 * mat
    if small + mat <= LDS_CAP:
        return 1, small + mat
    return 0, small


EDGE_RANKS = (1, 100, 101, 142, 143, 1024)


def test_place_edges_are_those_of_the_jacobi_kernel():
    assert [_place(r)[0] for r in EDGE_RANKS] == [2, 2, 1, 1, 0, 0]


def _check_layout(r, place, layout):
    v_l, v_r, lam_l, lam_r, ord_l, ord_r, kept, qa, u, w_l, w_r, total = layout
    mat, ints = r * r, (r + 1) // 2
    pieces = [(v_l, mat), (v_r, mat), (lam_l, r), (lam_r, r), (ord_l, ints), (ord_r, ints), (kept, 1), (qa, mat)]
    assert (u >= 0) == (place < 2) and (w_l >= 0) == (w_r >= 0) == (place < 1)
    pieces += [(x, mat) for x in (u, w_l, w_r) if x >= 0]
    pieces.sort()
    assert pieces[0][0] == 0
    for (a, n), (b, _) in zip(pieces, pieces[1:]):
        assert a + n <= b                                   # no two pieces overlap
    assert pieces[-1][0] + pieces[-1][1] == total             # and the slice ends with the last


@pytest.mark.parametrize("r", EDGE_RANKS)
def test_plan_of_one_bond_at_every_edge(plan, r):
    p = plan([(r, r)])
    assert p["rc"] == 0, p["msg"]
    place, lds = _place(r)
    grid_eig, grid_bond, p_lds, scratch, count, eps = p["top"]
    assert (grid_eig, grid_bond, count, p_lds) == (2, 1, 1, lds) and lds <= LDS_CAP
    (br, cap, p_place, k_place, k_bytes, ws, same), = p["bonds"]
    assert (br, cap, p_place, k_place, k_bytes, ws, same) == (r, r, place, place, lds, 0, 1)    # host and kernel agree on the place
    _check_layout(r, place, p["layouts"][0])
    assert scratch == 8 * p["layouts"][0][-1]
    max_bonds, max_rank, threads, lds_cap, arg_bytes = p["const"]
    assert (max_bonds, max_rank, threads, lds_cap) == (64, 1024, 1024, LDS_CAP) and arg_bytes <= 4096


def test_plan_of_mixed_bonds(plan):
    bonds = [(r, c) for r, c in zip(EDGE_RANKS, (1, 50, 200, 142, 7, 1024))]
    p = plan(bonds, eps=1e-6)
    assert p["rc"] == 0, p["msg"]
    grid_eig, grid_bond, lds, scratch, count, eps = p["top"]
    assert (grid_eig, grid_bond, count, eps) == (12, 6, 6, 1e-6)
    assert lds == max(_place(r)[1] for r in EDGE_RANKS)      # one launch: the largest need
    at = 0
    for (r, c), bond, layout in zip(bonds, p["bonds"], p["layouts"]):
        assert bond[:4] == [r, min(c, r), _place(r)[0], _place(r)[0]] and bond[5:] == [at, 1]      # a cap above the rank is the rank
        _check_layout(r, _place(r)[0], layout)
        at += layout[-1]                                     # the slices lie one after another
    assert scratch == 8 * at


def test_plan_refusals(plan):
    ok = [(5, 3), (7, 7)]
    assert plan(ok)["rc"] == 0
    for variant in ("null_gl", "null_gr", "null_ranks", "null_caps", "null_pt", "null_q", "null_sigma", "null_rank_out", "null_one_gl",
                    "null_one_q"):
        p = plan(ok, variant=variant)
        assert p["rc"] == ARG and "NULL" in p["msg"], variant
    assert plan(ok, variant="count0")["rc"] == ARG
    for bad in ([(0, 1)], [(5, 0)], [(-3, 2)], [(5, 3), (4, -1)]):
        assert plan(bad)["rc"] == ARG, bad
    for eps in (-1e-3, float("nan"), float("inf")):
        assert plan(ok, eps=eps)["rc"] == ARG, eps
    # ---- the cover
    assert plan([(1024, 1024)])["rc"] == 0
    p = plan([(5, 3), (1025, 10)])
    assert p["rc"] == UNSUPPORTED and "1025" in p["msg"]
    assert plan([(3, 3)] * 64)["rc"] == 0
    p = plan([(3, 3)] * 65)
    assert p["rc"] == UNSUPPORTED and "65 bonds" in p["msg"]
    # a refusal of the arguments comes before one of the cover
    assert plan([(1025, 10), (0, 1)])["rc"] == ARG


# ---------------------------------------------------------------- method="gram" before the device
class _Reached(Exception):
    pass


def test_gram_rounding_forms_lazy_terms_first(monkeypatch):
    """raised before any device call: this test has no device"""
    import tt_sketch_amd as tsa
    from tt_sketch_amd import HadamardProduct, hadamard_round, tt_gmres
    x = tsa.TensorTrain(gr.random_tt((4, 5, 4), (2, 3), 1))
    y = tsa.TensorTrain(gr.random_tt((4, 5, 4), (3, 2), 2))
    formed = []

    def to_tt(self):
        formed.append((self.x, self.y))
        raise _Reached("to_tt")
    monkeypatch.setattr(HadamardProduct, "to_tt", to_tt)
    with pytest.raises(_Reached):
        tt_gmres.round_tt_sum(x + x.hadamard(y), 4, method="gram")
    assert formed == [(x, y)]
    with pytest.raises(_Reached):
        hadamard_round(x, y, 4, method="gram")
    assert len(formed) == 2


def test_gram_is_a_rounding_mode_that_lazy_products_refuse():
    from tt_sketch_amd import tt_gmres
    assert "gram" in typing.get_args(tt_gmres.ROUNDING_MODE)
    assert typing.get_args(tt_gmres.ROUNDING_MODE)[:2] == ("exact", "pairwise")
    with pytest.raises(ValueError, match="lazy_products"):
        tt_gmres.tt_sum_gmres(None, None, 4, rounding_method="gram", lazy_products=True)


def test_round_gram_is_reached_from_inside_the_methods_only():
    import subprocess as sp
    import sys
    code = ("import sys, tt_sketch_amd.tensor as t; assert 'tt_sketch_amd.tensor_round' not in sys.modules; "
            "import tt_sketch_amd.tensor_round as r; assert r.TensorTrain is t.TensorTrain and not hasattr(r, '_host'); "
            "assert callable(t.TensorTrain.round_gram) and callable(t.TensorTrain.svdvals_gram)")
    run = sp.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    fresh = sp.run([sys.executable, "-c", "import tt_sketch_amd.tensor_round"], cwd=ROOT, capture_output=True, text=True)
    assert fresh.returncode == 0, fresh.stderr


def test_round_gram_checks_its_arguments_before_the_device():
    import tt_sketch_amd as tsa
    x = tsa.TensorTrain(gr.random_tt((4, 5, 4), (2, 3), 1))
    with pytest.raises(ValueError, match="eps"):
        x.round_gram(eps=-1.0)
    big = tsa.TensorTrain([np.zeros((1, 2, 1025)), np.zeros((1025, 2, 1))])
    with pytest.raises(ValueError, match="1024"):
        big.round_gram()
    assert x._dev is None and big._dev is None
