"""Inner products of Hadamard products that are never formed, without a GPU: the NumPy restatement of
``ttsk_hadamard_close`` (tests/hadamard_close_ref.py) against the explicit Kronecker core and against np.longdouble, the two
halves of a mode against the chain through the explicit cores, ``HadamardProduct.dot`` / ``norm`` / ``error(fast=True)`` on
host cores with ``to_tt`` and ``to_numpy`` forbidden, and the host-side plan of the entry (csrc/hadamard_close_plan.h, plain
C++) compiled with the host compiler."""

import numpy as np
import pytest

from tests import hadamard_close_ref as ref
from tests import hadamard_ref
from tests.host_driver import compile_driver, run_driver

ERR_ARG, UNSUPPORTED = -2, -3


# ---- 1. the restatement
@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.name)
def test_restatement_against_the_explicit_product_and_longdouble(case):
    Wl, U, V, out0 = ref.case_arrays(case)
    G, tol = ref.close_term(Wl, U, V, out0), ref.bound(Wl, U, V, out0)
    assert G.shape == (case.P, case.S1 * case.s1) and ref.depth(Wl, U, V) == case.s + case.S + case.n + 3
    through = ref.close_from_product(Wl, U, V) + (0.0 if out0 is None else out0)
    assert (np.abs(G - through) <= tol).all()
    exact = ref.close_term(Wl, U, V, out0, dtype=np.longdouble)
    ratio = float(np.max(np.abs(G - exact) / (tol / 2)))          # against the undoubled, first-order bound
    print(f"{case.name}: float64 against longdouble at {ratio:.2f} of the first-order bound")
    assert ratio <= 1.0
    for a, layout in ((U, case.u_layout), (V, case.v_layout)):
        assert a.flags.c_contiguous == (layout == "c") or a.size == max(a.shape)
    assert (out0 is not None) == bool(case.accumulate)
    assert max(a.nbytes for a in (Wl, U, V, G)) < 2 ** 20          # the largest operand is below a megabyte


def test_cases_reach_every_edge():
    """the case list is what the plan's constants make of it: every edge extent occurs"""
    for field in ("s", "s1", "P"):
        assert set(ref.EDGES_SMALL) <= {getattr(c, field) for c in ref.CASES}, field
    assert set(ref.EDGES_S) <= {c.S for c in ref.CASES} and set(ref.EDGES_S1) <= {c.S1 for c in ref.CASES}
    assert set(ref.EDGES_N) <= {c.n for c in ref.CASES}
    assert any(c.n % ref.layout(*c[1:7])[0] for c in ref.CASES)                   # a ragged last chunk of i
    assert any(ref.layout(*c[1:7])[1] > 1 for c in ref.CASES) and any(ref.layout(*c[1:7])[0] > 1 for c in ref.CASES)
    assert {c.u_layout for c in ref.CASES} | {c.v_layout for c in ref.CASES} == set(hadamard_ref.LAYOUTS)
    assert {c.accumulate for c in ref.CASES} == {0, 1}
    assert any(c.P == 1 and c.S1 > hadamard_ref.COLS_PER_WORKGROUP and c.S > hadamard_ref.BETA_CHUNK for c in ref.CASES)
    assert any(c.S != c.S1 and c.s != c.s1 for c in ref.CASES)
    assert len({c.name for c in ref.CASES}) == len(ref.CASES) and 10 <= len(ref.CASES) <= 14


# ---- 2. half A followed by half B is one step of the chain through the explicit cores
@pytest.mark.parametrize("dims", [(2, 3, 3, 2, 4, 2, 2, 5, 3), (1, 4, 1, 3, 5, 1, 2, 1, 6)], ids=["inner", "first"])
def test_two_halves_equal_the_chain_through_the_kronecker_cores(dims):
    R, R1, r, r1, n, S, S1, s, s1 = dims
    rng = np.random.default_rng(7)
    G = rng.standard_normal((R, r, S, s))
    X, Y = rng.standard_normal((R, n, R1)), rng.standard_normal((r, n, r1))
    U, V = rng.standard_normal((S, n, S1)), rng.standard_normal((s, n, s1))
    W = hadamard_ref.w_term(G.reshape(R, r, S * s), X, Y)                         # half A, l = S s
    assert W.shape == (S * s, n, R1 * r1)
    got = ref.close_term(W, U, V).reshape(R1, r1, S1, s1)                         # half B
    Pk = np.einsum("bik,aic->baikc", X, Y).reshape(R * r, n, R1 * r1)
    Qk = np.einsum("gih,cid->gcihd", U, V).reshape(S * s, n, S1 * s1)
    want = np.einsum("pq,pik,qil->kl", G.reshape(R * r, S * s), Pk, Qk).reshape(R1, r1, S1, s1)
    assert np.allclose(got, want, rtol=1e-13, atol=1e-13 * np.abs(want).max())


# ---- 3. HadamardProduct on host cores: nothing formed
SHAPE = (3, 4, 2, 5)


def _train(rng, rank):
    from tt_sketch_amd import TensorTrain
    rank = (1,) + tuple(rank) + (1,)
    return TensorTrain([rng.standard_normal((rank[k], SHAPE[k], rank[k + 1])) for k in range(len(SHAPE))])


@pytest.fixture()
def host_products(monkeypatch):
    """two host products and a host train with their dense tensors; after the dense tensors are taken, forming a product
    raises"""
    from tt_sketch_amd import HadamardProduct
    rng = np.random.default_rng(21)
    x, y, u, v, z = (_train(rng, rk) for rk in ((2, 3, 2), (3, 2, 4), (4, 2, 3), (2, 5, 2), (3, 6, 4)))
    dense = dict(h=x.to_numpy() * y.to_numpy(), q=u.to_numpy() * v.to_numpy(), z=z.to_numpy())

    def formed(self):
        raise AssertionError("the product was formed")
    monkeypatch.setattr(HadamardProduct, "to_tt", formed)
    monkeypatch.setattr(HadamardProduct, "to_numpy", formed)
    return HadamardProduct(x, y), HadamardProduct(u, v), z, dense


def test_host_dot_norm_and_fast_error_form_nothing(host_products, monkeypatch):
    from tt_sketch_amd import TensorSum, _native as nat
    h, q, z, dense = host_products
    monkeypatch.setattr(nat, "call", lambda *a: pytest.fail(f"the device was touched: {a[0]}"))
    scale = lambda a, b: 1e-12 * np.linalg.norm(dense[a]) * np.linalg.norm(dense[b])      # noqa: E731
    assert abs(h.dot(z) - np.vdot(dense["h"], dense["z"])) <= scale("h", "z")
    assert abs(z.dot(h) - np.vdot(dense["h"], dense["z"])) <= scale("h", "z")             # from the train's side
    assert abs(h.dot(q) - np.vdot(dense["h"], dense["q"])) <= scale("h", "q")
    assert abs(q.dot(h) - h.dot(q)) <= scale("h", "q")
    assert abs(h.norm() - np.linalg.norm(dense["h"])) <= 1e-12 * np.linalg.norm(dense["h"])
    assert abs((h @ q) - h.dot(q)) == 0.0
    both = TensorSum([z, q])
    assert abs(h.dot(both) - np.vdot(dense["h"], dense["z"] + dense["q"])) <= scale("h", "z") + scale("h", "q")
    # the fast formula against the dense difference; the pairs are far apart, so its floor of 1e-8 does not show
    for a, b, da, db in ((h, q, "h", "q"), (h, z, "h", "z"), (z, h, "z", "h")):
        want = np.linalg.norm(dense[da] - dense[db])
        assert want / np.linalg.norm(dense[db]) >= 0.1
        assert abs(a.error(b, fast=True) - want) <= 1e-10 * want
        assert abs(a.error(b, fast=True, relative=True) - want / np.linalg.norm(dense[db])) <= 1e-10
        assert abs(a.error(b, fast=True, rmse=True) - want / np.sqrt(dense[da].size)) <= 1e-10 * want
    assert h.error(h, fast=True, relative=True) < 1e-7
    idx = np.array([[0, 2, 1], [3, 0, 2], [1, 1, 0], [4, 2, 0]])
    assert np.allclose(h.gather(idx), dense["h"][tuple(idx)], rtol=1e-13, atol=0)


def test_host_dot_checks_shapes_and_keeps_other_partners(host_products):
    from tt_sketch_amd import DenseTensor, HadamardProduct, TensorTrain
    h, q, z, dense = host_products
    other = TensorTrain([np.ones((1, n, 1)) for n in SHAPE[:-1] + (7,)])
    with pytest.raises(ValueError, match="shapes"):
        h.dot(other)
    with pytest.raises(ValueError, match="shapes"):
        h.dot(HadamardProduct(other, other))
    with pytest.raises(ValueError, match="route"):
        h.dot(q, route="fastest")
    with pytest.raises(AssertionError, match="formed"):           # a dense partner still goes through the base class
        h.dot(DenseTensor(dense["z"]))


def test_route_rule_and_budget_are_stated():
    from tt_sketch_amd import hadamard_gram as hg
    kernel, composed = hg.close_route_ms(20, 20, 20, 20, 20, 400)
    assert kernel > 0 and composed > 0
    assert hg._slices(10, hg.W_BUDGET_BYTES // 8) == [(i, i + 1) for i in range(10)]          # a row fills the budget: one i each
    assert hg._slices(10, hg.W_BUDGET_BYTES // 32) == [(0, 4), (4, 8), (8, 10)]               # three slices, the last ragged
    assert hg._slices(7, 1) == [(0, 7)] and hg._slices(3, hg.W_BUDGET_BYTES) == [(0, 1), (1, 2), (2, 3)]
    assert "hadamard_gram" not in __import__("tt_sketch_amd").__all__


# ---- 4. the host-side plan
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "hadamard_close_plan.h"
using namespace ttsk;
int main(int argc, char **argv)
{
    if (argc != 10) return 2;
    static double cell;
    int64_t dims[6], strides[6] = {1, 1, 1, 1, 1, 1};
    for (int i = 0; i < 6; ++i) dims[i] = atoll(argv[1 + i]);
    const int accumulate = atoi(argv[7]);
    const long long work_doubles = atoll(argv[8]);
    const int null = atoi(argv[9]);            // bits: Wl, U, V, dims, strides, out, work
    static HadamardClosePlan p, q;
    const int rc = hadamard_close_plan(null & 1 ? nullptr : &cell, null & 2 ? nullptr : &cell, null & 4 ? nullptr : &cell,
                                       null & 8 ? nullptr : dims, null & 16 ? nullptr : strides, null & 32 ? nullptr : &cell,
                                       accumulate, null & 64 ? nullptr : &cell, work_doubles, &p);
    printf("rc %d\nmsg %s\n", rc, p.msg);
    printf("const %lld %d %d %d %zu %zu %lld %lld %d\n", (long long)HC_FILL, HD_KC, HD_COLS, HD_PITCH, HD_LDS, sizeof(HadamardCloseArgs),
           (long long)HC_TAIL_NUM, (long long)HC_TAIL_DEN, HC_TRIES);
    const int lrc = hadamard_close_layout(null & 8 ? nullptr : dims, &q);
    printf("layout %d %d %d %lld %lld\n", lrc, q.a.ichunks, q.a.iper, (long long)q.slab, (long long)q.blocks);
    if (rc) return 0;
    printf("top %lld %.17g %d %d %d %d %d %lld\n", (long long)p.blocks, p.flops, p.a.ptiles, p.a.ctiles, p.a.gblocks, p.a.ichunks, p.a.iper,
           (long long)p.slab);
    printf("args %d %d %d %d %d %d\n", p.a.S, p.a.S1, p.a.s, p.a.s1, p.a.n, p.a.P);
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "hadamard_close_plan", DRIVER)

    def run(dims, accumulate=0, work=2 ** 62, null=0):
        """dims: (S, S', s, s', n, P)"""
        args = list(dims) + [accumulate, work, null]
        out = run_driver(exe, args).splitlines()
        p = dict(rc=int(out[0].split()[1]), msg=out[1][4:])
        for line in out[2:]:
            key, *v = line.split()
            p[key] = [float(x) if "." in x or "e" in x else int(x) for x in v]
        return p
    return run


def test_plan_constants_and_grid_arithmetic(plan):
    fill, kc, cols, pitch, lds, arg_bytes, tail_num, tail_den, tries = plan((1, 1, 1, 1, 1, 1))["const"]
    assert (fill, (tail_num, tail_den), tries) == (ref.FILL, ref.TAIL, ref.TRIES)
    assert (cols, kc) == (hadamard_ref.COLS_PER_WORKGROUP, hadamard_ref.BETA_CHUNK)
    assert lds == kc * pitch * 8 and 2 * lds <= 160 * 1024       # the stage of hadamard_apply: two workgroups per compute unit
    assert arg_bytes <= 4096
    # ranks 32 x 32 against 32 x 32, n = 200: 64 x 2 tiles, cut into four ranges of 50
    p = plan((32, 32, 32, 32, 200, 1024))
    assert p["rc"] == 0 and p["top"][:1] + p["top"][2:] == [512, 64, 2, 1, 4, 50, 4 * 1024 * 1024]
    # one tile: every i a workgroup of its own
    p = plan((4, 4, 4, 4, 200, 16))
    assert p["top"][5:7] == [200, 1] and p["top"][0] == 200
    # 157 x 4 tiles, a second round of 512 that is 23% full: cut until the last round is nine tenths full
    p = plan((50, 50, 50, 50, 42, 2500))
    ichunks, iper, slab, blocks = ref.layout(50, 50, 50, 50, 42, 2500)
    assert (blocks, ichunks, iper) == (628 * 3, 3, 14) and p["top"][0] == blocks and p["top"][5:] == [ichunks, iper, slab]
    # tiles enough: the mode is not cut
    p = plan((4, 300, 5, 40, 7, 2000))
    assert p["top"][2:7] == [125, 3, 5, 1, 7] and p["top"][0] == 125 * 3 * 5 and p["top"][7] == 2000 * 300 * 40


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.name)
def test_plan_covers_every_case(plan, case):
    dims = tuple(case[1:7])
    ichunks, iper, slab, blocks = ref.layout(*dims)
    p = plan(dims, case.accumulate, slab)
    assert p["rc"] == 0, p["msg"]
    assert p["top"][2:5] == [-(-case.P // 16), -(-case.s1 // 16), -(-case.S1 // hadamard_ref.COLS_PER_WORKGROUP)]
    assert p["top"][0] == blocks and p["top"][5:] == [ichunks, iper, slab]
    assert (ichunks - 1) * iper < case.n <= ichunks * iper          # every chunk has an i, every i a chunk
    assert p["top"][1] == 2.0 * case.n * case.P * (case.S * case.s * case.s1 + case.S * case.S1 * case.s1)
    assert p["args"] == list(dims)
    assert p["layout"] == [0, ichunks, iper, slab, blocks]          # ttsk_hadamard_close_layout is the same arithmetic
    short = plan(dims, case.accumulate, slab - 1)
    assert short["rc"] == ERR_ARG and "slab" in short["msg"]


def test_plan_argument_errors_and_refusals(plan):
    ok = (2, 3, 4, 5, 6, 8)
    assert plan(ok)["rc"] == 0 and plan(ok, 1)["rc"] == 0
    for bit in range(7):
        p = plan(ok, null=1 << bit)
        assert p["rc"] == ERR_ARG and "NULL" in p["msg"], bit
    assert plan(ok, null=8)["layout"][0] == ERR_ARG
    names = ["S", "S'", "s", "s'", "n", "P"]
    for i in range(6):
        for value in (0, -3):
            bad = list(ok)
            bad[i] = value
            p = plan(bad)
            assert p["rc"] == ERR_ARG and f"{names[i]} = {value}" in p["msg"] and p["layout"][0] == ERR_ARG, i
    for accumulate in (-1, 2):
        p = plan(ok, accumulate)
        assert p["rc"] == ERR_ARG and "accumulate" in p["msg"]
    assert plan(ok, work=0)["rc"] == ERR_ARG and plan(ok, work=-1)["rc"] == ERR_ARG
    # the cover: extents and the number of workgroups below 2^31 (the slab is then below 2^45 doubles)
    big = 2 ** 31
    for i in range(6):
        wide = list(ok)
        wide[i] = big
        p = plan(wide)
        assert p["rc"] == UNSUPPORTED and "2^31" in p["msg"] and p["layout"][0] == UNSUPPORTED, i
    assert plan((2, 3, 4, 5, 6, big - 1))["rc"] == 0                     # the largest P: 2^27 tiles, the mode not cut
    assert plan((2, 3, 4, 5, big - 1, 8))["rc"] == 0                     # the longest mode: 512 chunks
    p = plan((2, 2 ** 26, 4, 2 ** 20, 6, 2 ** 16))                       # 2^12 x 2^16 x 2^20 tiles
    assert p["rc"] == UNSUPPORTED and "workgroups" in p["msg"]
    p = plan((2, 2 ** 30, 4, 16, 6, 2 ** 30))                            # 2^26 x 2^24 workgroups' worth
    assert p["rc"] == UNSUPPORTED
    p = plan((2, 64, 4, 2 ** 30, 6, 2 ** 30))                            # 2^26 x 2^26 tiles
    assert p["rc"] == UNSUPPORTED
    p = plan((2, big - 1, 4, 16, 6, 16))                                 # 2^25 blocks of gamma', a slab of 2^39 doubles
    assert p["rc"] == 0 and p["top"][7] == (big - 1) * 16 * 16
    p = plan((2, big - 1, 4, big - 1, 6, 1))                             # 2^62 columns: 2^27 x 2^25 tiles
    assert p["rc"] == UNSUPPORTED and "workgroups" in p["msg"]
