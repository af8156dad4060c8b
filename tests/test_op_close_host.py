"""Inner products of operator-times-train products that are never formed, without a GPU: the NumPy restatement of
``ttsk_op_close`` (tests/op_close_ref.py) against the explicit product core and against np.longdouble, the two halves of a
mode against the chain through the explicit cores, ``OperatorProduct.dot`` / ``norm`` / ``error(fast=True)`` and
``TTLinearMapSum.residual`` on host cores with ``to_tt`` and ``to_numpy`` forbidden, and the host-side plan of the entry
(csrc/op_close_plan.h, plain C++) compiled with the host compiler."""
import os

import numpy as np
import pytest

from tests import hadamard_close_ref, hadamard_ref
from tests import op_apply_ref
from tests import op_close_ref as ref
from tests.host_driver import ROOT, compile_driver, run_driver

ERR_ARG, UNSUPPORTED = -2, -3


# ---- 1. the restatement
@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.name)
def test_restatement_against_the_explicit_product_and_longdouble(case):
    Wl, N, Y, out0 = ref.case_arrays(case)
    G, tol = ref.close_term(Wl, N, Y, out0), ref.bound(Wl, N, Y, out0)
    assert G.shape == (case.P, case.s1 * case.S1) and ref.depth(Wl, N, Y) == case.S * case.n_out + case.s + case.n_in + 3
    through = ref.close_from_product(Wl, N, Y) + (0.0 if out0 is None else out0)
    assert (np.abs(G - through) <= tol).all()
    exact = ref.close_term(Wl, N, Y, out0, dtype=np.longdouble)
    ratio = float(np.max(np.abs(G - exact) / (tol / 2)))          # against the undoubled, first-order bound
    print(f"{case.name}: float64 against longdouble at {ratio:.2f} of the first-order bound")
    assert ratio <= 1.0
    assert ref.one_run(N) and N.shape == (case.S, case.n_in, case.n_out, case.S1)
    assert Y.flags.c_contiguous == (case.y_layout == "c") or Y.size == max(Y.shape)
    assert (out0 is not None) == bool(case.accumulate)
    assert max(a.nbytes for a in (Wl, N, Y, G)) < 2 ** 20          # the largest operand is below a megabyte


def test_cases_reach_every_edge():
    """the case list is what the plan's constants make of it: every edge extent occurs"""
    for field in ("S1", "s1", "P"):
        assert set(ref.EDGES_TILE) <= {getattr(c, field) for c in ref.CASES}, field
    assert any(c.s1 > hadamard_ref.COLS_PER_WORKGROUP for c in ref.CASES)
    assert set(ref.EDGES_S) <= {c.s for c in ref.CASES}
    assert set(ref.EDGES_K) <= {c.S * c.n_out for c in ref.CASES}
    assert any(c.n_in != c.n_out and c.n_in > 1 and c.n_out > 1 for c in ref.CASES) and any(c.n_in == 1 for c in ref.CASES)
    layouts = {c.name: ref.layout(*ref.dims(c)) for c in ref.CASES}
    assert any(c.n_in % layouts[c.name][0] for c in ref.CASES)                     # a ragged last chunk of j
    assert any(v[1] > 1 for v in layouts.values()) and any(v[0] > 1 for v in layouts.values())
    assert {c.y_layout for c in ref.CASES} == set(hadamard_ref.LAYOUTS) and {c.n_layout for c in ref.CASES} == set(ref.N_LAYOUTS)
    assert {c.accumulate for c in ref.CASES} == {0, 1}
    assert len({c.name for c in ref.CASES}) == len(ref.CASES) and 10 <= len(ref.CASES) <= 14
    assert (ref.FILL, ref.TAIL, ref.TRIES) == (hadamard_close_ref.FILL, hadamard_close_ref.TAIL, hadamard_close_ref.TRIES)


def test_a_stored_operator_core_is_not_one_run_and_its_transpose_is():
    rng = np.random.default_rng(0)
    N = rng.standard_normal((3, 4, 5, 2))                          # (S, n_in, n_out, S') as an MPO stores it
    assert not ref.one_run(N)
    packed = np.ascontiguousarray(N.transpose(0, 2, 1, 3)).transpose(0, 2, 1, 3)      # the core of mpo.T, viewed back
    assert ref.one_run(packed) and np.array_equal(packed, N)
    assert ref.one_run(N[:1]) and ref.one_run(N[:, :, :1])         # an extent of 1 leaves one stride


# ---- 2. half A followed by half B is one step of the chain through the explicit cores
@pytest.mark.parametrize("dims", [(2, 3, 3, 2, 4, 5, 2, 2, 5, 3, 3), (1, 4, 1, 3, 5, 2, 1, 2, 1, 6, 4)], ids=["inner", "first"])
def test_two_halves_equal_the_chain_through_the_product_cores(dims):
    R, R1, r, r1, m_in, n_out, S, S1, s, s1, n_in = dims
    rng = np.random.default_rng(7)
    G = rng.standard_normal((R, r, s, S))
    M, C = rng.standard_normal((R, m_in, n_out, R1)), rng.standard_normal((r, m_in, r1))
    N, Y = rng.standard_normal((S, n_in, n_out, S1)), rng.standard_normal((s, n_in, s1))
    W = op_apply_ref.w_term(G.reshape(R, r, s * S), M, C)                          # half A, l = s S
    assert W.shape == (s * S, n_out, R1 * r1)
    got = ref.close_term(W, N, Y).reshape(R1, r1, s1, S1)                          # half B
    Pk = np.einsum("ijkl,ajb->iaklb", M, C).reshape(R * r, n_out, R1 * r1)
    Qk = np.einsum("ijkl,ajb->iaklb", N, Y).reshape(S, s, n_out, S1, s1)
    want = np.einsum("pcg,pik,gcihd->kdh", G.reshape(R * r, s, S), Pk, Qk).reshape(R1, r1, s1, S1)
    assert np.allclose(got, want, rtol=1e-13, atol=1e-13 * np.abs(want).max())


# ---- 3. OperatorProduct on host cores: nothing formed
OUT_SHAPE = (3, 4, 2, 5)
IN_X = (2, 4, 3, 5)              # the mode sizes of x and of y differ; only the out shapes agree
IN_Y = (4, 3, 2, 2)


def _train(rng, shape, rank):
    from tt_sketch_amd import TensorTrain
    rank = (1,) + tuple(rank) + (1,)
    return TensorTrain([rng.standard_normal((rank[k], shape[k], rank[k + 1])) for k in range(len(shape))])


def _mpo(rng, in_shape, rank):
    from tt_sketch_amd.tt_gmres import MPO
    rank = (1,) + tuple(rank) + (1,)
    return MPO([rng.standard_normal((rank[k], in_shape[k], OUT_SHAPE[k], rank[k + 1])) for k in range(len(OUT_SHAPE))])


def _dense_apply(mpo, tt):
    """mpo(tt) as a dense array, from the dense operator (in_0, out_0, ...) and the dense train"""
    A, x = mpo.to_numpy(), tt.to_numpy()
    d = x.ndim
    return np.tensordot(A, x, axes=(list(range(0, 2 * d, 2)), list(range(d))))


@pytest.fixture()
def host_products(monkeypatch):
    """two host products and a host train with their dense tensors; after the dense tensors are taken, forming a product
    raises"""
    from tt_sketch_amd import OperatorProduct
    rng = np.random.default_rng(21)
    M, N = _mpo(rng, IN_X, (2, 3, 2)), _mpo(rng, IN_Y, (3, 2, 2))
    x, y, z = _train(rng, IN_X, (2, 3, 2)), _train(rng, IN_Y, (4, 2, 3)), _train(rng, OUT_SHAPE, (3, 5, 4))
    dense = dict(h=_dense_apply(M, x), q=_dense_apply(N, y), z=z.to_numpy())

    def formed(self):
        raise AssertionError("the product was formed")
    monkeypatch.setattr(OperatorProduct, "to_tt", formed)
    monkeypatch.setattr(OperatorProduct, "to_numpy", formed)
    return OperatorProduct(M, x), OperatorProduct(N, y), z, dense


def test_host_dot_norm_and_fast_error_form_nothing(host_products, monkeypatch):
    from tt_sketch_amd import TensorSum, _native as nat, operator_gram as og
    h, q, z, dense = host_products
    monkeypatch.setattr(nat, "call", lambda *a: pytest.fail(f"the device was touched: {a[0]}"))
    scale = lambda a, b: 1e-12 * np.linalg.norm(dense[a]) * np.linalg.norm(dense[b])      # noqa: E731
    assert abs(og.op_tt_dot(h, z) - np.vdot(dense["h"], dense["z"])) <= scale("h", "z")
    assert abs(og.op_dot(h, q) - np.vdot(dense["h"], dense["q"])) <= scale("h", "q")
    assert abs(h.dot(z) - np.vdot(dense["h"], dense["z"])) <= scale("h", "z")
    assert abs(z.dot(h) - np.vdot(dense["h"], dense["z"])) <= scale("h", "z")             # from the train's side
    assert abs(h.dot(q) - np.vdot(dense["h"], dense["q"])) <= scale("h", "q")
    assert abs(q.dot(h) - h.dot(q)) <= scale("h", "q")
    assert abs(h.norm() - np.linalg.norm(dense["h"])) <= 1e-12 * np.linalg.norm(dense["h"])
    assert abs((h @ q) - h.dot(q)) == 0.0
    both = TensorSum([z, q])
    assert abs(h.dot(both) - np.vdot(dense["h"], dense["z"] + dense["q"])) <= scale("h", "z") + scale("h", "q")
    assert abs(both.dot(h) - np.vdot(dense["h"], dense["z"] + dense["q"])) <= scale("h", "z") + scale("h", "q")
    # the fast formula against the dense difference; the pairs are far apart, so its floor of 1e-8 does not show
    for a, b, da, db in ((h, q, "h", "q"), (h, z, "h", "z"), (z, h, "z", "h")):
        want = np.linalg.norm(dense[da] - dense[db])
        assert want / np.linalg.norm(dense[db]) >= 0.1
        assert abs(a.error(b, fast=True) - want) <= 1e-10 * want
        assert abs(a.error(b, fast=True, relative=True) - want / np.linalg.norm(dense[db])) <= 1e-10
        assert abs(a.error(b, fast=True, rmse=True) - want / np.sqrt(dense[da].size)) <= 1e-10 * want
    assert h.error(h, fast=True, relative=True) < 1e-7


def test_host_dot_checks_shapes_and_keeps_other_partners(host_products):
    from tt_sketch_amd import DenseTensor, OperatorProduct, TensorTrain
    h, q, z, dense = host_products
    other = TensorTrain([np.ones((1, n, 1)) for n in OUT_SHAPE[:-1] + (7,)])
    with pytest.raises(ValueError, match="shapes"):
        h.dot(other)
    wrong = OperatorProduct(_mpo(np.random.default_rng(1), IN_Y, (1, 1, 1)), q.tt)
    wrong.shape = other.shape
    with pytest.raises(ValueError, match="shapes"):
        h.dot(wrong)
    with pytest.raises(ValueError, match="route"):
        h.dot(q, route="fastest")
    with pytest.raises(AssertionError, match="formed"):           # a dense partner still goes through the base class
        h.dot(DenseTensor(dense["z"]))
    with pytest.raises(AssertionError, match="formed"):           # and fast=False keeps the path that forms the product
        z.error(h, fast=False)


@pytest.mark.parametrize("d", [3, 4])
def test_host_residual_of_a_sum_of_maps_against_dense(d, monkeypatch):
    from tt_sketch_amd import OperatorProduct, _native as nat
    from tt_sketch_amd.tt_gmres import MPO, TTLinearMapSum, TTLinearMap
    shape = (3, 5, 2, 4)[:d]
    rng = np.random.default_rng(d)
    rk = lambda r: (1,) + (r,) * (d - 1) + (1,)                                           # noqa: E731
    maps = [MPO([rng.standard_normal((rk(R)[k], shape[k], shape[k], rk(R)[k + 1])) for k in range(d)]) for R in (2, 3, 1)]
    x = _train(rng, shape, (3,) * (d - 1))
    b = _train(rng, shape, (2,) * (d - 1))

    class Twice(TTLinearMap):                                     # a map that is no MPO: applied, enters as a plain train
        in_shape = out_shape = shape

        def __call__(self, t):
            return t * 2.0

    A = TTLinearMapSum(maps + [Twice()])
    want = b.to_numpy() - sum(_dense_apply(m, x) for m in maps) - 2.0 * x.to_numpy()
    monkeypatch.setattr(OperatorProduct, "to_tt", lambda self: pytest.fail("a product was formed"))
    monkeypatch.setattr(MPO, "__call__", lambda self, t: pytest.fail("an operator was applied"))
    monkeypatch.setattr(nat, "call", lambda *a: pytest.fail(f"the device was touched: {a[0]}"))
    bn = np.linalg.norm(b.to_numpy())
    assert np.linalg.norm(want) / bn >= 0.1
    assert abs(A.residual(x, b) - np.linalg.norm(want)) <= 1e-10 * np.linalg.norm(want)
    assert abs(A.residual(x, b, relative=True) - np.linalg.norm(want) / bn) <= 1e-10 * np.linalg.norm(want) / bn


def test_route_rule_is_stated_and_nothing_is_exported():
    from tt_sketch_amd import hadamard_gram as hg, operator_gram as og
    kernel, composed = og.close_route_ms(4, 4, 20, 20, 20, 20, 80)
    assert kernel > 0 and composed > 0
    assert og._slices is hg._slices and og._scalar is hg._scalar and og._check is hg._check      # one definition
    assert "operator_gram" not in __import__("tt_sketch_amd").__all__
    rng = np.random.default_rng(0)
    assert not og.one_run(rng.standard_normal((3, 4, 5, 2))) and og.one_run(rng.standard_normal((3, 5, 4, 2)).transpose(0, 2, 1, 3))


def test_routing_rule_against_the_recorded_verdicts():
    """Only the rule is evaluated: at every shape of step B alone in profiles/operator_gram_bench.json where the two measured
    ranges are apart, it names the faster route; and it is within a quarter of the measured median of each route there."""
    import json
    from tt_sketch_amd import operator_gram as og
    with open(os.path.join(ROOT, "profiles", "operator_gram_bench.json")) as f:
        rows = json.load(f)["close_alone"]
    assert len(rows) >= 2
    decided = set()
    for row in rows:
        k, c = row["kernel_ms"], row["composed_ms"]                    # each [median, min, max]
        kernel_ms, composed_ms = og.close_route_ms(row["S"], row["S1"], row["s"], row["s1"], row["n_in"], row["n_out"], row["P"])
        named = "composed" if composed_ms < kernel_ms else "kernel"
        print(f"S {row['S']} s {row['s']} n {row['n_in']} P {row['P']}: kernel {k}, composed {c}; the rule expects {kernel_ms:.3f} / {composed_ms:.3f} ms -> {named}")
        assert abs(kernel_ms - k[0]) <= 0.25 * k[0] and abs(composed_ms - c[0]) <= 0.25 * c[0]
        if k[2] < c[1]:
            decided.add("kernel")
            assert named == "kernel"
        elif c[2] < k[1]:
            decided.add("composed")
            assert named == "composed"
    assert decided == {"kernel", "composed"}                           # each route wins at a measured shape


# ---- 4. the host-side plan
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "op_close_plan.h"
using namespace ttsk;
int main(int argc, char **argv)
{
    if (argc != 15) return 2;
    static double cell;
    int64_t dims[7], strides[7] = {1, 1, 1, 1, 1, 1, 1};
    for (int i = 0; i < 7; ++i) dims[i] = atoll(argv[1 + i]);
    const int accumulate = atoi(argv[8]);
    const long long work_doubles = atoll(argv[9]);
    const int null = atoi(argv[10]);           // bits: Wl, N, Y, dims, strides, out, work
    for (int i = 0; i < 4; ++i) strides[i] = atoll(argv[11 + i]);     // of N over (gamma, j, i, gamma')
    static OpClosePlan p, q;
    const int rc = op_close_plan(null & 1 ? nullptr : &cell, null & 2 ? nullptr : &cell, null & 4 ? nullptr : &cell,
                                 null & 8 ? nullptr : dims, null & 16 ? nullptr : strides, null & 32 ? nullptr : &cell,
                                 accumulate, null & 64 ? nullptr : &cell, work_doubles, &p);
    printf("rc %d\nmsg %s\n", rc, p.msg);
    printf("const %lld %d %d %d %zu %zu %lld %lld %d\n", (long long)HC_FILL, HD_KC, HD_COLS, HD_PITCH, HD_LDS, sizeof(OpCloseArgs),
           (long long)HC_TAIL_NUM, (long long)HC_TAIL_DEN, HC_TRIES);
    const int lrc = op_close_layout(null & 8 ? nullptr : dims, &q);
    printf("layout %d %d %d %lld %lld\n", lrc, q.a.jchunks, q.a.jper, (long long)q.slab, (long long)q.blocks);
    if (rc) return 0;
    printf("top %lld %.17g %d %d %d %d %d %lld\n", (long long)p.blocks, p.flops, p.a.ptiles, p.a.gtiles, p.a.cblocks, p.a.jchunks, p.a.jper,
           (long long)p.slab);
    printf("args %d %d %d %d %d %d %d\n", p.a.S, p.a.S1, p.a.s, p.a.s1, p.a.n_in, p.a.n_out, p.a.P);
    printf("run %lld\n", (long long)p.a.sNk);
    return 0;
}
"""


def _packed_strides(d):
    """element strides over (gamma, j, i, gamma') of a contiguous (S, n_out, n_in, S') array"""
    S, S1, s, s1, n_in, n_out, P = d
    return (n_out * n_in * S1, S1, n_in * S1, 1)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "op_close_plan", DRIVER)

    def run(dims, accumulate=0, work=2 ** 62, null=0, n_strides=None):
        """dims: (S, S', s, s', n_in, n_out, P); n_strides: of N, a packed core's unless given"""
        args = list(dims) + [accumulate, work, null] + list(_packed_strides(dims) if n_strides is None else n_strides)
        out = run_driver(exe, args).splitlines()
        p = dict(rc=int(out[0].split()[1]), msg=out[1][4:])
        for line in out[2:]:
            key, *v = line.split()
            p[key] = [float(x) if "." in x or "e" in x else int(x) for x in v]
        return p
    return run


def test_plan_constants_and_grid_arithmetic(plan):
    fill, kc, cols, pitch, lds, arg_bytes, tail_num, tail_den, tries = plan((1, 1, 1, 1, 1, 1, 1))["const"]
    assert (fill, (tail_num, tail_den), tries) == (ref.FILL, ref.TAIL, ref.TRIES)
    assert (cols, kc) == (hadamard_ref.COLS_PER_WORKGROUP, hadamard_ref.BETA_CHUNK)
    assert lds == kc * pitch * 8 and 2 * lds <= 160 * 1024       # the stage of hadamard_apply: two workgroups per compute unit
    assert arg_bytes <= 4096
    # the GMRES shape: operator rank 4 against train rank 20, n = 20, P = 80: five p tiles, one gamma' tile, one c' block;
    # every j a workgroup of its own
    p = plan((4, 4, 20, 20, 20, 20, 80))
    assert p["rc"] == 0 and p["top"][:1] + p["top"][2:] == [100, 5, 1, 1, 20, 1, 20 * 80 * 80]
    assert p["top"][1] == 2.0 * 20 * 80 * 4 * (20 * 4 * 20 + 20 * 20)
    # the wide shape: rank 8 against 64, n = 100, P = 512: 32 tiles, 16 chunks wanted: 15 ranges of seven j (the last of two)
    p = plan((8, 8, 64, 64, 100, 100, 512))
    jchunks, jper, slab, blocks = ref.layout(8, 8, 64, 64, 100, 100, 512)
    assert (jchunks, jper) == (15, 7) and p["top"][0] == blocks == 32 * 15 and p["top"][5:] == [jchunks, jper, slab]
    # tiles enough: the in-index is not cut
    p = plan((4, 40, 5, 300, 7, 3, 2000))
    assert p["top"][2:7] == [125, 3, 5, 1, 7] and p["top"][0] == 125 * 3 * 5 and p["top"][7] == 2000 * 300 * 40


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.name)
def test_plan_covers_every_case(plan, case):
    dims = ref.dims(case)
    _, N, _, _ = ref.case_arrays(case)
    jchunks, jper, slab, blocks = ref.layout(*dims)
    strides = tuple(x // 8 for x in N.strides)
    p = plan(dims, case.accumulate, slab, n_strides=strides)
    assert p["rc"] == 0, p["msg"]
    assert p["top"][2:5] == [-(-case.P // 16), -(-case.S1 // 16), -(-case.s1 // hadamard_ref.COLS_PER_WORKGROUP)]
    assert p["top"][0] == blocks and p["top"][5:] == [jchunks, jper, slab]
    assert (jchunks - 1) * jper < case.n_in <= jchunks * jper       # every chunk has a j, every j a chunk
    assert p["top"][1] == 2.0 * case.n_in * case.P * case.S1 * (case.s * case.S * case.n_out + case.s * case.s1)
    assert p["args"] == list(dims)
    assert p["run"] == [strides[2] if case.n_out > 1 else strides[0]]
    assert p["layout"] == [0, jchunks, jper, slab, blocks]          # ttsk_op_close_layout is the same arithmetic
    short = plan(dims, case.accumulate, slab - 1, n_strides=strides)
    assert short["rc"] == ERR_ARG and "slab" in short["msg"]


def test_plan_argument_errors_and_refusals(plan):
    ok = (2, 3, 4, 5, 6, 7, 8)
    assert plan(ok)["rc"] == 0 and plan(ok, 1)["rc"] == 0
    for bit in range(7):
        p = plan(ok, null=1 << bit)
        assert p["rc"] == ERR_ARG and "NULL" in p["msg"], bit
    assert plan(ok, null=8)["layout"][0] == ERR_ARG
    names = ["S", "S'", "s", "s'", "n_in", "n_out", "P"]
    for i in range(7):
        for value in (0, -3):
            bad = list(ok)
            bad[i] = value
            p = plan(bad)
            assert p["rc"] == ERR_ARG and f"{names[i]} = {value}" in p["msg"] and p["layout"][0] == ERR_ARG, i
    for accumulate in (-1, 2):
        p = plan(ok, accumulate)
        assert p["rc"] == ERR_ARG and "accumulate" in p["msg"]
    assert plan(ok, work=0)["rc"] == ERR_ARG and plan(ok, work=-1)["rc"] == ERR_ARG
    # the stride condition: (gamma, i) of N one run.  A core as an MPO stores it, (S, n_in, n_out, S') contiguous, is not
    S, S1, s, s1, n_in, n_out, P = ok
    stored = (n_in * n_out * S1, n_out * S1, S1, 1)
    p = plan(ok, n_strides=stored)
    assert p["rc"] == UNSUPPORTED and "one run" in p["msg"]
    assert plan(ok, work=0, n_strides=stored)["rc"] == ERR_ARG                     # argument errors come first
    padded = (n_out * (n_in + 2) * (S1 + 3), S1 + 3, (n_in + 2) * (S1 + 3), 1)    # runs apart: still one per (gamma, i)
    assert plan(ok, n_strides=padded)["rc"] == 0 and plan(ok, n_strides=padded)["run"] == [(n_in + 2) * (S1 + 3)]
    one_rank, one_out = (1,) + ok[1:], ok[:5] + (1,) + ok[6:]                      # an extent of 1 leaves one stride
    assert plan(one_rank, n_strides=stored)["rc"] == 0 and plan(one_rank, n_strides=stored)["run"] == [S1]
    assert plan(one_out, n_strides=stored)["rc"] == 0 and plan(one_out, n_strides=stored)["run"] == [stored[0]]
    # the cover: extents, S n_out and the number of workgroups below 2^31 (the slab is then below 2^45 doubles)
    big = 2 ** 31
    for i in range(7):
        wide = list(ok)
        wide[i] = big
        p = plan(wide)
        assert p["rc"] == UNSUPPORTED and "2^31" in p["msg"] and p["layout"][0] == UNSUPPORTED, i
    p = plan((2 ** 16, 3, 4, 5, 6, 2 ** 15, 8))
    assert p["rc"] == UNSUPPORTED and "S n_out" in p["msg"] and p["layout"][0] == UNSUPPORTED
    assert plan((2 ** 15, 3, 4, 5, 6, 2 ** 15, 8))["rc"] == 0
    assert plan((2, 3, 4, 5, 6, 7, big - 1))["rc"] == 0                  # the largest P: 2^27 tiles, the in-index not cut
    assert plan((2, 3, 4, 5, big - 1, 7, 8))["rc"] == 0                  # the longest in-index: 512 chunks
    p = plan((2, 2 ** 20, 4, 2 ** 26, 6, 7, 2 ** 16))                    # 2^12 x 2^16 x 2^20 tiles
    assert p["rc"] == UNSUPPORTED and "workgroups" in p["msg"]
    p = plan((2, 2 ** 30, 4, 64, 6, 7, 2 ** 30))                         # 2^26 x 2^26 tiles
    assert p["rc"] == UNSUPPORTED
    p = plan((2, 16, 4, big - 1, 6, 7, 16))                              # 2^25 blocks of c', a slab of 2^39 doubles
    assert p["rc"] == 0 and p["top"][7] == (big - 1) * 16 * 16
