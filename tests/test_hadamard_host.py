"""Entrywise products of two tensor trains that are never formed, without a GPU: the NumPy restatement of
``ttsk_hadamard_apply`` (tests/hadamard_ref.py) against the explicit Kronecker core and against np.longdouble,
``HadamardProduct`` on host cores, its registration in the dispatch tables, and the host-side plan of the entry
(csrc/hadamard_plan.h, plain C++) compiled with the host compiler."""

import numpy as np
import pytest

from tests import hadamard_ref as ref
from tests.edge_kit import rel_fro as rel
from tests.host_driver import compile_driver, run_driver

ERR_ARG, UNSUPPORTED = -2, -3


# ---- 1. the restatement
@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.name)
def test_restatement_against_the_explicit_product_and_longdouble(case):
    L, X, Y, w_off, w_cols = ref.case_arrays(case)
    W, tol = ref.w_term(L, X, Y), ref.bound(L, X, Y)
    assert W.shape == (case.l, case.n, case.R1 * case.r1) and ref.depth(L, X, Y) == case.r + case.R + 2
    assert (np.abs(W - ref.w_from_product(L, X, Y)) <= tol).all()
    exact = ref.w_term(L, X, Y, dtype=np.longdouble)
    ratio = float(np.max(np.abs(W - exact) / (tol / 2)))          # against the undoubled, first-order bound
    print(f"{case.name}: float64 against longdouble at {ratio:.2f} of the first-order bound")
    assert ratio <= 1.0
    for a, layout in ((X, case.x_layout), (Y, case.y_layout)):
        assert a.flags.c_contiguous == (layout == "c") or a.size == max(a.shape)
    assert w_off == case.gap and w_cols == case.gap + case.R1 * case.r1 + case.tail


def test_cases_reach_every_edge():
    """the case list is what the plan's constants make of it: every edge extent occurs"""
    for field in ("r", "r1", "l"):
        assert set(ref.EDGES_SMALL) <= {getattr(c, field) for c in ref.CASES}, field
    assert set(ref.EDGES_R) <= {c.R for c in ref.CASES} and set(ref.EDGES_R1) <= {c.R1 for c in ref.CASES}
    assert set(ref.EDGES_N) <= {c.n for c in ref.CASES}
    assert any(c.R != c.R1 and c.r != c.r1 for c in ref.CASES)
    assert any(c.x_layout == c.y_layout == "flipped" for c in ref.CASES)
    assert any(c.x_layout != c.y_layout and "c" not in (c.x_layout, c.y_layout) for c in ref.CASES)
    assert any(c.gap and c.tail for c in ref.CASES)
    assert any(c.R1 > ref.COLS_PER_WORKGROUP and c.R > ref.BETA_CHUNK for c in ref.CASES)       # stage 1 formed again, two chunks
    assert len({c.name for c in ref.CASES}) == len(ref.CASES)


# ---- 2. HadamardProduct on host cores
def _pair(seed=4, shape=(4, 5, 3), Rx=(1, 3, 2, 1), ry=(1, 2, 4, 1)):
    from tt_sketch_amd import TensorTrain
    rng = np.random.default_rng(seed)
    d = len(shape)
    x = TensorTrain([rng.standard_normal((Rx[k], shape[k], Rx[k + 1])) for k in range(d)])
    y = TensorTrain([rng.standard_normal((ry[k], shape[k], ry[k + 1])) for k in range(d)])
    return x, y


def test_hadamard_product_on_host_cores():
    from tt_sketch_amd import HadamardProduct, OperatorProduct, hadamard_product
    from tt_sketch_amd.tt_gmres import MPO
    x, y = _pair()
    h = x.hadamard(y)
    assert type(h) is HadamardProduct is hadamard_product.HadamardProduct and h.x is x and h.y is y
    dense = x.to_numpy() * y.to_numpy()
    assert h.shape == x.shape and h.rank == (6, 8) and h.ndim == 3 and h.size == x.size + y.size
    assert rel(h.to_numpy(), dense) < 1e-12
    tt = h.to_tt()
    assert tt.rank == h.rank and tt.shape == h.shape and rel(tt.to_numpy(), dense) < 1e-12
    # x outer: the cores of the diagonal operator of x applied to y
    diag = []
    for C in x.cores:
        M = np.zeros((C.shape[0], C.shape[1], C.shape[1], C.shape[2]))
        for i in range(C.shape[1]):
            M[:, i, i, :] = C[:, i, :]
        diag.append(M)
    want = OperatorProduct(MPO(diag), y).to_tt()
    assert tt.rank == want.rank
    for got, exp in zip(tt.cores, want.cores):
        assert got.shape == exp.shape and np.allclose(got, exp, rtol=1e-15, atol=0.0)
    assert rel(y.hadamard(x).to_numpy(), dense) < 1e-12 and y.hadamard(x).rank == h.rank         # the other factor outer
    assert "asymmetric" in HadamardProduct.__doc__ or "not symmetric" in HadamardProduct.__doc__
    assert "Hadamard" in repr(h) and str(h.shape) in repr(h)


def test_mode_reversal_scalar_multiples_and_shape_errors():
    from tt_sketch_amd import HadamardProduct, TensorTrain
    x, y = _pair(5)
    h = HadamardProduct(x, y)
    dense = x.to_numpy() * y.to_numpy()
    assert h.T.shape == h.shape[::-1] and h.T.rank == h.rank[::-1]
    assert rel(h.T.to_numpy(), dense.transpose(2, 1, 0)) < 1e-13 and rel(h.T.T.to_numpy(), dense) < 1e-15
    assert all(np.shares_memory(a, b) for a, b in zip(h.T.x.cores, x.cores[::-1]))            # views: nothing is copied
    assert all(np.shares_memory(a, b) for a, b in zip(h.T.y.cores, y.cores[::-1]))
    assert rel((h * -2.5).to_numpy(), -2.5 * dense) < 1e-13 and rel((0.5 * h).to_numpy(), 0.5 * dense) < 1e-13
    assert rel((h / 4).to_numpy(), dense / 4) < 1e-13 and rel((-h).to_numpy(), -dense) < 1e-13
    assert (h * 2.0).x is x                                                # the scalar goes into y
    assert type(h + h).__name__ == "TensorSum" and (h + h).shape == h.shape
    assert rel((x * 3.0).to_numpy(), 3.0 * x.to_numpy()) < 1e-15 and type(x * 3.0) is TensorTrain      # __mul__ is the scalar's still
    other = TensorTrain([np.ones((1, n, 1)) for n in (4, 5, 4)])
    with pytest.raises(ValueError):
        HadamardProduct(x, other)
    with pytest.raises(ValueError):
        x.hadamard(TensorTrain([np.ones((1, n, 1)) for n in (4, 5)]))


class _Reached(Exception):
    pass


@pytest.mark.parametrize("method", ["exact", "pairwise", None])
def test_unsketched_roundings_form_the_product_first(method, monkeypatch):
    """raised before any device call: this test has no device"""
    from tt_sketch_amd import HadamardProduct, hadamard_round, tt_gmres
    assert hadamard_round is __import__("tt_sketch_amd").hadamard_product.hadamard_round
    x, y = _pair(6)
    formed = []

    def to_tt(self):
        formed.append((self.x, self.y))
        raise _Reached("to_tt")
    monkeypatch.setattr(HadamardProduct, "to_tt", to_tt)
    with pytest.raises(_Reached):
        hadamard_round(x, y, 4, method=method)
    assert formed == [(x, y)]
    formed.clear()
    with pytest.raises(_Reached):
        tt_gmres.round_tt_sum(x + x.hadamard(y), 4, method=method)
    assert len(formed) == 1
    with pytest.raises(ValueError, match="Unknown rounding"):
        monkeypatch.undo()
        hadamard_round(x, y, 4, method="nearest")


# ---- 3. the plug-in surface
def test_dispatch_tables_know_the_new_kind():
    from tt_sketch_amd import DenseGaussianDRM, HadamardProduct, TensorTrainDRM, hadamard_fused, sketch_dispatch as sd
    from tt_sketch_amd.sketching_methods import abstract_methods as am, hadamard_product_sketch as hps
    assert sd.ABSTRACT_TENSOR_SKETCH_DISPATCH[HadamardProduct] is am.CansketchHadamardProduct
    assert sd.DRM_SKETCH_METHOD_DISPATCH[HadamardProduct] == "sketch_hadamard_product"
    assert sd.OMEGA_METHODS[HadamardProduct] is hps.sketch_omega_hadamard_product
    assert sd.PSI_METHODS[HadamardProduct] is hps.sketch_psi_hadamard_product
    assert issubclass(TensorTrainDRM, am.CansketchHadamardProduct) and not issubclass(DenseGaussianDRM, am.CansketchHadamardProduct)
    assert hadamard_fused.try_hadamard_sketch in sd.FUSED_PATHS + sd.PRODUCT_PATHS
    x, y = _pair()
    drm = DenseGaussianDRM.__new__(DenseGaussianDRM)                        # no device behind it: the lookup alone
    with pytest.raises(ValueError, match="can't sketch"):
        sd.get_sketch_method(x.hadamard(y), drm)
    # the fused path declines what is not its own before it touches anything
    assert hadamard_fused.try_hadamard_sketch(object(), None, None, sd.SketchMethod.streaming) is None
    assert hadamard_fused.try_hadamard_sketch(x.hadamard(y), None, None, sd.SketchMethod.orthogonal) is None


def test_route_is_validated_before_the_device():
    from tt_sketch_amd import hadamard_product as hp
    with pytest.raises(ValueError, match="route"):
        hp.hadamard_apply(None, None, None, route="fastest")
    kernel, composed = hp.route_ms(20, 20, 20, 20, 20, 20)
    assert kernel > 0 and composed > 0


# ---- 4. the host-side plan
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "hadamard_plan.h"
using namespace ttsk;
int main(int argc, char **argv)
{
    if (argc != 10) return 2;
    static double cell;
    int64_t dims[6], strides[6] = {1, 1, 1, 1, 1, 1};
    for (int i = 0; i < 6; ++i) dims[i] = atoll(argv[1 + i]);
    const long long w_cols = atoll(argv[7]), w_off = atoll(argv[8]);
    const int null = atoi(argv[9]);            // bits: L, X, Y, dims, strides, W
    static HadamardPlan p;
    const int rc = hadamard_apply_plan(null & 1 ? nullptr : &cell, null & 2 ? nullptr : &cell, null & 4 ? nullptr : &cell,
                                       null & 8 ? nullptr : dims, null & 16 ? nullptr : strides, null & 32 ? nullptr : &cell,
                                       w_cols, w_off, &p);
    printf("rc %d\nmsg %s\n", rc, p.msg);
    printf("const %d %d %d %d %zu %zu\n", HD_KC, HD_COL_TILES, HD_COLS, HD_PITCH, HD_LDS, sizeof(HadamardArgs));
    if (rc) return 0;
    printf("top %lld %.17g %d %d %d\n", (long long)p.blocks, p.flops, p.a.ltiles, p.a.atiles, p.a.cblocks);
    printf("args %d %d %d %d %d %d %lld %lld\n", p.a.R, p.a.R1, p.a.r, p.a.r1, p.a.n, p.a.l, (long long)p.a.w_cols, (long long)p.a.w_off);
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "hadamard_plan", DRIVER)

    def run(dims, w_cols, w_off=0, null=0):
        """dims: (R, R', r, r', n, l)"""
        args = list(dims) + [w_cols, w_off, null]
        out = run_driver(exe, args).splitlines()
        p = dict(rc=int(out[0].split()[1]), msg=out[1][4:])
        for line in out[2:]:
            key, *v = line.split()
            p[key] = [float(x) if "." in x or "e" in x else int(x) for x in v]
        return p
    return run


def test_plan_lds_and_grid_arithmetic(plan):
    kc, col_tiles, cols, pitch, lds, arg_bytes = plan((1, 1, 1, 1, 1, 1), 1)["const"]
    assert (cols, kc) == (ref.COLS_PER_WORKGROUP, ref.BETA_CHUNK) and cols == ref.TILE * col_tiles and kc % ref.KBLOCK == 0
    # a row of T1 is one 16 x 16 tile plus padding; the two rows a half-wave's 64-bit LDS read touches are `pitch` doubles
    # apart, 16 modulo 32 puts their 2 x 32 dwords on 64 different banks
    assert pitch >= ref.TILE * ref.TILE and pitch % 32 == 16
    assert lds == kc * pitch * 8 and 2 * lds <= 160 * 1024       # two workgroups' stages fit the LDS of a compute unit
    assert arg_bytes <= 4096
    p = plan((50, 50, 50, 50, 200, 50), 2500)
    assert p["rc"] == 0 and p["top"][0] == 200 * 4 * 4 * 1               # i sits in the grid: thousands of workgroups
    p = plan((3, 300, 5, 40, 7, 33), 12000)
    cblocks = -(-300 // cols)
    assert p["top"][2:] == [3, 3, cblocks] and p["top"][0] == 7 * 3 * 3 * cblocks


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.name)
def test_plan_covers_every_case(plan, case):
    _, _, _, w_off, w_cols = ref.case_arrays(case)
    p = plan((case.R, case.R1, case.r, case.r1, case.n, case.l), w_cols, w_off)
    assert p["rc"] == 0, p["msg"]
    blocks, flops, ltiles, atiles, cblocks = p["top"]
    assert (ltiles, atiles, cblocks) == (-(-case.l // ref.TILE), -(-case.r1 // ref.TILE), -(-case.R1 // ref.COLS_PER_WORKGROUP))
    assert blocks == case.n * ltiles * atiles * cblocks
    assert flops == 2.0 * case.l * case.n * (case.R * case.r * case.r1 + case.R * case.R1 * case.r1)
    assert p["args"] == [case.R, case.R1, case.r, case.r1, case.n, case.l, w_cols, w_off]


def test_plan_argument_errors_and_refusals(plan):
    ok = (2, 3, 4, 5, 6, 8)
    assert plan(ok, 15)["rc"] == 0 and plan(ok, 20, 5)["rc"] == 0
    for bit in range(6):
        p = plan(ok, 15, null=1 << bit)
        assert p["rc"] == ERR_ARG and "NULL" in p["msg"], bit
    names = ["R", "R'", "r", "r'", "n", "l"]
    for i in range(6):
        bad = list(ok)
        bad[i] = 0
        p = plan(bad, 15)
        assert p["rc"] == ERR_ARG and f"{names[i]} = 0" in p["msg"], i
    assert plan(ok, 0)["rc"] == ERR_ARG and plan(ok, 15, -1)["rc"] == ERR_ARG
    p = plan(ok, 14)                                                    # 3 x 5 columns do not fit 14
    assert p["rc"] == ERR_ARG and "pass w_cols = 14" in p["msg"]
    assert plan(ok, 15, 1)["rc"] == ERR_ARG and plan(ok, 15, 16)["rc"] == ERR_ARG     # nor 15 from offset 1
    # the cover: extents and the number of workgroups below 2^31
    big = 2 ** 31
    for i in range(6):
        wide = list(ok)
        wide[i] = big
        p = plan(wide, 15)
        assert p["rc"] == UNSUPPORTED and "2^31" in p["msg"], i
    assert plan(ok, big)["rc"] == UNSUPPORTED
    assert plan((2, 3, 4, 5, 6, big - 1), 15)["rc"] == 0                # the largest l: 2^27 tiles x 6 modes
    p = plan((2, 3, 4, 5, 2 ** 20, 2 ** 16), 15)                        # 2^20 modes x 2^12 tiles
    assert p["rc"] == UNSUPPORTED and "workgroups" in p["msg"]
    assert plan((2, 3, 4, 5, 2 ** 19, 2 ** 16 - 16), 15)["rc"] == 0
