"""Operator-times-train products that are never formed, without a GPU: the NumPy restatement of ``ttsk_op_apply``
(tests/op_apply_ref.py) against the explicit product and against np.longdouble, ``OperatorProduct`` on host cores against
the reference's recorded MPO product, its registration in the dispatch tables, and the host-side plan of the entry
(csrc/op_apply_plan.h, plain C++) compiled with the host compiler."""
import os

import numpy as np
import pytest

from tests import op_apply_ref as ref
from tests.edge_kit import rel_fro as rel
from tests.host_driver import ROOT, compile_driver, run_driver

ERR_ARG, UNSUPPORTED = -2, -3


# ---- 1. the restatement
@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.name)
def test_restatement_against_the_explicit_product_and_longdouble(case):
    terms, offs, w_cols = ref.case_arrays(case)
    assert len(terms) <= ref.MAX_TERMS
    for (L, M, C), t in zip(terms, case.terms):
        W, tol = ref.w_term(L, M, C), ref.bound(L, M, C)
        assert W.shape == (case.l, case.n_out, t.R1 * t.r1)
        assert (np.abs(W - ref.w_from_product(L, M, C)) <= tol).all()
        exact = ref.w_term(L, M, C, dtype=np.longdouble)
        ratio = float(np.max(np.abs(W - exact) / (tol / 2)))          # against the undoubled, first-order bound
        print(f"{case.name}: float64 against longdouble at {ratio:.2f} of the first-order bound")
        assert ratio <= 1.0
        if t.flipped:
            assert not C.flags.c_contiguous and (M is None or not M.flags.c_contiguous)
    # the blocks and the gaps tile the columns
    used = np.zeros(w_cols, dtype=int)
    for off, t in zip(offs, case.terms):
        used[off:off + t.R1 * t.r1] += 1
    assert used.max() == 1 and (used == 0).sum() == sum(t.gap for t in case.terms) + case.tail


# ---- 2. OperatorProduct on host cores
def _golden():
    from tt_sketch_amd import TensorTrain
    from tt_sketch_amd.tt_gmres import MPO
    z = np.load(os.path.join(ROOT, "tests", "golden", "gmres_case.npz"))
    d = len(z["shape"])
    return z, MPO([z[f"map2_core{k}"] for k in range(d)]), TensorTrain([z[f"b_core{k}"] for k in range(d)])


def test_operator_product_on_host_cores_against_the_recorded_product():
    from tt_sketch_amd import OperatorProduct, tt_gmres
    z, mpo, b = _golden()
    op = mpo.lazy(b)
    assert type(op) is OperatorProduct is tt_gmres.OperatorProduct
    assert op.shape == mpo.out_shape and op.rank == tuple(R * r for R, r in zip(mpo.rank, b.rank))
    assert op.size == mpo.size + b.size and op.ndim == len(op.shape)
    assert rel(op.to_numpy(), z["mpo_apply"]) < 1e-13
    tt = op.to_tt()
    assert tt.rank == op.rank and tt.shape == op.shape
    assert rel(tt.to_numpy(), z["mpo_apply"]) < 1e-13


def test_mode_reversal_scalar_multiples_and_shape_errors():
    from tt_sketch_amd import OperatorProduct, TensorTrain
    from tt_sketch_amd.tt_gmres import MPO
    rng = np.random.default_rng(4)
    in_shape, out_shape, R, r = (4, 5, 3), (5, 3, 6), (1, 3, 2, 1), (1, 2, 4, 1)
    mpo = MPO([rng.standard_normal((R[k], in_shape[k], out_shape[k], R[k + 1])) for k in range(3)])
    x = TensorTrain([rng.standard_normal((r[k], in_shape[k], r[k + 1])) for k in range(3)])
    op = OperatorProduct(mpo, x)
    dense = np.einsum("ijk,iajbkc->abc", x.to_numpy(), mpo.to_numpy())
    assert op.shape == out_shape and rel(op.to_numpy(), dense) < 1e-13
    assert op.T.shape == out_shape[::-1] and op.T.rank == op.rank[::-1]
    assert rel(op.T.to_numpy(), dense.transpose(2, 1, 0)) < 1e-13          # the mode reversal, not mpo.T
    assert rel(op.T.T.to_numpy(), op.to_numpy()) < 1e-15
    assert rel((op * -2.5).to_numpy(), -2.5 * dense) < 1e-13 and rel((0.5 * op).to_numpy(), 0.5 * dense) < 1e-13
    assert rel((op / 4).to_numpy(), dense / 4) < 1e-13 and rel((-op).to_numpy(), -dense) < 1e-13
    assert (op * 2.0).mpo is mpo                                           # the scalar goes into the train
    assert type(op + op).__name__ == "TensorSum" and (op + op).shape == out_shape
    with pytest.raises(ValueError):
        OperatorProduct(mpo, TensorTrain([rng.standard_normal((1, n, 1)) for n in (4, 5, 4)]))
    with pytest.raises(ValueError):
        mpo.lazy(TensorTrain([rng.standard_normal((1, n, 1)) for n in out_shape]))


# ---- 3. the plug-in surface
def test_dispatch_tables_know_the_new_kind():
    from tt_sketch_amd import DenseGaussianDRM, OperatorProduct, TensorTrainDRM, sketch_dispatch as sd
    from tt_sketch_amd.sketching_methods import abstract_methods as am, operator_product_sketch as ops
    assert sd.ABSTRACT_TENSOR_SKETCH_DISPATCH[OperatorProduct] is am.CansketchOperatorProduct
    assert sd.DRM_SKETCH_METHOD_DISPATCH[OperatorProduct] == "sketch_operator_product"
    assert sd.OMEGA_METHODS[OperatorProduct] is ops.sketch_omega_operator_product
    assert sd.PSI_METHODS[OperatorProduct] is ops.sketch_psi_operator_product
    assert issubclass(TensorTrainDRM, am.CansketchOperatorProduct) and not issubclass(DenseGaussianDRM, am.CansketchOperatorProduct)
    z, mpo, b = _golden()
    op = mpo.lazy(b)
    drm = DenseGaussianDRM.__new__(DenseGaussianDRM)                        # no device behind it: the lookup alone
    with pytest.raises(ValueError, match="can't sketch"):
        sd.get_sketch_method(op, drm)


def test_lazy_products_need_a_sketched_rounding():
    """raised before any device call: this test has no device"""
    from tt_sketch_amd.tt_gmres import MPO, TTLinearMapSum, tt_sum_gmres
    z, mpo, b = _golden()
    A = TTLinearMapSum([mpo])
    assert A.lazy is False and TTLinearMapSum([mpo], lazy=True).lazy is True
    for method in ("exact", "pairwise", None):
        with pytest.raises(ValueError, match="lazy_products"):
            tt_sum_gmres(A, b, max_rank=4, rounding_method=method, lazy_products=True)


# ---- 4. the host-side plan
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "op_apply_plan.h"
using namespace ttsk;
int main(int argc, char **argv)
{
    if (argc < 5) return 2;
    const int K = atoi(argv[1]), listed = atoi(argv[2]);
    const long long l = atoll(argv[3]), w_cols = atoll(argv[4]);
    if (listed < 0 || argc != 5 + 8 * listed) return 2;
    static double cell;
    std::vector<int64_t> dims, strides(7 * (size_t)listed, 1);
    std::vector<const double *> L, M, C;
    char **v = argv + 5;
    for (int t = 0; t < listed; ++t) {
        for (int i = 0; i < 7; ++i) dims.push_back(atoll(*v++));
        const int flags = atoi(*v++);          // 1: no operator, 2: NULL chain, 4: NULL train core
        M.push_back(flags & 1 ? nullptr : &cell);
        L.push_back(flags & 2 ? nullptr : &cell);
        C.push_back(flags & 4 ? nullptr : &cell);
    }
    static OpPlan p;
    const int rc = op_apply_plan(K, L.data(), M.data(), C.data(), dims.data(), strides.data(), l, &cell, w_cols, &p);
    printf("rc %d\nmsg %s\n", rc, p.msg);
    printf("const %d %d %d %d %d %zu %zu\n", OP_MAX_TERMS, OP_KC, OP_COL_TILES, OP_COLS, OP_PITCH, OP_LDS, sizeof(OpApplyArgs));
    if (rc) return 0;
    printf("top %lld %.17g %d %d %d\n", (long long)p.blocks, p.flops, p.a.K, p.a.l, p.a.n_out);
    for (int t = 0; t < K; ++t)
        printf("term %d %d %d %d %lld\n", p.a.t[t].block0, p.a.t[t].atiles, p.a.t[t].cblocks, p.a.t[t].plain, (long long)p.a.t[t].w_off);
    return 0;
}
"""


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "op_apply_plan", DRIVER)

    def run(l, w_cols, terms, K=None):
        """terms: rows (R, R', r, r', n_in, n_out, w_off, flags)"""
        args = [len(terms) if K is None else K, len(terms), l, w_cols] + [x for row in terms for x in row]
        out = run_driver(exe, args).splitlines()
        p = dict(rc=int(out[0].split()[1]), msg=out[1][4:], terms=[])
        for line in out[2:]:
            key, *v = line.split()
            if key == "term":
                p["terms"].append([int(x) for x in v])
            else:
                p[key] = [float(x) if "." in x or "e" in x else int(x) for x in v]
        return p
    return run


def _rows(case):
    _, offs, w_cols = ref.case_arrays(case)
    return [(t.R, t.R1, t.r, t.r1, t.n_in, case.n_out, off, 1 if t.plain else 0) for t, off in zip(case.terms, offs)], w_cols


def test_plan_lds_and_argument_arithmetic(plan):
    rows, w_cols = _rows(ref.CASES[0])
    max_terms, kc, col_tiles, cols, pitch, lds, arg_bytes = plan(1, w_cols, rows)["const"]
    assert (max_terms, cols, kc) == (ref.MAX_TERMS, ref.COLS_PER_WORKGROUP, ref.ROW_CHUNK) and cols == 16 * col_tiles
    # a row of T1 is one 16 x 16 tile plus padding; the two rows a half-wave's 64-bit LDS read touches are `pitch` doubles
    # apart, 16 modulo 32 puts their 2 x 32 dwords on 64 different banks
    assert pitch >= 256 and pitch % 32 == 16
    assert lds == (kc * pitch + kc) * 8 and 2 * lds <= 160 * 1024       # two workgroups' stages fit the LDS of a compute unit
    assert arg_bytes <= 4096                                            # the table travels as the kernel's argument


@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.name)
def test_plan_covers_every_case(plan, case):
    rows, w_cols = _rows(case)
    p = plan(case.l, w_cols, rows)
    assert p["rc"] == 0, p["msg"]
    blocks, flops, K, l, n_out = p["top"]
    want, at = [], 0
    for t in case.terms:
        atiles, cblocks = -(-t.r1 // 16), -(-(case.n_out * t.R1) // ref.COLS_PER_WORKGROUP)
        want.append([at, atiles, cblocks, int(t.plain)])
        at += -(-case.l // 16) * atiles * cblocks
    assert [row[:4] for row in p["terms"]] == want and blocks == at
    assert (K, l, n_out) == (len(case.terms), case.l, case.n_out)
    assert flops == sum(2.0 * case.l * (t.R * t.r * t.n_in * t.r1 + t.R * t.n_in * case.n_out * t.R1 * t.r1) for t in case.terms)


def test_plan_argument_errors_and_refusals(plan):
    ok = (2, 3, 4, 5, 6, 7, 0, 0)
    assert plan(8, 15, [ok])["rc"] == 0
    assert plan(8, 15, [ok], K=0)["rc"] == ERR_ARG
    assert plan(0, 15, [ok])["rc"] == ERR_ARG and plan(8, 0, [ok])["rc"] == ERR_ARG
    for i in range(6):
        bad = list(ok)
        bad[i] = 0
        assert plan(8, 15, [tuple(bad)])["rc"] == ERR_ARG, i
    assert plan(8, 15, [ok[:6] + (-1, 0)])["rc"] == ERR_ARG
    assert plan(8, 15, [ok[:7] + (2,)])["rc"] == ERR_ARG and plan(8, 15, [ok[:7] + (4,)])["rc"] == ERR_ARG      # NULL chain / core
    assert plan(8, 14, [ok])["rc"] == ERR_ARG                                  # 3 x 5 columns do not fit 14
    assert plan(8, 15, [ok[:6] + (1, 0)])["rc"] == ERR_ARG                     # nor 15 from offset 1
    assert plan(8, 30, [ok, (2, 3, 4, 5, 6, 8, 15, 0)])["rc"] == ERR_ARG       # differing n_out
    plain = (1, 1, 4, 5, 7, 7, 0, 1)
    assert plan(8, 5, [plain])["rc"] == 0
    assert plan(8, 5, [(2, 1, 4, 5, 7, 7, 0, 1)])["rc"] == ERR_ARG             # no operator and R != 1
    assert plan(8, 10, [(1, 2, 4, 5, 7, 7, 0, 1)])["rc"] == ERR_ARG
    assert plan(8, 5, [(1, 1, 4, 5, 6, 7, 0, 1)])["rc"] == ERR_ARG             # no operator and n_in != n_out
    # the cover: extents below 2^31, at most OP_MAX_TERMS terms
    big = 2 ** 31
    assert plan(big, 15, [ok])["rc"] == UNSUPPORTED and plan(8, big, [ok])["rc"] == UNSUPPORTED
    for i in range(6):
        wide = list(ok)
        wide[i] = big
        assert plan(8, 15, [tuple(wide)])["rc"] == UNSUPPORTED, i
    assert plan(8, 15, [(2 ** 16, 3, 4, 5, 2 ** 15, 7, 0, 0)])["rc"] == UNSUPPORTED      # R n_in = 2^31
    one = (1, 1, 1, 1, 1, 1)
    assert plan(1, ref.MAX_TERMS, [one + (t, 0) for t in range(ref.MAX_TERMS)])["rc"] == 0
    p = plan(1, ref.MAX_TERMS + 1, [one + (t, 0) for t in range(ref.MAX_TERMS + 1)])
    assert p["rc"] == UNSUPPORTED and str(ref.MAX_TERMS) in p["msg"]
