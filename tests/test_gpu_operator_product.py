"""Operator-times-train products that are never formed, on the device: ``ttsk_op_apply`` (csrc/op_apply.hip) entry by
entry, ``OperatorProduct`` through the generic sketch driver and through the fused path of ``operator_fused``, and
``tt_sum_gmres(..., lazy_products=True)``.

Bar of the entry (tests/op_apply_ref.py): |W - W_ref| <= 2 (r + R n_in + 2) 2^-53 W_abs entry by entry, the same bits on a
second call, nothing written outside the terms' column blocks.  Bars of the sketches: Psi / Omega
within 1e-12 ||ref||_F of the same call on the explicit product, the results as tensors within 1e-8.
"""
import ctypes
import os

import numpy as np
import pytest

from oracle import ttsk_oracle as orc
from tests import op_apply_ref as ref
from tests.edge_kit import rel_fro as rel, tsa  # noqa: F401

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3


def _upload(a):
    """(device array that owns the data, element strides of `a` in it): a transposed view is uploaded as its base"""
    from tt_sketch_amd.device import DevArray
    if a.flags.c_contiguous:
        return DevArray.from_host(a), tuple(s // 8 for s in a.strides)
    assert a.base is not None and a.base.flags.c_contiguous and a.base.size == a.size
    return DevArray.from_host(a.base), tuple(s // 8 for s in a.strides)


def c_op_apply(terms, offs, l, n_out, w_cols, K=None, dims=None, l_arg=None, w_cols_arg=None, null=()):
    """One direct call of the C entry on host arrays into a W pre-filled with NaN: (status, W).  The keyword arguments
    overwrite what the arrays say, for the argument tests."""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    keep, Lp, Mp, Cp, dm, st = [], [], [], [], [], []
    for (L, M, C), off in zip(terms, offs):
        dL = DevArray.from_host(np.ascontiguousarray(L))
        dC, sC = _upload(C)
        dM, sM = _upload(M) if M is not None else (None, (0, 0, 0, 0))
        keep += [dL, dC, dM]
        Lp.append(dL.ptr); Cp.append(dC.ptr); Mp.append(None if dM is None else dM.ptr)
        R1 = 1 if M is None else M.shape[3]
        dm += [L.shape[0], R1, C.shape[0], C.shape[2], C.shape[1], n_out, off]
        st += list(sM) + list(sC)
    W = DevArray.from_host(np.full((l, n_out, w_cols), np.nan))
    k = len(terms)
    args = dict(L=(ctypes.c_void_p * k)(*Lp), M=(ctypes.c_void_p * k)(*Mp), C=(ctypes.c_void_p * k)(*Cp),
                dims=nat.i64_array(dm if dims is None else dims), strides=nat.i64_array(st), W=ctypes.c_void_p(W.ptr))
    for name in null:
        args[name] = None
    rc = nat.lib().ttsk_op_apply(k if K is None else K, args["L"], args["M"], args["C"], args["dims"], args["strides"],
                                 l if l_arg is None else l_arg, args["W"], w_cols if w_cols_arg is None else w_cols_arg, 0)
    nat.call("ttsk_sync", -1)
    return rc, W.get()


# ---- 1. the C entry against the restatement at every edge
@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.name)
def test_c_entry_vs_restatement(tsa, case):
    terms, offs, w_cols = ref.case_arrays(case)
    rc, W = c_op_apply(terms, offs, case.l, case.n_out, w_cols)
    assert rc == 0
    touched = np.zeros(w_cols, dtype=bool)
    for (L, M, C), off in zip(terms, offs):
        want, tol = ref.w_term(L, M, C), ref.bound(L, M, C)
        got = W[:, :, off:off + want.shape[2]]
        touched[off:off + want.shape[2]] = True
        assert np.isfinite(got).all()
        miss = np.abs(got - want)
        print(f"{case.name}: max |W - W_ref| / bound = {np.max(miss / np.maximum(tol, 1e-300)):.3f}")
        assert (miss <= tol).all()
    assert np.isnan(W[:, :, ~touched]).all()                 # nothing outside the terms' blocks
    rc2, W2 = c_op_apply(terms, offs, case.l, case.n_out, w_cols)
    assert rc2 == 0 and np.array_equal(W, W2, equal_nan=True)          # the same bits on every call


# ---- 2. the ABI
def test_argument_errors_and_refusals_write_nothing(tsa):
    from tt_sketch_amd import _native as nat
    case = next(c for c in ref.CASES if c.name == "ragged3_gaps")
    terms, offs, w_cols = ref.case_arrays(case)
    l, n_out = case.l, case.n_out
    good = [x for (L, M, C), off in zip(terms, offs)
            for x in (L.shape[0], 1 if M is None else M.shape[3], C.shape[0], C.shape[2], C.shape[1], n_out, off)]

    def status(**kw):
        rc, W = c_op_apply(terms, offs, l, n_out, w_cols, **kw)
        assert np.isnan(W).all(), kw                          # refused before anything is launched
        return rc

    def with_dim(term, field, value):
        d = list(good)
        d[7 * term + field] = value
        return d

    for name in ("L", "M", "C", "dims", "strides", "W"):
        assert status(null=(name,)) == nat.TTSK_ERR_ARG, name
    assert status(K=0) == nat.TTSK_ERR_ARG and status(l_arg=0) == nat.TTSK_ERR_ARG and status(w_cols_arg=0) == nat.TTSK_ERR_ARG
    for field in range(6):
        assert status(dims=with_dim(0, field, 0)) == nat.TTSK_ERR_ARG, field
    assert status(dims=with_dim(1, 0, 2)) == nat.TTSK_ERR_ARG                     # the term without operator: R != 1
    assert b"no operator" in nat.lib().ttsk_last_error()
    assert status(dims=with_dim(1, 1, 2)) == nat.TTSK_ERR_ARG                     # R' != 1
    assert status(dims=with_dim(1, 4, 6)) == nat.TTSK_ERR_ARG                     # n_in != n_out
    assert status(dims=with_dim(2, 6, w_cols)) == nat.TTSK_ERR_ARG                # its block passes w_cols
    assert status(w_cols_arg=offs[2]) == nat.TTSK_ERR_ARG
    assert status(dims=with_dim(2, 5, n_out + 1)) == nat.TTSK_ERR_ARG             # differing n_out
    assert status(l_arg=2 ** 31) == UNSUPPORTED and status(w_cols_arg=2 ** 31) == UNSUPPORTED
    assert b"2^31" in nat.lib().ttsk_last_error()
    assert status(dims=with_dim(0, 2, 2 ** 31)) == UNSUPPORTED
    one = (np.ones((1, 1, 1)), np.ones((1, 1, 1, 1)), np.ones((1, 1, 1)))
    many = ref.MAX_TERMS + 1
    rc, W = c_op_apply([one] * many, list(range(many)), 1, 1, many)
    assert rc == UNSUPPORTED and np.isnan(W).all() and str(ref.MAX_TERMS).encode() in nat.lib().ttsk_last_error()
    rc, W = c_op_apply([one] * ref.MAX_TERMS, list(range(ref.MAX_TERMS)), 1, 1, ref.MAX_TERMS)
    assert rc == 0 and np.array_equal(W, np.ones((1, 1, ref.MAX_TERMS)))


def test_python_cuts_lists_longer_than_one_call(tsa):
    """51 small terms: the routing rule keeps the kernel, in three calls of at most 24 terms"""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    from tt_sketch_amd.operator_product import op_apply
    rng = np.random.default_rng(7)
    K, l, n = 2 * ref.MAX_TERMS + 3, 3, 4
    host = [(rng.standard_normal((2, 3, l)), rng.standard_normal((2, n, n, 1)) if p % 5 else None, rng.standard_normal((3, n, 2))) for p in range(K)]
    host = [(L[:1] if M is None else L, M, C) for L, M, C in host]
    calls, real = [], nat.call
    try:
        nat.call = lambda name, *args: (calls.append(name), real(name, *args))[1]
        W, offs = op_apply([DevArray.from_host(L) for L, _, _ in host], [None if M is None else DevArray.from_host(M) for _, M, _ in host],
                           [DevArray.from_host(C) for _, _, C in host])
    finally:
        nat.call = real
    assert calls.count("ttsk_op_apply") == 3 and offs == [2 * p for p in range(K)]
    got = W.get()
    for (L, M, C), off in zip(host, offs):
        assert (np.abs(got[:, :, off:off + 2] - ref.w_term(L, M, C)) <= ref.bound(L, M, C)).all()


# ---- 3. the generic driver
IN_SHAPE, OUT_SHAPE = (4, 5, 3, 6), (5, 3, 6, 4)


def _product(tsa, seed, op_rank=3, tt_rank=(2, 17, 3)):
    from tt_sketch_amd.tt_gmres import MPO
    rng = np.random.default_rng(seed)
    R = (1,) + (op_rank,) * 3 + (1,)
    mpo = MPO([rng.standard_normal((R[k], IN_SHAPE[k], OUT_SHAPE[k], R[k + 1])) / np.sqrt(R[k] * IN_SHAPE[k]) for k in range(4)])
    x = tsa.TensorTrain(orc.random_tt(IN_SHAPE, tt_rank, rng))
    return mpo, x


def _drms(tsa, left_rank, right_rank, seed=0):
    rng = np.random.default_rng(seed)
    ld, rd = orc.random_tt_drm(OUT_SHAPE, left_rank, False, rng), orc.random_tt_drm(OUT_SHAPE, right_rank, True, rng)
    return (tsa.TensorTrainDRM(left_rank, OUT_SHAPE, transpose=False, cores=ld.cores),
            tsa.TensorTrainDRM(right_rank, OUT_SHAPE, transpose=True, cores=rd.cores))


def _same_sketch(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and np.linalg.norm(a - b) <= 1e-12 * np.linalg.norm(b)


def test_routing_rule_at_the_measured_shapes(tsa):
    """the rule against the verdicts of profiles/operator_sketch_bench.json: the composed W for one term at K1 and K2, the
    kernel for the three small terms of a Krylov step; and both routes give the same W inside the bound"""
    from tt_sketch_amd import operator_product as opm
    from tt_sketch_amd.device import DevArray
    k1, k2 = (4, 4, 20, 20, 20, 20, 20, False), (8, 8, 64, 64, 100, 100, 50, False)
    for one in (k1, k2):
        kernel, composed = opm.route_ms([one])
        assert composed < kernel
    kernel, composed = opm.route_ms([k1] * 3)
    assert kernel < composed
    case = next(c for c in ref.CASES if c.name == "ragged3_gaps")
    terms, offs, _ = ref.case_arrays(case)
    dev = [(DevArray.from_host(np.ascontiguousarray(L)), None if M is None else _upload(M), _upload(C)) for L, M, C in terms]
    view = lambda up, a: DevArray(up[0].buf, 0, a.shape, up[1])
    Ls, Ms, Cs = [d[0] for d in dev], [None if d[1] is None else view(d[1], t[1]) for d, t in zip(dev, terms)], [view(d[2], t[2]) for d, t in zip(dev, terms)]
    for route in ("composed", "kernel"):                       # all terms and one term
        W, got_offs = opm.op_apply(Ls, Ms, Cs, route=route)
        W1, _ = opm.op_apply(Ls[:1], Ms[:1], Cs[:1], route=route)
        W, W1, at = W.get(), W1.get(), 0
        for (L, M, C) in terms:
            want, tol = ref.w_term(L, M, C), ref.bound(L, M, C)
            assert (np.abs(W[:, :, at:at + want.shape[2]] - want) <= tol).all()
            at += want.shape[2]
        assert at == W.shape[2] and (np.abs(W1 - ref.w_term(*terms[0])) <= ref.bound(*terms[0])).all()
    with pytest.raises(ValueError):
        opm.op_apply(Ls, Ms, Cs, route="fastest")


@pytest.mark.parametrize("routed", [False, True], ids=["kernel", "routed"])
def test_generic_driver_against_the_explicit_product(tsa, routed, monkeypatch):
    from tt_sketch_amd import OperatorProduct, SketchMethod, operator_product
    from tt_sketch_amd.sketch_dispatch import general_sketch_device
    if not routed:          # the rule sends one term to the composed W: here the kernel at every step, undone by monkeypatch
        monkeypatch.setattr(operator_product, "route_ms", lambda dims: (0.0, 1.0))
    mpo, x = _product(tsa, 1)
    op, explicit = OperatorProduct(mpo, x), mpo(x)
    assert op.rank == explicit.rank == (6, 51, 9)
    assert rel(op.to_numpy(), explicit.to_numpy()) < 1e-13 and rel(op.T.to_numpy(), explicit.T.to_numpy()) < 1e-13
    lr, rr = (4, 7, 5), (6, 9, 8)
    left, right = _drms(tsa, lr, rr)
    # streaming, through general_sketch_device: the plug-in tables, not the fused path
    Psi, Om = general_sketch_device(op, left, right, SketchMethod.streaming)
    Psi_e, Om_e = general_sketch_device(explicit, left, right, SketchMethod.streaming)
    _same_sketch(Psi, Psi_e)
    _same_sketch(Om, Om_e)
    # a rank slice of seeded DRMs (the blocked sketch): the fused path declines it
    ls = tsa.TensorTrainDRM(lr, OUT_SHAPE, transpose=False, seed=3).slice((1, 2, 1), (3, 6, 4))
    rs = tsa.TensorTrainDRM(rr, OUT_SHAPE, transpose=True, seed=4).slice((2, 1, 3), (6, 8, 8))
    s_op = tsa.stream_sketch(op, ls.rank, tuple(rs.rank[::-1]), left_drm=ls, right_drm=rs)
    s_ex = tsa.stream_sketch(explicit, ls.rank, tuple(rs.rank[::-1]), left_drm=ls, right_drm=rs)
    assert [P.shape for P in s_op.Psi_cores] == [(1, 5, 4), (2, 3, 7), (4, 6, 5), (3, 4, 1)]
    _same_sketch(s_op.Psi_cores, s_ex.Psi_cores)
    _same_sketch(s_op.Omega_mats, s_ex.Omega_mats)
    # orthogonal and hmt: OrthogTTDRM walks the DRM method with the cores it is given one by one
    o_op = tsa.orthogonal_sketch(op, lr, rr, left_drm=left, right_drm=right)
    o_ex = tsa.orthogonal_sketch(explicit, lr, rr, left_drm=left, right_drm=right)
    assert o_op.rank == o_ex.rank and rel(o_op.to_numpy(), o_ex.to_numpy()) < 1e-8
    hr = (4, 7, 4)                                            # an unfolding is orthogonalised: ranks within its rows
    _, hright = _drms(tsa, (3, 3, 3), hr, seed=5)
    h_op = tsa.hmt_sketch(op, hr, drm=hright)
    h_ex = tsa.hmt_sketch(explicit, hr, drm=hright)
    assert h_op.rank == h_ex.rank and rel(h_op.to_numpy(), h_ex.to_numpy()) < 1e-8
    # a sum fans out term by term
    both = general_sketch_device(op + explicit * 0.5, left, right, SketchMethod.streaming)
    _same_sketch(both[0], [1.5 * np.asarray(P) for P in Psi_e])
    with pytest.raises(ValueError, match="can't sketch"):
        tsa.stream_sketch(op, lr, rr, left_drm_type=tsa.DenseGaussianDRM, right_drm_type=tsa.DenseGaussianDRM)


# ---- 4. the fused path
def test_fused_path_of_a_weighted_sum(tsa):
    from tt_sketch_amd import OperatorProduct, TensorSum, _native as nat
    from tt_sketch_amd.device import DevArray
    from tt_sketch_amd.tt_gmres import MPO
    d = 4
    pairs = [_product(tsa, 10 + p, op_rank=3, tt_rank=(17, 17, 17)) for p in range(3)]
    plain = tsa.TensorTrain(orc.random_tt(OUT_SHAPE, (5, 9, 2), np.random.default_rng(5)))
    weights = [0.5, -2.0, 1.5, 3.0]
    lr, rr = (4, 4, 4), (6, 6, 6)
    left, right = _drms(tsa, lr, rr, seed=2)
    explicit = TensorSum([mpo(x) for mpo, x in pairs] + [plain]) * weights
    assert max(t.rank[1] for t in explicit.tensors) == 51
    biggest = max(int(np.prod(c.shape)) for t in explicit.tensors for c in t.cores)       # 51 x 6 x 51
    want = tsa.stream_sketch(explicit, lr, rr, left_drm=left, right_drm=right)

    lazy = TensorSum([OperatorProduct(mpo, x) for mpo, x in pairs] + [plain]) * weights
    assert [type(t).__name__ for t in lazy.tensors] == ["OperatorProduct"] * 3 + ["TensorTrain"]
    calls, sizes, entered = [], [], []
    real_call, real_empty, real_mpo = nat.call, DevArray.__dict__["empty"], MPO.__call__
    try:
        nat.call = lambda name, *args: (calls.append(name), real_call(name, *args))[1]
        DevArray.empty = classmethod(lambda cls, shape, *a, **k: (sizes.append(int(np.prod(shape))), real_empty.__func__(cls, shape, *a, **k))[1])
        MPO.__call__ = lambda self, other: (entered.append(1), real_mpo(self, other))[1]
        got = tsa.stream_sketch(lazy, lr, rr, left_drm=left, right_drm=right)
    finally:
        nat.call, DevArray.empty, MPO.__call__ = real_call, real_empty, real_mpo
    assert calls.count("ttsk_op_apply") == 2 * (d - 1)        # d - 1 per side, whatever the number of terms
    assert calls.count("ttsk_gemm") == 4 * (d - 1) + 1        # a chain step per side, Psi and Omega per bond, the last Psi
    assert not entered                                        # no product is formed
    assert sizes and max(sizes) < biggest / 2, (max(sizes), biggest)
    _same_sketch(got.Psi_cores, want.Psi_cores)
    _same_sketch(got.Omega_mats, want.Omega_mats)
    assert rel(got.to_tt().to_numpy(), want.to_tt().to_numpy()) < 1e-8
    # one product alone takes the same path (its W from the kernel or composed, as the routing rule has it)
    try:
        MPO.__call__ = lambda self, other: (entered.append(1), real_mpo(self, other))[1]
        one = tsa.stream_sketch(lazy.tensors[0], lr, rr, left_drm=left, right_drm=right)
    finally:
        MPO.__call__ = real_mpo
    assert not entered
    _same_sketch(one.Psi_cores, tsa.stream_sketch(explicit.tensors[0], lr, rr, left_drm=left, right_drm=right).Psi_cores)


# ---- 5. TT-GMRES on products that are never formed
def _gmres_problem(tsa):
    from tt_sketch_amd.tt_gmres import MPO, TTLinearMapSum, TTPrecond
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gmres_case.npz"))
    shape = tuple(int(n) for n in z["shape"])
    d = len(shape)
    maps = [[z[f"map{m}_core{k}"] for k in range(d)] for m in range(3)]
    b = tsa.TensorTrain([z[f"b_core{k}"] for k in range(d)])
    return z, shape, b, TTLinearMapSum([MPO(list(cores)) for cores in maps]), TTPrecond(z["precond"], shape, mode=1)


@pytest.fixture(scope="module")
def dense_solution(tsa):
    z, shape, b, A, pre = _gmres_problem(tsa)
    N = int(np.prod(shape))
    dense = sum(np.einsum("aibjckdl->abcdijkl", m.to_numpy()).reshape(N, N) for m in A.linear_maps)
    return np.linalg.solve(dense.T, b.to_numpy().ravel()).reshape(shape)


def test_operator_cores_are_uploaded_once_per_mpo(tsa):
    """An MPO of host cores (what MPO.random, MPO.eye and the fixtures give) becomes resident once: the products made of
    it at every Krylov step share its device cores, with and without the preconditioner."""
    from tt_sketch_amd.device import DevArray
    from tt_sketch_amd.tt_gmres import tt_sum_gmres
    z, shape, b, A, pre = _gmres_problem(tsa)
    d = len(shape)
    mpo = A.linear_maps[1]
    assert not mpo.resident()
    p1, p2 = mpo.lazy(b), mpo.lazy(b * 2.0)
    assert all(x is y for x, y in zip(p1.dev_parts()[0], p2.dev_parts()[0])) and mpo.resident()
    assert all(x is y for x, y in zip(p1.dev_parts()[0], mpo.dev_cores()))            # contiguous cores: the eager path's too
    assert all(x.buf is y.buf for x, y in zip(p1.T.dev_parts()[0], mpo.dev_views()[::-1]))
    uploads, real = [], DevArray.__dict__["from_host"]
    try:
        DevArray.from_host = classmethod(lambda cls, arr, *a, **k: (uploads.append(np.ndim(arr)), real.__func__(cls, arr, *a, **k))[1])
        for precond in (None, pre):
            tt_sum_gmres(A, b, max_rank=30, precond=precond, tolerance=1e-9, maxiter=6, rounding_method="sketch", lazy_products=True)
    finally:
        DevArray.from_host = real
    assert uploads.count(4) == 2 * d                          # the cores of the two maps not resident yet, once each
    assert all(m.resident() for m in A.linear_maps)


@pytest.mark.parametrize("method", ["sketch", "orth_sketch"])
def test_gmres_with_lazy_products(tsa, dense_solution, method):
    from tt_sketch_amd.tt_gmres import MPO, tt_sum_gmres
    z, shape, b, A, pre = _gmres_problem(tsa)
    entered, real_mpo = [], MPO.__call__
    try:
        MPO.__call__ = lambda self, other: (entered.append(1), real_mpo(self, other))[1]
        x, hist = tt_sum_gmres(A, b, max_rank=30, tolerance=1e-9, maxiter=25, rounding_method=method, lazy_products=True)
        xp, hp = tt_sum_gmres(A, b, max_rank=30, precond=pre, tolerance=1e-9, maxiter=25, rounding_method=method, lazy_products=True)
    finally:
        MPO.__call__ = real_mpo
    assert not entered
    assert np.allclose(hist["residual_norm"], z[method + "_full_residual_norm"], rtol=1e-4)
    assert np.array_equal(np.array(hist["rank"]), z[method + "_full_rank"])
    assert rel(x.to_numpy(), z[method + "_full_x"]) < 1e-7
    assert rel(x.to_numpy(), dense_solution) < 10 * hist["residual_norm"][-1]
    assert rel(xp.to_numpy(), dense_solution) < 10 * hp["residual_norm"][-1]
