"""Entrywise products of two tensor trains that are never formed, on the device: ``ttsk_hadamard_apply``
(csrc/hadamard_apply.hip) entry by entry, ``hadamard_apply`` on both routes, ``HadamardProduct`` through the generic sketch
driver and through the fused path of ``hadamard_fused``, in sums, and ``hadamard_round``.

Bar of the entry (tests/hadamard_ref.py): |W - W_ref| <= 2 (r + R + 2) 2^-53 W_abs entry by entry, the same bits on a
second call, nothing written outside the call's column block.  Bars of the sketches: Psi / Omega
within 1e-12 ||ref||_F of the same call on the explicit product, the results as tensors within 1e-8.
"""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import ttsk_oracle as orc
from tests import hadamard_ref as ref
from tests.edge_kit import rel_fro as rel, tsa  # noqa: F401

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ("kernel", "composed")


def _upload(a):
    """the host array as a device view of the same strides: a view is uploaded as its contiguous base"""
    from tt_sketch_amd.device import DevArray
    if a.flags.c_contiguous:
        return DevArray.from_host(a)
    base = a.base
    assert base is not None and base.flags.c_contiguous
    off = (a.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // 8
    return DevArray(DevArray.from_host(base).buf, off, a.shape, tuple(s // 8 for s in a.strides))


def c_hadamard_apply(L, X, Y, w_off, w_cols, dims=None, w_cols_arg=None, w_off_arg=None, null=()):
    """One direct call of the C entry on host arrays into a W pre-filled with NaN: (status, W).  The keyword arguments
    overwrite what the arrays say, for the argument tests."""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    dL, dX, dY = DevArray.from_host(np.ascontiguousarray(L)), _upload(X), _upload(Y)
    R, n, R1 = X.shape
    r, _, r1 = Y.shape
    l = L.shape[2]
    W = DevArray.from_host(np.full((l, n, w_cols), np.nan))
    args = dict(L=ctypes.c_void_p(dL.ptr), X=ctypes.c_void_p(dX.ptr), Y=ctypes.c_void_p(dY.ptr),
                dims=nat.i64_array((R, R1, r, r1, n, l) if dims is None else dims),
                strides=nat.i64_array(tuple(dX.strides) + tuple(dY.strides)), W=ctypes.c_void_p(W.ptr))
    for name in null:
        args[name] = None
    rc = nat.lib().ttsk_hadamard_apply(args["L"], args["X"], args["Y"], args["dims"], args["strides"], args["W"],
                                       w_cols if w_cols_arg is None else w_cols_arg, w_off if w_off_arg is None else w_off_arg, 0)
    nat.call("ttsk_sync", -1)
    return rc, W.get()


@pytest.fixture(scope="module")
def truth():
    """the restatement and its bound per case, computed once"""
    out = {}
    for case in ref.CASES:
        L, X, Y, w_off, w_cols = ref.case_arrays(case)
        out[case.name] = (L, X, Y, w_off, w_cols, ref.w_term(L, X, Y), ref.bound(L, X, Y))
    return out


# ---- 1. the C entry against the restatement at every edge
@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.name)
def test_c_entry_vs_restatement(tsa, truth, case):
    L, X, Y, w_off, w_cols, want, tol = truth[case.name]
    rc, W = c_hadamard_apply(L, X, Y, w_off, w_cols)
    assert rc == 0
    got = W[:, :, w_off:w_off + want.shape[2]]
    assert np.isfinite(got).all()
    miss = np.abs(got - want)
    print(f"{case.name}: max |W - W_ref| / bound = {np.max(miss / np.maximum(tol, 1e-300)):.3f}")
    assert (miss <= tol).all()
    assert W[:, :, :w_off].size + W[:, :, w_off + want.shape[2]:].size == W.shape[0] * W.shape[1] * (case.gap + case.tail)
    assert np.isnan(W[:, :, :w_off]).all() and np.isnan(W[:, :, w_off + want.shape[2]:]).all()     # nothing outside the block
    rc2, W2 = c_hadamard_apply(L, X, Y, w_off, w_cols)
    assert rc2 == 0 and np.array_equal(W, W2, equal_nan=True)          # the same bits on every call


# ---- 2. the ABI
def test_argument_errors_and_refusals_write_nothing(tsa, truth):
    from tt_sketch_amd import _native as nat
    L, X, Y, w_off, w_cols, _, _ = truth[next(c.name for c in ref.CASES if c.name.endswith("_gaps_around"))]
    good = [X.shape[0], X.shape[2], Y.shape[0], Y.shape[2], X.shape[1], L.shape[2]]

    def status(**kw):
        rc, W = c_hadamard_apply(L, X, Y, w_off, w_cols, **kw)
        assert np.isnan(W).all(), kw                          # refused before anything is launched
        return rc

    def with_dim(field, value):
        d = list(good)
        d[field] = value
        return d

    for name in ("L", "X", "Y", "dims", "strides", "W"):
        assert status(null=(name,)) == nat.TTSK_ERR_ARG, name
    assert b"NULL" in nat.lib().ttsk_last_error()
    for field in range(6):
        assert status(dims=with_dim(field, 0)) == nat.TTSK_ERR_ARG, field
        assert status(dims=with_dim(field, -3)) == nat.TTSK_ERR_ARG, field
    assert status(w_cols_arg=0) == nat.TTSK_ERR_ARG and status(w_off_arg=-1) == nat.TTSK_ERR_ARG
    assert status(w_cols_arg=w_off + good[1] * good[3] - 1) == nat.TTSK_ERR_ARG          # the block passes w_cols
    assert b"pass w_cols" in nat.lib().ttsk_last_error()
    assert status(w_off_arg=w_cols - good[1] * good[3] + 1) == nat.TTSK_ERR_ARG
    # refused by arithmetic alone: nothing of that size exists
    for field in range(6):
        assert status(dims=with_dim(field, 2 ** 31)) == UNSUPPORTED, field
    assert b"2^31" in nat.lib().ttsk_last_error()
    assert status(w_cols_arg=2 ** 31) == UNSUPPORTED
    d = with_dim(4, 2 ** 20)
    d[5] = 2 ** 16                                            # 2^20 modes x 2^12 tiles of l
    assert status(dims=d) == UNSUPPORTED and b"workgroups" in nat.lib().ttsk_last_error()


# ---- 3. hadamard_apply on both routes
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", [c.name for c in ref.CASES if c.R == ref.BETA_CHUNK + 1 or c.name.endswith("_gaps_flipped_split")])
def test_hadamard_apply_routes_vs_restatement(tsa, truth, name, route):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    from tt_sketch_amd.hadamard_product import hadamard_apply
    L, X, Y, _, _, want, tol = truth[name]
    calls, real = [], nat.call
    try:
        nat.call = lambda entry, *args: (calls.append(entry), real(entry, *args))[1]
        W = hadamard_apply(DevArray.from_host(L), _upload(X), _upload(Y), route=route)
    finally:
        nat.call = real
    assert calls.count("ttsk_hadamard_apply") == (1 if route == "kernel" else 0)
    assert (calls.count("ttsk_gemm") == 0) == (route == "kernel")
    got = W.get()
    assert got.shape == want.shape
    miss = np.abs(got - want)
    print(f"{name}, {route}: max |W - W_ref| / bound = {np.max(miss / np.maximum(tol, 1e-300)):.3f}")
    assert (miss <= tol).all()


def test_hadamard_apply_checks_its_operands(tsa):
    from tt_sketch_amd.device import DevArray
    from tt_sketch_amd.hadamard_product import hadamard_apply
    L, X, Y = DevArray.zeros((2, 3, 4)), DevArray.zeros((2, 5, 3)), DevArray.zeros((3, 5, 2))
    assert hadamard_apply(L, X, Y, route="kernel").shape == (4, 5, 6)
    with pytest.raises(ValueError, match="mode size"):
        hadamard_apply(L, X, DevArray.zeros((3, 4, 2)))
    with pytest.raises(ValueError, match="chain"):
        hadamard_apply(DevArray.zeros((3, 2, 4)), X, Y)
    with pytest.raises(ValueError, match="route"):
        hadamard_apply(L, X, Y, route="fastest")


# ---- 4. the generic driver
SHAPE = (5, 7, 4, 6)


def _factors(tsa, seed, x_rank=(3, 6, 2), y_rank=(2, 5, 4)):
    rng = np.random.default_rng(seed)
    return tsa.TensorTrain(orc.random_tt(SHAPE, x_rank, rng)), tsa.TensorTrain(orc.random_tt(SHAPE, y_rank, rng))


def _drms(tsa, left_rank, right_rank, seed=0):
    rng = np.random.default_rng(seed)
    ld, rd = orc.random_tt_drm(SHAPE, left_rank, False, rng), orc.random_tt_drm(SHAPE, right_rank, True, rng)
    return (tsa.TensorTrainDRM(left_rank, SHAPE, transpose=False, cores=ld.cores),
            tsa.TensorTrainDRM(right_rank, SHAPE, transpose=True, cores=rd.cores))


def _same_sketch(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and np.linalg.norm(a - b) <= 1e-12 * np.linalg.norm(b)


def _diagonal_mpo(x):
    from tt_sketch_amd.tt_gmres import MPO
    cores = []
    for C in x.cores:
        C = np.asarray(C)
        M = np.zeros((C.shape[0], C.shape[1], C.shape[1], C.shape[2]))
        for i in range(C.shape[1]):
            M[:, i, i, :] = C[:, i, :]
        cores.append(M)
    return MPO(cores)


@pytest.fixture(scope="module")
def explicit(tsa):
    """the factors, the lazy product, its explicit train and the explicit train's sketches: computed once"""
    from tt_sketch_amd import HadamardProduct, SketchMethod
    from tt_sketch_amd.sketch_dispatch import general_sketch_device
    x, y = _factors(tsa, 1)
    h = HadamardProduct(x, y)
    tt = h.to_tt()
    assert h.rank == tt.rank == (6, 30, 8) and rel(tt.to_numpy(), x.to_numpy() * y.to_numpy()) < 1e-13
    lr, rr, hr = (4, 7, 5), (6, 9, 8), (4, 7, 4)
    left, right = _drms(tsa, lr, rr)
    _, hright = _drms(tsa, (3, 3, 3), hr, seed=5)
    Psi, Om = general_sketch_device(tt, left, right, SketchMethod.streaming)
    return dict(x=x, y=y, h=h, tt=tt, lr=lr, rr=rr, hr=hr, left=left, right=right, hright=hright,
                Psi=[P.get() for P in Psi], Om=[O.get() for O in Om],
                orth=tsa.orthogonal_sketch(tt, lr, rr, left_drm=left, right_drm=right).to_numpy(),
                hmt=tsa.hmt_sketch(tt, hr, drm=hright).to_numpy())


def test_to_tt_on_resident_cores(tsa, explicit):
    from tt_sketch_amd import HadamardProduct
    x, y, tt = explicit["x"], explicit["y"], explicit["tt"]
    resident = HadamardProduct(x.to_device(), y.to_device()).to_tt()
    assert resident.resident() and resident.rank == tt.rank
    for a, b in zip(resident.cores, tt.cores):
        assert np.array_equal(a.get(), np.asarray(b))                 # single products: the same bits as NumPy's
    half = HadamardProduct(x.to_device(), y).to_tt()                  # one resident factor is enough
    assert half.resident() and rel(half.to_numpy(), tt.to_numpy()) < 1e-15
    flipped = HadamardProduct(x.to_device(), y.to_device()).T.to_tt()
    assert rel(flipped.to_numpy(), tt.to_numpy().transpose(3, 2, 1, 0)) < 1e-15


@pytest.mark.parametrize("route", ROUTES)
def test_generic_driver_against_the_explicit_product(tsa, explicit, route):
    from tt_sketch_amd import OperatorProduct, SketchMethod, paths
    from tt_sketch_amd.sketch_dispatch import general_sketch_device
    e = explicit
    h, left, right = e["h"], e["left"], e["right"]
    with paths.forced(route):
        # streaming, through general_sketch_device: the plug-in tables, not the fused path
        Psi, Om = general_sketch_device(h, left, right, SketchMethod.streaming)
        _same_sketch(Psi, e["Psi"])
        _same_sketch(Om, e["Om"])
        # orthogonal and hmt: OrthogTTDRM walks the DRM method with the cores it is given one by one
        o = tsa.orthogonal_sketch(h, e["lr"], e["rr"], left_drm=left, right_drm=right)
        assert rel(o.to_numpy(), e["orth"]) < 1e-8
        m = tsa.hmt_sketch(h, e["hr"], drm=e["hright"])
        assert rel(m.to_numpy(), e["hmt"]) < 1e-8
    # x outer is the layout of the diagonal operator of x applied to y: the same sketch, bond by bond
    op = OperatorProduct(_diagonal_mpo(e["x"]), e["y"])
    Psi_op, Om_op = general_sketch_device(op, left, right, SketchMethod.streaming)
    _same_sketch(Psi, Psi_op)
    _same_sketch(Om, Om_op)
    with pytest.raises(ValueError, match="can't sketch"):
        tsa.stream_sketch(h, e["lr"], e["rr"], left_drm_type=tsa.DenseGaussianDRM, right_drm_type=tsa.DenseGaussianDRM)


def test_rank_slices_go_through_the_generic_driver(tsa, explicit):
    e = explicit
    ls = tsa.TensorTrainDRM(e["lr"], SHAPE, transpose=False, seed=3).slice((1, 2, 1), (3, 6, 4))
    rs = tsa.TensorTrainDRM(e["rr"], SHAPE, transpose=True, seed=4).slice((2, 1, 3), (6, 8, 8))
    s_h = tsa.stream_sketch(e["h"], ls.rank, tuple(rs.rank[::-1]), left_drm=ls, right_drm=rs)
    s_ex = tsa.stream_sketch(e["tt"], ls.rank, tuple(rs.rank[::-1]), left_drm=ls, right_drm=rs)
    assert [P.shape for P in s_h.Psi_cores] == [(1, 5, 4), (2, 7, 7), (4, 4, 5), (3, 6, 1)]
    _same_sketch(s_h.Psi_cores, s_ex.Psi_cores)
    _same_sketch(s_h.Omega_mats, s_ex.Omega_mats)


# ---- 5. the fused path
@pytest.mark.parametrize("route", ROUTES + (None,))
def test_fused_path_of_a_single_product(tsa, explicit, route):
    from tt_sketch_amd import SketchMethod, hadamard_fused, paths
    from tt_sketch_amd.sketch_dispatch import general_sketch_device
    e = explicit
    h, left, right, d = e["h"], e["left"], e["right"], len(SHAPE)
    applies, formed, real_apply, real_to_tt = [], [], hadamard_fused.hadamard_apply, type(h).to_tt
    try:
        hadamard_fused.hadamard_apply = lambda L, X, Y, **kw: (applies.append(kw.get("route")), real_apply(L, X, Y, **kw))[1]
        type(h).to_tt = lambda self: (formed.append(1), real_to_tt(self))[1]
        with paths.forced(route):
            got = tsa.stream_sketch(h, e["lr"], e["rr"], left_drm=left, right_drm=right)
    finally:
        hadamard_fused.hadamard_apply, type(h).to_tt = real_apply, real_to_tt
    assert len(applies) == 2 * (d - 1) and not formed         # two applies per mode, no product formed
    _same_sketch(got.Psi_cores, e["Psi"])
    _same_sketch(got.Omega_mats, e["Om"])
    with paths.forced(route):
        Psi, Om = general_sketch_device(h, left, right, SketchMethod.streaming)
    _same_sketch(got.Psi_cores, [P.get() for P in Psi])       # equals the generic driver
    _same_sketch(got.Omega_mats, [O.get() for O in Om])
    assert rel(got.to_tt().to_numpy(), tsa.stream_sketch(e["tt"], e["lr"], e["rr"], left_drm=left, right_drm=right).to_tt().to_numpy()) < 1e-8


def test_fused_path_declines_what_is_not_its_own(tsa, explicit):
    from tt_sketch_amd import SketchMethod, TensorSum
    from tt_sketch_amd.hadamard_fused import try_hadamard_sketch
    e = explicit
    h, left, right = e["h"], e["left"], e["right"]
    assert try_hadamard_sketch(h, left, right, SketchMethod.streaming, route="kernel") is not None
    assert try_hadamard_sketch(TensorSum([h, h]), left, right, SketchMethod.streaming) is None
    assert try_hadamard_sketch(e["tt"], left, right, SketchMethod.streaming) is None
    assert try_hadamard_sketch(h, left, right, SketchMethod.orthogonal) is None
    assert try_hadamard_sketch(h, None, right, SketchMethod.hmt) is None
    ls = tsa.TensorTrainDRM(e["lr"], SHAPE, transpose=False, seed=3).slice((1, 2, 1), (3, 6, 4))
    rs = tsa.TensorTrainDRM(e["rr"], SHAPE, transpose=True, seed=4)
    assert try_hadamard_sketch(h, ls, rs, SketchMethod.streaming) is None
    assert try_hadamard_sketch(h, tsa.TensorTrainDRM(e["lr"], SHAPE, transpose=False, seed=3), rs, SketchMethod.streaming) is not None


def test_blocked_sketch_agrees_with_the_unblocked_one(tsa, explicit):
    e = explicit
    left = tsa.TensorTrainDRM(e["lr"], SHAPE, transpose=False, seed=8)
    right = tsa.TensorTrainDRM(e["rr"], SHAPE, transpose=True, seed=9)
    whole = tsa.stream_sketch(e["h"], e["lr"], e["rr"], left_drm=left, right_drm=right)
    blocked = tsa.blocked_stream_sketch(e["h"], left, right, [(0, 0, 0), (2, 3, 2), e["lr"]], [(0, 0, 0), (3, 4, 5), e["rr"]])
    _same_sketch(blocked.Psi_cores, whole.Psi_cores)
    _same_sketch(blocked.Omega_mats, whole.Omega_mats)


# ---- 6. sums and rounding
def test_sum_with_a_train_and_a_weighted_product(tsa, explicit):
    from tt_sketch_amd import HadamardProduct, TensorSum
    e = explicit
    u, v = _factors(tsa, 2, x_rank=(2, 2, 3), y_rank=(3, 4, 2))
    plain = tsa.TensorTrain(orc.random_tt(SHAPE, (5, 9, 2), np.random.default_rng(5)))
    weighted = HadamardProduct(u, v) * -1.5
    assert type(weighted) is HadamardProduct
    lazy = TensorSum([e["h"], plain, weighted])
    formed = TensorSum([e["tt"], plain, weighted.to_tt()])
    left, right = e["left"], e["right"]
    got = tsa.stream_sketch(lazy, e["lr"], e["rr"], left_drm=left, right_drm=right)
    want = tsa.stream_sketch(formed, e["lr"], e["rr"], left_drm=left, right_drm=right)
    _same_sketch(got.Psi_cores, want.Psi_cores)
    _same_sketch(got.Omega_mats, want.Omega_mats)
    dense = e["x"].to_numpy() * e["y"].to_numpy() + plain.to_numpy() - 1.5 * u.to_numpy() * v.to_numpy()
    assert rel(lazy.to_numpy(), dense) < 1e-13


@pytest.mark.parametrize("max_rank", [9, 12])
@pytest.mark.parametrize("method", ["sketch", "orth_sketch", "exact"])
def test_hadamard_round_recovers_a_square(tsa, method, max_rank):
    x = tsa.TensorTrain(orc.random_tt((6, 7, 5, 6), 3, np.random.default_rng(11)))
    sq = tsa.hadamard_round(x, x, max_rank, method=method)
    assert type(sq) is tsa.TensorTrain and max(sq.rank) <= max_rank
    assert rel(sq.to_numpy(), x.to_numpy() ** 2) < 1e-8


# ---- 7. the routing rule
def _recorded():
    path = os.path.join(ROOT, "profiles", "hadamard_sketch_bench.json")
    with open(path) as f:
        return json.load(f)


def test_routing_rule_against_the_recorded_verdicts(tsa):
    """Only the rule is evaluated: at every kernel-alone shape of profiles/hadamard_sketch_bench.json where the two measured
    ranges are apart, it names the faster route."""
    from tt_sketch_amd import hadamard_product as hp
    rows = _recorded()["kernel_alone"]
    assert len(rows) >= 4
    decided = 0
    for row in rows:
        k, c = row["kernel_ms"], row["composed_ms"]                    # each [median, min, max]
        kernel_ms, composed_ms = hp.route_ms(row["R"], row["R1"], row["r"], row["r1"], row["n"], row["l"])
        named = "composed" if composed_ms < kernel_ms else "kernel"
        print(f"R {row['R']} r {row['r']} n {row['n']} l {row['l']}: kernel {k}, composed {c}; the rule expects {kernel_ms:.3f} / {composed_ms:.3f} ms -> {named}")
        if k[2] < c[1]:
            decided += 1
            assert named == "kernel"
        elif c[2] < k[1]:
            decided += 1
            assert named == "composed"
    assert decided >= 1


@pytest.mark.parametrize("dims", [(4, 4, 3, 3, 5, 6), (32, 32, 32, 32, 40, 50)], ids=["small", "large"])
def test_unforced_calls_take_the_route_the_rule_names(tsa, dims):
    from tt_sketch_amd import _native as nat, hadamard_product as hp
    from tt_sketch_amd.device import DevArray
    R, R1, r, r1, n, l = dims
    rng = np.random.default_rng(3)
    L, X, Y = rng.standard_normal((R, r, l)), rng.standard_normal((R, n, R1)), rng.standard_normal((r, n, r1))
    kernel_ms, composed_ms = hp.route_ms(*dims)
    named = "composed" if composed_ms < kernel_ms else "kernel"
    calls, real = [], nat.call
    try:
        nat.call = lambda entry, *args: (calls.append(entry), real(entry, *args))[1]
        W = hp.hadamard_apply(DevArray.from_host(L), DevArray.from_host(X), DevArray.from_host(Y))
    finally:
        nat.call = real
    assert calls.count("ttsk_hadamard_apply") == (1 if named == "kernel" else 0)
    assert (np.abs(W.get() - ref.w_term(L, X, Y)) <= ref.bound(L, X, Y)).all()
