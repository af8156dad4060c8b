"""Tucker tensors on the device: ``ttsk_tucker_gather`` (csrc/tucker_gather.hip) at every edge of its plan, and the Python
surface built on it and on ``tensor_tucker`` (``gather``, ``gather_dev``, ``support_error``, ``SparseTensor.dot``, ``dot`` /
``norm`` / ``error(fast=True)`` against Tucker, TT and CP partners).

Bars (tests/tucker_ref.py, derived there and held against np.longdouble by tests/test_tucker_gather_host.py): an entry
within 2 (prod s_k + d) 2^-53 T_abs of the long-double truth, the three sums within the propagated bar, the inner products
within 2 L 2^-53 of their chain on absolute values.  Small-integer data must come out exactly.
"""
import ctypes

import numpy as np
import pytest

from tests import tucker_ref as tr
from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

ARG, UNSUPPORTED = -2, -3
GUARD = 16
SENTINEL = -123.25


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ptr)


def c_gather(factors, core, shape, idx, val=None, want_out=True, want_stats=False, reverse_rows=False, pad=0, ranks=None):
    """One direct call of the C entry: (status, t (N,) or None, sums (3,) or None).  The outputs are NaN-filled and lie
    between guard bands, which must come back untouched; ``reverse_rows``: the index matrix is stored with its rows in
    reverse order and addressed through ``row_order``; ``pad``: row stride N + pad, the padding holds -7."""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    d, N = len(shape), idx.shape[1]
    phys = np.full((d, N + pad), -7, dtype=np.int64)
    order = list(range(d))[::-1] if reverse_rows else list(range(d))
    for k in range(d):
        phys[order[k], :N] = idx[k]
    dev_idx = DevArray.from_host(phys, dtype=np.int64)
    dev_f = [DevArray.from_host(np.ascontiguousarray(U, dtype=np.float64)) for U in factors]
    dev_c = DevArray.from_host(np.ascontiguousarray(core, dtype=np.float64))
    dev_val = DevArray.from_host(np.asarray(val, dtype=np.float64)) if val is not None else None

    def banded(n):
        host = np.full(n + 2 * GUARD, SENTINEL)
        host[GUARD:GUARD + n] = np.nan
        return DevArray.from_host(host)

    out_b = banded(N) if want_out else None
    stats_b = banded(3) if want_stats else None
    out = out_b[GUARD:GUARD + N] if want_out else None
    stats = stats_b[GUARD:GUARD + 3] if want_stats else None
    ranks = [U.shape[0] for U in factors] if ranks is None else ranks
    rc = nat.lib().ttsk_tucker_gather(_ptr(dev_c), (ctypes.c_void_p * d)(*[f.ptr for f in dev_f]), (ctypes.c_int64 * d)(*ranks),
                                      (ctypes.c_int64 * d)(*shape), d, _ptr(dev_idx), N + pad, (ctypes.c_int * d)(*order),
                                      ctypes.c_size_t(N), _ptr(dev_val), _ptr(out), _ptr(stats), 0)
    nat.call("ttsk_sync", -1)
    got = []
    for band, n in ((out_b, N), (stats_b, 3)):
        if band is None:
            got.append(None)
            continue
        host = band.get()
        assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all(), "a guard band was written"
        if rc != 0:
            assert np.isnan(host[GUARD:GUARD + n]).all(), "a refused call wrote its output"
        got.append(host[GUARD:GUARD + n] if rc == 0 else None)
    return rc, got[0], got[1]


def check_entries(t, factors, core, idx, what):
    truth = tr.gather(factors, core, idx, dtype=np.longdouble)
    bar = tr.entry_bar(factors, core, idx)
    worst = float(np.max(np.abs(t - truth) / np.maximum(bar, 1e-300), initial=0.0))
    print(f"{what}: max |t - truth| / bar = {worst:.3f}")
    assert np.isfinite(t).all(), what
    assert (np.abs(t - truth) <= bar).all(), (what, worst)
    return truth, bar


def check_sums(s, truth, val, bar, what):
    want = tr.stats(truth, val.astype(np.longdouble))
    tol = tr.stats_bar(truth, val, bar)
    print(f"{what}: sums off by {np.abs(s - want) / np.maximum(tol, 1e-300)} of their bars")
    assert (np.abs(s - want) <= tol).all(), (what, s, want)


# ---- 1. the C entry at every edge of the plan
@pytest.mark.parametrize("case", tr.CASES, ids=lambda c: c[0])
def test_c_entry_at_every_edge(tsa, case):
    tag, ranks, shape, N, rev, pad = case
    # small integers: float64 is exact, every entry equals the integer formula
    fi, ci, ii, vi = tr.case_data(tag, ranks, shape, N, integer=True)
    rc, t, s = c_gather(fi, ci, shape, ii, np.round(vi), True, True, rev, pad)
    assert rc == 0
    want = tr.gather(fi, ci, ii)
    assert (want == np.round(want)).all()
    assert (t == want).all(), (tag, np.flatnonzero(t != want)[:10])
    assert (s == tr.stats(want, np.round(vi))).all()                    # integers below 2^53: any order gives the same sums
    # normal data against the long-double truth
    factors, core, idx, val = tr.case_data(tag, ranks, shape, N)
    rc, t, s = c_gather(factors, core, shape, idx, val, True, True, rev, pad)
    assert rc == 0
    truth, bar = check_entries(t, factors, core, idx, tag)
    check_sums(s, truth, val, bar, tag)
    # the calling conventions: the same bits with dev_out only, dev_stats only, both, and on a second call
    rc1, t1, _ = c_gather(factors, core, shape, idx, None, True, False, rev, pad)
    rc2, _, s2 = c_gather(factors, core, shape, idx, val, False, True, not rev, 0)
    rc3, t3, s3 = c_gather(factors, core, shape, idx, val, True, True, rev, pad)
    assert rc1 == rc2 == rc3 == 0
    assert t.tobytes() == t1.tobytes() == t3.tobytes()
    assert s.tobytes() == s2.tobytes() == s3.tobytes()


def test_empty_list(tsa):
    factors, core, idx, val = tr.case_data("empty", (3, 4), (5, 6), 8)
    rc, t, s = c_gather(factors, core, (5, 6), idx[:, :0], val[:0], True, True)
    assert rc == 0 and t.shape == (0,) and (s == 0).all()


def test_refusals_leave_the_outputs_untouched(tsa):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    # d = 9
    ranks, shape = (2,) * 9, (3,) * 9
    factors, core, idx, val = tr.case_data("d9", ranks, shape, 20)
    assert c_gather(factors, core, shape, idx, val, True, True)[0] == UNSUPPORTED
    assert b"9 modes" in nat.lib().ttsk_last_error()
    # a core beyond the cover: the ranks announce 2^21 entries (nothing is read before the refusal)
    factors, core, idx, val = tr.case_data("big", (2, 2), (3, 3), 20)
    assert c_gather(factors, core, (3, 3), idx, val, True, True, ranks=[2 ** 11, 2 ** 10])[0] == UNSUPPORTED
    assert b"2^20" in nat.lib().ttsk_last_error()
    assert c_gather(factors, core, (2 ** 31, 3), idx, val, True, True)[0] == UNSUPPORTED
    # the argument errors of ttsk_tt_gather
    assert c_gather(factors, core, (3, 3), idx, val, False, False)[0] == ARG                  # no output at all
    assert c_gather(factors, core, (3, 3), idx, None, True, True)[0] == ARG                    # sums without entries
    assert c_gather(factors, core, (3, 3), idx, None, False, True)[0] == ARG
    assert c_gather(factors, core, (3, 3), idx, val, True, True, ranks=[2, 0])[0] == ARG
    one = DevArray.from_host(np.full(8, np.nan))
    z = (ctypes.c_int64 * 1)(1)
    fac = (ctypes.c_void_p * 1)(one.ptr)
    lib = nat.lib()
    args = lambda core, f, rk, sh, d, ix: (core, f, rk, sh, d, ix, 8, None, ctypes.c_size_t(1), None, _ptr(one), None, 0)
    assert lib.ttsk_tucker_gather(*args(None, fac, z, z, 1, _ptr(one))) == ARG
    assert lib.ttsk_tucker_gather(*args(_ptr(one), None, z, z, 1, _ptr(one))) == ARG
    assert lib.ttsk_tucker_gather(*args(_ptr(one), fac, None, z, 1, _ptr(one))) == ARG
    assert lib.ttsk_tucker_gather(*args(_ptr(one), fac, z, None, 1, _ptr(one))) == ARG
    assert lib.ttsk_tucker_gather(*args(_ptr(one), fac, z, z, 0, _ptr(one))) == ARG
    assert lib.ttsk_tucker_gather(*args(_ptr(one), fac, z, z, 1, None)) == ARG
    assert lib.ttsk_tucker_gather(*args(_ptr(one), (ctypes.c_void_p * 1)(None), z, z, 1, _ptr(one))) == ARG
    nat.call("ttsk_sync", -1)
    assert np.isnan(one.get()).all()


# ---- 2. the Python surface
def _surface_cases():
    out = [(c["name"], c["factors"], c["core"], c["idx"], c["entries"], c) for c in tr.load_cases()]
    factors, core, idx, val = tr.case_data("surface", (16, 17, 5), (40, 40, 40), 5000)
    out.append(("d3_n40", factors, core, idx, val, None))
    return out


def _resident(tsa, factors, core):
    from tt_sketch_amd.device import DevArray
    return tsa.TuckerTensor([DevArray.from_host(np.ascontiguousarray(U)) for U in factors], DevArray.from_host(np.ascontiguousarray(core)))


@pytest.mark.parametrize("case", _surface_cases(), ids=lambda c: c[0])
def test_gather_surface_on_both_routes(tsa, case, monkeypatch):
    from tt_sketch_amd import tensor as tmod
    name, factors, core, idx, val, golden = case
    shape = tuple(U.shape[1] for U in factors)
    a = _resident(tsa, factors, core)
    assert a.resident() and a.T.resident() and not tsa.TuckerTensor(factors, core).resident()
    sp = tsa.SparseTensor(shape, idx, val)
    truth = tr.gather(factors, core, idx, dtype=np.longdouble)
    bar = tr.entry_bar(factors, core, idx)
    want, tol = tr.stats(truth, val.astype(np.longdouble)), tr.stats_bar(truth, val, bar)

    def closed(x):
        raise AssertionError("host detour: tensor._host was called")

    monkeypatch.setattr(tmod, "_host", closed)
    for route in ("kernel", "composed"):
        for t, i, s in ((a, idx, sp), (a.T, idx[::-1], sp.T)):
            for got in (t.gather(i, route=route), t.gather_dev(tuple(i), route=route).get(), t.gather(s, route=route)):
                assert got.shape == (idx.shape[1],) and got.dtype == np.float64
                assert (np.abs(got - truth) <= bar).all(), (name, route)
            err = t.support_error(s, route=route)
            assert abs(err ** 2 - want[2]) <= tol[2] + 4 * tr.U53 * float(want[2]), (name, route)
            rel = t.support_error(s, relative=True, route=route)
            assert abs(rel - err / np.linalg.norm(val)) <= 4 * tr.U53 * rel
            dot = s.dot(t, route=route)
            assert dot == t.dot(s, route=route)
            assert abs(dot - want[0]) <= tol[0], (name, route)
    # a host tensor with an uploaded SparseTensor takes the device path too
    monkeypatch.undo()
    host = tsa.TuckerTensor(factors, core)
    assert abs(sp.dot(host) - want[0]) <= tol[0] and host._dev is not None
    if golden is not None:
        assert (np.abs(a.gather(idx) - golden["gather"]) <= 2 * bar).all()
        # the reference sums the dense array: its own rounding is within 1e-12 of the sum of the |terms| (depth prod n_k
        # + prod s_k + d < 3000 for the fixtures, 2 x 3000 x 2^-53 < 1e-12)
        assert abs(sp.dot(a) - golden["dot_sparse"]) <= tol[0] + 1e-12 * float(np.abs(truth) @ np.abs(val))


@pytest.mark.parametrize("case", tr.load_cases(), ids=lambda c: c["name"])
def test_inner_products_against_restatement_and_reference(tsa, case, monkeypatch):
    from tt_sketch_amd import tensor as tmod
    from tt_sketch_amd.device import DevArray
    f, c, fb, cb, cores, cp = case["factors"], case["core"], case["factors_b"], case["core_b"], case["cores"], case["cp"]
    ld = np.longdouble
    a, b = _resident(tsa, f, c), _resident(tsa, fb, cb)
    tt = tsa.TensorTrain([DevArray.from_host(g) for g in cores])
    cpt = tsa.CPTensor([DevArray.from_host(g) for g in cp])

    def closed(x):
        raise AssertionError("host detour: tensor._host was called")

    monkeypatch.setattr(tmod, "_host", closed)
    # (value, (long-double truth, bar, sum of the |terms|), the reference's value).  The reference evaluates on dense
    # arrays: its own rounding is within 1e-12 of the sum of the |terms| (depth prod n_k + prod s_k + d < 3000 for the
    # fixtures, 2 x 3000 x 2^-53 < 1e-12)
    def tri(fn, bar_fn, *args):
        return fn(*args, dtype=ld), bar_fn(*args), float(fn(*args, absolute=True))

    aa, bb = tri(tr.tucker_dot, tr.tucker_dot_bar, f, c, f, c), tri(tr.tucker_dot, tr.tucker_dot_bar, fb, cb, fb, cb)
    ab = tri(tr.tucker_dot, tr.tucker_dot_bar, f, c, fb, cb)
    at = tri(tr.tucker_tt_dot, tr.tucker_tt_dot_bar, f, c, cores)
    ac = tri(tr.tucker_cp_dot, tr.tucker_cp_dot_bar, f, c, cp)
    rows = [
        ("norm^2", a.norm() ** 2, aa, case["norm"] ** 2), ("norm_b^2", b.norm() ** 2, bb, case["norm_b"] ** 2),
        ("a.b", a.dot(b), ab, case["dot_tucker"]), ("b.a", b.dot(a), ab, case["dot_tucker"]),
        ("a.T.b.T", a.T.dot(b.T), ab, case["dot_tucker"]),
        ("a.tt", a.dot(tt), at, case["dot_tt"]), ("tt.a", tt.dot(a), at, case["dot_tt_rev"]), ("a.T.tt.T", a.T.dot(tt.T), at, case["dot_tt"]),
        ("a.cp", a.dot(cpt), ac, case["dot_cp"]), ("cp.a", cpt.dot(a), ac, case["dot_cp_rev"]), ("a.T.cp.T", a.T.dot(cpt.T), ac, case["dot_cp"]),
    ]
    for what, got, (truth, bar, scale), ref in rows:
        bar = bar + 4 * tr.U53 * abs(float(truth))          # the square of a rounded root
        print(f"{case['name']} {what}: off by {float(abs(got - truth) / bar):.3f} of the bar")
        assert abs(got - truth) <= bar, what
        assert abs(got - ref) <= bar + 1e-12 * scale, what
    # fast errors: the reference's formula on device norms and dots
    for x, y, key in ((tt, a, "error_tt"), (cpt, a, "error_cp"), (b, a, "error_tucker"), (a, tt, "error_self_tt")):
        got = x.error(y, fast=True, relative=True)
        assert abs(got - case[key]) <= 1e-9 * case[key], key
    # a TensorSum with a Tucker term, and the recursion of Tensor.dot through `reverse`
    total = a + tt
    assert abs(total.dot(b) - (rows[2][1] + b.dot(tt))) <= 4 * tr.U53 * (abs(rows[2][1]) + abs(b.dot(tt)))
    assert abs(b.dot(total) - total.dot(b)) <= 4 * tr.U53 * (abs(rows[2][1]) + abs(b.dot(tt)))
    want = rows[0][1] + 2 * rows[5][1] + tt.norm() ** 2
    assert abs(total.norm() ** 2 - want) <= 1e-12 * (rows[0][1] + 2 * abs(rows[5][1]) + tt.norm() ** 2)
    # a host partner of a resident tensor is uploaded and takes the same path; two host objects stay on the host
    monkeypatch.undo()
    host_b = tsa.TuckerTensor(fb, cb)
    assert a.dot(host_b) == rows[2][1] and host_b._dev is not None
    h1, h2 = tsa.TuckerTensor(f, c), tsa.TuckerTensor(fb, cb)
    assert abs(h1.dot(h2) - case["dot_tucker"]) <= 1e-12 * float(tr.tucker_dot(f, c, fb, cb, absolute=True))
    assert h1._dev is None and h2._dev is None


def test_sketched_train_is_checked_against_the_tucker_tensor(tsa):
    factors, core, idx, val = tr.case_data("surface", (16, 17, 5), (40, 40, 40), 5000)
    a = _resident(tsa, factors, core)
    tt = tsa.stream_sketch(a, (20, 9), (26, 14), seed=11).to_tt()
    assert tt.resident()
    err = tt.error(a, fast=True, relative=True)
    print(f"stream_sketch(tucker).to_tt(): fast relative error {err:.2e}")
    assert err < 1e-7


def test_forced_unsupported_reaches_the_composed_fallback(tsa):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd import paths
    from tt_sketch_amd import tensor_gather as tmod
    ranks, shape, N = (2,) * 9, (3, 2, 3, 2, 3, 2, 3, 2, 3), 3000
    factors, core, idx, val = tr.case_data("d9_composed", ranks, shape, N)
    a = _resident(tsa, factors, core)
    sp = tsa.SparseTensor(shape, idx, val)
    truth, bar = tr.gather(factors, core, idx, dtype=np.longdouble), tr.entry_bar(factors, core, idx)
    with pytest.raises(nat.TtskUnsupported):
        a.gather_dev(idx, route="kernel")
    with paths.forced("kernel"):
        with pytest.raises(nat.TtskUnsupported):
            sp.dot(a)
    old = tmod._PANEL_BYTES
    try:
        tmod._PANEL_BYTES = 16 * 256 * 1000                           # three chunks of the list
        got = a.gather(idx)
        assert (np.abs(got - truth) <= bar).all()
        want, tol = tr.stats(truth, val.astype(np.longdouble)), tr.stats_bar(truth, val, bar)
        assert abs(sp.dot(a) - want[0]) <= tol[0]
        assert abs(a.support_error(sp) ** 2 - want[2]) <= tol[2] + 4 * tr.U53 * float(want[2])
        with paths.forced("composed"):
            assert a.gather(idx).tobytes() == got.tobytes()
    finally:
        tmod._PANEL_BYTES = old


# ---- 3. no dense array
def test_shape_whose_dense_form_cannot_exist(tsa, monkeypatch):
    """d = 6, n = 200: 6.4e13 entries, 512 TB as float64."""
    from tt_sketch_amd import tensor as tmod
    from tt_sketch_amd.device import DevArray
    d, n, r, N = 6, 200, 4, 1000
    rng = np.random.default_rng(66)
    factors = [rng.standard_normal((r, n)) / np.sqrt(n) for _ in range(d)]
    core = rng.standard_normal((r,) * d)
    cores = tr.random_tt(rng, (n,) * d, (3,) * (d - 1))
    idx = np.stack([rng.integers(0, n, N) for _ in range(d)]).astype(np.int64)
    a = _resident(tsa, factors, core)
    tt = tsa.TensorTrain([DevArray.from_host(g) for g in cores])

    def closed(*x, **k):
        raise AssertionError("a dense array was asked for")

    monkeypatch.setattr(tmod, "_host", closed)
    monkeypatch.setattr(tsa.TuckerTensor, "to_numpy", closed)
    monkeypatch.setattr(tsa.TensorTrain, "to_numpy", closed)
    nrm, dot, t = a.norm(), a.dot(tt), a.gather(idx)
    assert np.isfinite(nrm) and np.isfinite(dot) and np.isfinite(t).all()
    ld = np.longdouble
    truth = tr.tucker_dot(factors, core, factors, core, dtype=ld)
    assert abs(nrm ** 2 - truth) <= tr.tucker_dot_bar(factors, core, factors, core) + 4 * tr.U53 * float(truth)
    assert abs(dot - tr.tucker_tt_dot(factors, core, cores, dtype=ld)) <= tr.tucker_tt_dot_bar(factors, core, cores)
    assert (np.abs(t - tr.gather(factors, core, idx, dtype=ld)) <= tr.entry_bar(factors, core, idx)).all()
    assert abs(tt.error(a, fast=True, relative=True) - tr.fast_error(tt.norm(), nrm, dot, True)) <= 1e-12
