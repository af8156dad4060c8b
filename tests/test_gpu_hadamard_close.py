"""Inner products of Hadamard products that are never formed, on the device: ``ttsk_hadamard_close``
(csrc/hadamard_close.hip) entry by entry, ``hadamard_close`` on both routes, and ``HadamardProduct.dot`` / ``norm`` /
``gather`` and ``TensorTrain.error(fast=True)`` on resident trains against dense NumPy.

Bar of the entry (tests/hadamard_close_ref.py): |G' - G'_ref| <= 2 (s + S + n + 3) 2^-53 G'_abs entry by entry, the same bits on
a second call, nothing written past the plan's slab; at n = 1 the floats of ``ttsk_hadamard_apply`` on the same operands
(both kernels run the stages of csrc/hadamard_stages.h).  Bars of the surface: inner products within 1e-12 ||a|| ||b||, the fast
error within 1e-10 of the dense one on tensors at a relative distance of 0.1 or more.
"""
import ctypes
import json
import os

import numpy as np
import pytest

from oracle import ttsk_oracle as orc
from tests import hadamard_close_ref as ref
from tests import hadamard_ref as apply_ref
from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ("kernel", "composed")
PAD = 8                        # doubles past the plan's slab that must stay untouched


def _upload(a):
    """the host array as a device view of the same strides: a view is uploaded as its contiguous base"""
    from tt_sketch_amd.device import DevArray
    if a.flags.c_contiguous:
        return DevArray.from_host(a)
    base = a.base
    assert base is not None and base.flags.c_contiguous
    off = (a.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // 8
    return DevArray(DevArray.from_host(base).buf, off, a.shape, tuple(s // 8 for s in a.strides))


def c_hadamard_close(Wl, U, V, out0, dims=None, accumulate=None, work_doubles=None, null=()):
    """One direct call of the C entry on host arrays into NaN-filled `out` (or out0 when it accumulates) and `work`:
    (status, out, work).  The keyword arguments overwrite what the arrays say, for the argument tests."""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    dW, dU, dV = DevArray.from_host(np.ascontiguousarray(Wl)), _upload(U), _upload(V)
    S, n, S1 = U.shape
    s, _, s1 = V.shape
    P = Wl.shape[2]
    slab = ref.layout(S, S1, s, s1, n, P)[2]
    out = DevArray.from_host(np.full((P, S1 * s1), np.nan) if out0 is None else out0)
    work = DevArray.from_host(np.full(slab + PAD, np.nan))
    args = dict(Wl=ctypes.c_void_p(dW.ptr), U=ctypes.c_void_p(dU.ptr), V=ctypes.c_void_p(dV.ptr),
                dims=nat.i64_array((S, S1, s, s1, n, P) if dims is None else dims),
                strides=nat.i64_array(tuple(dU.strides) + tuple(dV.strides)), out=ctypes.c_void_p(out.ptr), work=ctypes.c_void_p(work.ptr))
    for name in null:
        args[name] = None
    rc = nat.lib().ttsk_hadamard_close(args["Wl"], args["U"], args["V"], args["dims"], args["strides"], args["out"],
                                       (0 if out0 is None else 1) if accumulate is None else accumulate, args["work"],
                                       slab if work_doubles is None else work_doubles, 0)
    nat.call("ttsk_sync", -1)
    return rc, out.get(), work.get()


@pytest.fixture(scope="module")
def truth():
    """the restatement and its bound per case, computed once"""
    out = {}
    for case in ref.CASES:
        Wl, U, V, out0 = ref.case_arrays(case)
        out[case.name] = (Wl, U, V, out0, ref.close_term(Wl, U, V, out0), ref.bound(Wl, U, V, out0))
    return out


# ---- 1. the C entry against the restatement at every edge
@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.name)
def test_c_entry_vs_restatement(tsa, truth, case):
    from tt_sketch_amd import hadamard_gram as hg
    Wl, U, V, out0, want, tol = truth[case.name]
    ichunks, _, slab, _ = ref.layout(*case[1:7])
    assert hg.close_layout(*case[1:7]) == (ichunks, slab)              # ttsk_hadamard_close_layout
    rc, got, work = c_hadamard_close(Wl, U, V, out0)
    assert rc == 0
    assert np.isfinite(got).all()
    miss = np.abs(got - want)
    print(f"{case.name}: max |G' - G'_ref| / bound = {np.max(miss / np.maximum(tol, 1e-300)):.3f}, {ichunks} chunks of i")
    assert (miss <= tol).all()
    assert np.isfinite(work[:slab]).all() and np.isnan(work[slab:]).all()      # the slab, all of it and nothing past it
    if out0 is not None:                                                # a pre-filled `out` is added to
        assert (np.abs((got - out0) - ref.close_term(Wl, U, V)) <= tol).all()
    rc2, got2, work2 = c_hadamard_close(Wl, U, V, out0)
    assert rc2 == 0 and np.array_equal(got, got2) and np.array_equal(work, work2, equal_nan=True)     # the same bits on every call


@pytest.mark.parametrize("case", apply_ref.CASES, ids=lambda c: c.name)
def test_one_mode_of_close_is_apply_bit_for_bit(tsa, case):
    """The two kernels run the same stages (csrc/hadamard_stages.h).  At n = 1 the plan makes one chunk of i and
    ttsk_sum_slices adds a single slice, so closing Wl = L (R r, 1, l) with mode i of X and Y performs the matrix
    instructions of ttsk_hadamard_apply at that i in the same order: the same floats, +0 and -0 taken as equal."""
    from tests.test_gpu_hadamard import c_hadamard_apply
    L, X, Y, w_off, w_cols = apply_ref.case_arrays(case)
    rc, W = c_hadamard_apply(L, X, Y, w_off, w_cols)
    assert rc == 0
    assert ref.layout(case.R, case.R1, case.r, case.r1, 1, case.l)[0] == 1          # one chunk of i
    for i in sorted({0, case.n - 1}):
        rc, out, _ = c_hadamard_close(L.reshape(case.R * case.r, 1, case.l), X[:, i:i + 1, :], Y[:, i:i + 1, :], None)
        assert rc == 0
        want = W[:, i, w_off:w_off + case.R1 * case.r1]
        print(f"{case.name}, i = {i}: {np.count_nonzero(out != want)} of {want.size} floats differ")
        assert np.array_equal(out, want), i


# ---- 2. the ABI
def test_argument_errors_and_refusals_write_nothing(tsa, truth):
    from tt_sketch_amd import _native as nat
    case = next(c for c in ref.CASES if c.name.endswith("_flipped_views"))
    Wl, U, V, _, _, _ = truth[case.name]
    good = list(case[1:7])
    slab = ref.layout(*good)[2]

    def status(**kw):
        rc, out, work = c_hadamard_close(Wl, U, V, None, **kw)
        assert np.isnan(out).all() and np.isnan(work).all(), kw         # refused before anything is launched
        return rc

    def with_dim(field, value):
        d = list(good)
        d[field] = value
        return d

    for name in ("Wl", "U", "V", "dims", "strides", "out", "work"):
        assert status(null=(name,)) == nat.TTSK_ERR_ARG, name
    assert b"NULL" in nat.lib().ttsk_last_error()
    for field in range(6):
        assert status(dims=with_dim(field, 0)) == nat.TTSK_ERR_ARG, field
        assert status(dims=with_dim(field, -3)) == nat.TTSK_ERR_ARG, field
    assert status(accumulate=2) == nat.TTSK_ERR_ARG and status(accumulate=-1) == nat.TTSK_ERR_ARG
    assert status(work_doubles=slab - 1) == nat.TTSK_ERR_ARG and b"slab" in nat.lib().ttsk_last_error()
    assert status(work_doubles=0) == nat.TTSK_ERR_ARG
    # refused by arithmetic alone: nothing of that size exists
    for field in range(6):
        assert status(dims=with_dim(field, 2 ** 31), work_doubles=2 ** 62) == UNSUPPORTED, field
    assert b"2^31" in nat.lib().ttsk_last_error()
    d = with_dim(1, 2 ** 26)
    d[3], d[5] = 2 ** 20, 2 ** 16
    assert status(dims=d, work_doubles=2 ** 62) == UNSUPPORTED and b"workgroups" in nat.lib().ttsk_last_error()
    out = nat.i64_array((-1, -1))
    assert nat.lib().ttsk_hadamard_close_layout(nat.i64_array(with_dim(2, 0)), out) == nat.TTSK_ERR_ARG
    assert nat.lib().ttsk_hadamard_close_layout(nat.i64_array(good), None) == nat.TTSK_ERR_ARG
    assert nat.lib().ttsk_hadamard_close_layout(nat.i64_array(with_dim(4, 2 ** 31)), out) == UNSUPPORTED and list(out) == [-1, -1]


# ---- 3. hadamard_close on both routes
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", [c.name for c in ref.CASES if "_mixed_strides" in c.name or c.name.endswith("_split")])
def test_hadamard_close_routes_vs_restatement(tsa, truth, name, route):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    from tt_sketch_amd.hadamard_gram import hadamard_close
    Wl, U, V, out0, want, tol = truth[name]
    out = None if out0 is None else DevArray.from_host(out0)
    calls, real = [], nat.call
    try:
        nat.call = lambda entry, *args: (calls.append(entry), real(entry, *args))[1]
        G = hadamard_close(DevArray.from_host(Wl), _upload(U), _upload(V), out=out, accumulate=out0 is not None, route=route)
    finally:
        nat.call = real
    assert calls.count("ttsk_hadamard_close") == (1 if route == "kernel" else 0)
    assert (calls.count("ttsk_gemm") == 0) == (route == "kernel")
    if route == "composed":                                             # whatever n is
        launches = [c for c in calls if c in ("ttsk_gemm", "ttsk_copy_strided", "ttsk_axpby")]
        # five launches (four where U lies mode-major already) and one more to accumulate
        assert calls.count("ttsk_gemm") == 2 and 4 <= len(launches) - (out0 is not None) <= 5
    got = G.get()
    assert got.shape == want.shape and (out is None or G is out)
    miss = np.abs(got - want)
    print(f"{name}, {route}: max |G' - G'_ref| / bound = {np.max(miss / np.maximum(tol, 1e-300)):.3f}")
    assert (miss <= tol).all()


@pytest.mark.parametrize("S", [8, 16])
def test_routes_agree_at_a_long_mode(tsa, S):
    """n = 100 with few gamma: the composition sums over (i, gamma) as one contracted index of 100 S terms"""
    from tt_sketch_amd.device import DevArray
    from tt_sketch_amd.hadamard_gram import hadamard_close
    s, n, P = 4, 100, 16
    rng = np.random.default_rng(S)
    Wl, U, V = rng.standard_normal((S * s, n, P)), rng.standard_normal((S, n, S)), rng.standard_normal((s, n, s))
    want, tol = ref.close_term(Wl, U, V), ref.bound(Wl, U, V)
    for route in ROUTES:
        got = hadamard_close(DevArray.from_host(Wl), DevArray.from_host(U), DevArray.from_host(V), route=route).get()
        print(f"S = {S}, {route}: max |G' - G'_ref| / bound = {np.max(np.abs(got - want) / tol):.3f}")
        assert (np.abs(got - want) <= tol).all(), route


def test_hadamard_close_checks_its_operands(tsa):
    from tt_sketch_amd.device import DevArray
    from tt_sketch_amd.hadamard_gram import hadamard_close
    Wl, U, V = DevArray.zeros((6, 5, 4)), DevArray.zeros((2, 5, 3)), DevArray.zeros((3, 5, 2))
    assert hadamard_close(Wl, U, V, route="kernel").shape == (4, 6)
    with pytest.raises(ValueError, match="mode size"):
        hadamard_close(Wl, U, DevArray.zeros((3, 4, 2)))
    with pytest.raises(ValueError, match="W of shape"):
        hadamard_close(DevArray.zeros((5, 5, 4)), U, V)
    with pytest.raises(ValueError, match="out of shape"):
        hadamard_close(Wl, U, V, out=DevArray.zeros((6, 4)))
    with pytest.raises(ValueError, match="route"):
        hadamard_close(Wl, U, V, route="fastest")


# ---- 4. the surface on resident trains
SHAPES = {4: (5, 7, 4, 6), 5: (3, 4, 2, 5, 3)}
RANKS = {4: dict(x=(3, 17, 2), y=(2, 5, 4), u=(4, 2, 3), v=(2, 18, 2), z=(3, 6, 4)),           # R r and S s cross 16 on the second bond
         5: dict(x=(2, 3, 17, 2), y=(3, 2, 2, 3), u=(2, 4, 2, 2), v=(3, 2, 9, 2), z=(4, 5, 3, 2))}


@pytest.fixture(scope="module")
def resident(tsa):
    """per d: resident factors x, y, u, v and a train z, the lazy products and every dense tensor, computed once"""
    out = {}
    for d, shape in SHAPES.items():
        rng = np.random.default_rng(40 + d)
        host = {k: tsa.TensorTrain(orc.random_tt(shape, rk, rng)) for k, rk in RANKS[d].items()}
        t = {k: v.to_device() for k, v in host.items()}
        assert all(v.resident() for v in t.values())
        dense = dict(h=host["x"].to_numpy() * host["y"].to_numpy(), q=host["u"].to_numpy() * host["v"].to_numpy(), z=host["z"].to_numpy())
        out[d] = dict(t, h=tsa.HadamardProduct(t["x"], t["y"]), q=tsa.HadamardProduct(t["u"], t["v"]), dense=dense, host=host)
    return out


def _close(got, want, a, b):
    scale = 1e-12 * np.linalg.norm(a) * np.linalg.norm(b)
    print(f"got {got!r}, dense {want!r}: off by {abs(got - want) / scale:.3g} of the bar")
    return abs(got - want) <= scale


@pytest.mark.parametrize("route", ROUTES + (None,))
@pytest.mark.parametrize("d", sorted(SHAPES))
def test_dots_and_norm_against_dense(tsa, resident, d, route, monkeypatch):
    from tt_sketch_amd import HadamardProduct, hadamard_gram as hg, paths
    e = resident[d]
    h, q, z, D = e["h"], e["q"], e["z"], e["dense"]
    formed = []
    monkeypatch.setattr(HadamardProduct, "to_tt", lambda self: formed.append(1) or pytest.fail("to_tt was entered"))
    with paths.forced(route):
        assert _close(hg.hadamard_dot(h, q), np.vdot(D["h"], D["q"]), D["h"], D["q"])
        assert _close(h.dot(q), np.vdot(D["h"], D["q"]), D["h"], D["q"]) and _close(q.dot(h), np.vdot(D["h"], D["q"]), D["h"], D["q"])
        assert _close(hg.hadamard_tt_dot(h, z), np.vdot(D["h"], D["z"]), D["h"], D["z"])
        assert _close(z.dot(h), np.vdot(D["h"], D["z"]), D["h"], D["z"])                     # from the train's side
        assert _close(h.norm() ** 2, np.vdot(D["h"], D["h"]), D["h"], D["h"])
        # .T operands: views of the cores, the chain runs from the other end
        assert _close(h.T.dot(q.T), np.vdot(D["h"], D["q"]), D["h"], D["q"])
        assert _close(h.T.dot(z.T), np.vdot(D["h"], D["z"]), D["h"], D["z"])
    assert h.dot(q, route="kernel") == h.dot(q, route="kernel")                              # the same bits
    assert not formed


@pytest.mark.parametrize("d", sorted(SHAPES))
def test_fast_error_gather_and_sums_against_dense(tsa, resident, d, monkeypatch):
    from tt_sketch_amd import HadamardProduct, TensorSum
    e = resident[d]
    h, q, z, D = e["h"], e["q"], e["z"], e["dense"]
    entered = []
    monkeypatch.setattr(HadamardProduct, "to_tt", lambda self: entered.append(1) or pytest.fail("to_tt was entered"))
    for a, b, da, db in ((z, h, D["z"], D["h"]), (h, q, D["h"], D["q"]), (h, z, D["h"], D["z"])):
        want = np.linalg.norm(da - db) / np.linalg.norm(db)
        assert want >= 0.1                                            # far above the floor of the fast formula
        got = a.error(b, fast=True, relative=True)
        print(f"d = {d}: fast relative error {got!r}, dense {want!r}")
        assert abs(got - want) <= 1e-10
    assert abs(z.error(h, fast=True) - np.linalg.norm(D["z"] - D["h"])) <= 1e-10 * np.linalg.norm(D["h"])
    assert abs(z.error(h, fast=True, rmse=True) * np.sqrt(D["h"].size) - np.linalg.norm(D["z"] - D["h"])) <= 1e-10 * np.linalg.norm(D["h"])
    # a sum that holds a Hadamard term arrives term by term
    both, dboth = TensorSum([z, q * -1.5]), D["z"] - 1.5 * D["q"]
    terms = np.linalg.norm(D["z"]) + 1.5 * np.linalg.norm(D["q"])       # each term's inner product has its own bar
    assert abs(h.dot(both) - np.vdot(D["h"], dboth)) <= 1e-12 * np.linalg.norm(D["h"]) * terms
    assert abs(both.dot(h) - np.vdot(D["h"], dboth)) <= 1e-12 * np.linalg.norm(D["h"]) * terms
    want = np.linalg.norm(D["h"] - dboth) / np.linalg.norm(dboth)
    assert want >= 0.1 and abs(h.error(both, fast=True, relative=True) - want) <= 1e-10
    # gather: two device passes and a host multiply
    rng = np.random.default_rng(d)
    idx = np.stack([rng.integers(0, n, 50) for n in SHAPES[d]])
    got = h.gather(idx)
    assert got.shape == (50,) and np.allclose(got, D["h"][tuple(idx)], rtol=1e-12, atol=1e-13 * np.abs(D["h"]).max())
    assert not entered


def test_one_resident_factor_is_enough_and_host_factors_stay_on_the_host(tsa, resident):
    from tt_sketch_amd import HadamardProduct, _native as nat
    e = resident[4]
    host, D = e["host"], e["dense"]
    mixed = HadamardProduct(e["x"], tsa.TensorTrain([np.array(c) for c in host["y"].cores]))
    assert _close(mixed.dot(e["q"]), np.vdot(D["h"], D["q"]), D["h"], D["q"])
    on_host = HadamardProduct(*(tsa.TensorTrain([np.array(c) for c in host[k].cores]) for k in ("x", "y")))
    calls, real = [], nat.call
    try:
        nat.call = lambda entry, *args: (calls.append(entry), real(entry, *args))[1]
        got = on_host.dot(on_host)
    finally:
        nat.call = real
    assert not calls and _close(got, np.vdot(D["h"], D["h"]), D["h"], D["h"])


def test_a_small_budget_cuts_a_mode_into_three_slices(tsa, resident, monkeypatch):
    """the second mode (n = 7) in slices of 3, 3 and 1, the later ones accumulated; the same inner product"""
    from tt_sketch_amd import _native as nat, hadamard_gram as hg
    e = resident[4]
    h, q, z, D = e["h"], e["q"], e["z"], e["dense"]
    rk = RANKS[4]
    seen, real = [], nat.call

    def spy(entry, *args):
        if entry == "ttsk_hadamard_close":
            seen.append((int(args[3][4]), int(args[6])))               # n of the call, accumulate
        if entry == "ttsk_gemm":
            seen.append(("gemm", int(args[0]._obj.accumulate)))
        return real(entry, *args)
    whole = h.dot(q, route="kernel")
    monkeypatch.setattr(hg, "W_BUDGET_BYTES", 8 * 3 * (rk["u"][0] * rk["v"][0]) * (rk["x"][1] * rk["y"][1]))
    try:
        nat.call = spy
        cut = h.dot(q, route="kernel")
    finally:
        nat.call = real
    closes = [c for c in seen if c[0] != "gemm"]
    assert closes[1:4] == [(3, 0), (3, 1), (1, 1)], closes
    assert _close(cut, np.vdot(D["h"], D["q"]), D["h"], D["q"]) and abs(cut - whole) <= 1e-13 * abs(whole)
    # the chain against a train, its `contract` accumulating
    monkeypatch.setattr(hg, "W_BUDGET_BYTES", 8 * 3 * rk["z"][0] * (rk["x"][1] * rk["y"][1]))
    seen.clear()
    try:
        nat.call = spy
        cut = h.dot(z)
    finally:
        nat.call = real
    assert [c[1] for c in seen if c[0] == "gemm"].count(1) >= 2
    assert _close(cut, np.vdot(D["h"], D["z"]), D["h"], D["z"])


# ---- 5. the routing rule
def _recorded():
    with open(os.path.join(ROOT, "profiles", "hadamard_gram_bench.json")) as f:
        return json.load(f)


def test_routing_rule_against_the_recorded_verdicts(tsa):
    """Only the rule is evaluated: at every shape of step B alone in profiles/hadamard_gram_bench.json where the two measured
    ranges are apart, it names the faster route."""
    from tt_sketch_amd import hadamard_gram as hg
    rows = _recorded()["close_alone"]
    assert len(rows) >= 4
    decided = 0
    for row in rows:
        k, c = row["kernel_ms"], row["composed_ms"]                    # each [median, min, max]
        kernel_ms, composed_ms = hg.close_route_ms(row["S"], row["S1"], row["s"], row["s1"], row["n"], row["P"])
        named = "composed" if composed_ms < kernel_ms else "kernel"
        print(f"S {row['S']} s {row['s']} n {row['n']} P {row['P']}: kernel {k}, composed {c}; the rule expects {kernel_ms:.3f} / {composed_ms:.3f} ms -> {named}")
        if k[2] < c[1]:
            decided += 1
            assert named == "kernel"
        elif c[2] < k[1]:
            decided += 1
            assert named == "composed"
    assert decided >= 1


@pytest.mark.parametrize("dims,expected", [((4, 4, 3, 3, 5, 6), "kernel"), ((20, 20, 20, 20, 20, 400), "kernel"),
                                           ((17, 17, 17, 17, 20, 1700), "composed")], ids=["small", "large", "padded"])
def test_unforced_calls_take_the_route_the_rule_names(tsa, dims, expected):
    from tt_sketch_amd import _native as nat, hadamard_gram as hg
    from tt_sketch_amd.device import DevArray
    S, S1, s, s1, n, P = dims
    rng = np.random.default_rng(3)
    Wl, U, V = rng.standard_normal((S * s, n, P)), rng.standard_normal((S, n, S1)), rng.standard_normal((s, n, s1))
    kernel_ms, composed_ms = hg.close_route_ms(*dims)
    named = "composed" if composed_ms < kernel_ms else "kernel"
    assert named == expected                       # tiles of 17 are padded to 20 and 32: 3.4 times the flops, past the composition's
    calls, real = [], nat.call
    try:
        nat.call = lambda entry, *args: (calls.append(entry), real(entry, *args))[1]
        G = hg.hadamard_close(DevArray.from_host(Wl), DevArray.from_host(U), DevArray.from_host(V))
    finally:
        nat.call = real
    assert calls.count("ttsk_hadamard_close") == (1 if named == "kernel" else 0)
    assert (np.abs(G.get() - ref.close_term(Wl, U, V)) <= ref.bound(Wl, U, V)).all()
