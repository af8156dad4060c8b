"""Inner products of operator-times-train products that are never formed, on the device: ``ttsk_op_close``
(csrc/op_close.hip) entry by entry, ``op_close`` on both routes, and ``OperatorProduct.dot`` / ``norm`` /
``error(fast=True)``, ``TensorTrain.error(fast=True)`` and ``TTLinearMapSum.residual`` on resident factors against dense
NumPy.

Bar of the entry (tests/op_close_ref.py): |G' - G'_ref| <= 2 (S n_out + s + n_in + 3) 2^-53 G'_abs entry by entry, the same
bits on a second call, nothing written past the plan's slab; at n_in = n_out = 1 the floats of ``ttsk_hadamard_close`` on the
same operands (both kernels run the stages of csrc/hadamard_stages.h).  Bars of the surface, those of
tests/test_gpu_hadamard_close.py: inner products within 1e-12 ||a|| ||b||, the fast error within 1e-10 of the dense one on
tensors at a relative distance of 0.1 or more.
"""
import ctypes

import numpy as np
import pytest

from tests import hadamard_close_ref
from tests import op_close_ref as ref
from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3
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


def c_op_close(Wl, N, Y, out0, dims=None, accumulate=None, work_doubles=None, null=(), n_strides=None):
    """One direct call of the C entry on host arrays into NaN-filled `out` (or out0 when it accumulates) and `work`:
    (status, out, work).  The keyword arguments overwrite what the arrays say, for the argument tests."""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    dW, dN, dY = DevArray.from_host(np.ascontiguousarray(Wl)), _upload(N), _upload(Y)
    S, n_in, n_out, S1 = N.shape
    s, _, s1 = Y.shape
    P = Wl.shape[2]
    good = (S, S1, s, s1, n_in, n_out, P)
    slab = ref.layout(*good)[2]
    out = DevArray.from_host(np.full((P, s1 * S1), np.nan) if out0 is None else out0)
    work = DevArray.from_host(np.full(slab + PAD, np.nan))
    args = dict(Wl=ctypes.c_void_p(dW.ptr), N=ctypes.c_void_p(dN.ptr), Y=ctypes.c_void_p(dY.ptr),
                dims=nat.i64_array(good if dims is None else dims),
                strides=nat.i64_array(tuple(dN.strides if n_strides is None else n_strides) + tuple(dY.strides)),
                out=ctypes.c_void_p(out.ptr), work=ctypes.c_void_p(work.ptr))
    for name in null:
        args[name] = None
    rc = nat.lib().ttsk_op_close(args["Wl"], args["N"], args["Y"], args["dims"], args["strides"], args["out"],
                                 (0 if out0 is None else 1) if accumulate is None else accumulate, args["work"],
                                 slab if work_doubles is None else work_doubles, 0)
    nat.call("ttsk_sync", -1)
    return rc, out.get(), work.get()


@pytest.fixture(scope="module")
def truth():
    """the restatement and its bound per case, computed once"""
    out = {}
    for case in ref.CASES:
        Wl, N, Y, out0 = ref.case_arrays(case)
        out[case.name] = (Wl, N, Y, out0, ref.close_term(Wl, N, Y, out0), ref.bound(Wl, N, Y, out0))
    return out


# ---- 1. the C entry against the restatement at every edge
@pytest.mark.parametrize("case", ref.CASES, ids=lambda c: c.name)
def test_c_entry_vs_restatement(tsa, truth, case):
    from tt_sketch_amd import operator_gram as og
    Wl, N, Y, out0, want, tol = truth[case.name]
    jchunks, _, slab, _ = ref.layout(*ref.dims(case))
    assert og.close_layout(*ref.dims(case)) == (jchunks, slab)          # ttsk_op_close_layout
    rc, got, work = c_op_close(Wl, N, Y, out0)
    assert rc == 0
    assert np.isfinite(got).all()
    miss = np.abs(got - want)
    print(f"{case.name}: max |G' - G'_ref| / bound = {np.max(miss / np.maximum(tol, 1e-300)):.3f}, {jchunks} chunks of j")
    assert (miss <= tol).all()
    assert np.isfinite(work[:slab]).all() and np.isnan(work[slab:]).all()      # the slab, all of it and nothing past it
    if out0 is not None:                                                # a pre-filled `out` is added to
        assert (np.abs((got - out0) - ref.close_term(Wl, N, Y)) <= tol).all()
    rc2, got2, work2 = c_op_close(Wl, N, Y, out0)
    assert rc2 == 0 and np.array_equal(got, got2) and np.array_equal(work, work2, equal_nan=True)     # the same bits on every call


@pytest.mark.parametrize("name", [hadamard_close_ref.CASES[k].name for k in (0, 7, 9)])
def test_one_index_pair_of_op_close_is_hadamard_close_bit_for_bit(tsa, name):
    """The two kernels run the same stages (csrc/hadamard_stages.h).  At n_in = n_out = 1 the pair (gamma, i) is gamma alone and
    the loop over j has one turn, so closing Wl with N = V and Y = U performs the matrix instructions of ttsk_hadamard_close
    at n = 1 with that U and V in the same order: the same floats, +0 and -0 taken as equal."""
    from tests.test_gpu_hadamard_close import c_hadamard_close
    case = next(c for c in hadamard_close_ref.CASES if c.name == name)
    Wl, U, V, _ = hadamard_close_ref.case_arrays(case)
    for i in sorted({0, case.n - 1}):
        Wi, Ui, Vi = Wl[:, i:i + 1, :], U[:, i:i + 1, :], V[:, i:i + 1, :]
        rc, want, _ = c_hadamard_close(Wi, Ui, Vi, None)
        assert rc == 0
        N = Vi[:, :, None, :]                                           # (S, 1, 1, S') of this entry: the s, s' of that one
        assert ref.layout(case.s, case.s1, case.S, case.S1, 1, 1, case.P)[0] == 1      # one chunk of j
        rc, got, _ = c_op_close(Wi, N, Ui, None)
        assert rc == 0
        print(f"{name}, i = {i}: {np.count_nonzero(got != want)} of {want.size} floats differ")
        assert np.array_equal(got, want), i


# ---- 2. the ABI
def test_argument_errors_and_refusals_write_nothing(tsa, truth):
    from tt_sketch_amd import _native as nat
    case = next(c for c in ref.CASES if c.name.endswith("_flipped_views"))
    Wl, N, Y, _, _, _ = truth[case.name]
    good = list(ref.dims(case))
    slab = ref.layout(*good)[2]

    def status(**kw):
        rc, out, work = c_op_close(Wl, N, Y, None, **kw)
        assert np.isnan(out).all() and np.isnan(work).all(), kw         # refused before anything is launched
        return rc

    def with_dim(field, value):
        d = list(good)
        d[field] = value
        return d

    for name in ("Wl", "N", "Y", "dims", "strides", "out", "work"):
        assert status(null=(name,)) == nat.TTSK_ERR_ARG, name
    assert b"NULL" in nat.lib().ttsk_last_error()
    for field in range(7):
        assert status(dims=with_dim(field, 0)) == nat.TTSK_ERR_ARG, field
        assert status(dims=with_dim(field, -3)) == nat.TTSK_ERR_ARG, field
    assert status(accumulate=2) == nat.TTSK_ERR_ARG and status(accumulate=-1) == nat.TTSK_ERR_ARG
    assert status(work_doubles=slab - 1) == nat.TTSK_ERR_ARG and b"slab" in nat.lib().ttsk_last_error()
    assert status(work_doubles=0) == nat.TTSK_ERR_ARG
    # an N that is not one run: the strides of a core as an MPO stores it
    S, S1, s, s1, n_in, n_out, P = good
    assert S > 1 and n_out > 1
    assert status(n_strides=(n_in * n_out * S1, n_out * S1, S1, 1)) == UNSUPPORTED and b"one run" in nat.lib().ttsk_last_error()
    # refused by arithmetic alone: nothing of that size exists
    for field in range(7):
        assert status(dims=with_dim(field, 2 ** 31), work_doubles=2 ** 62) == UNSUPPORTED, field
    assert b"2^31" in nat.lib().ttsk_last_error()
    d = with_dim(0, 2 ** 16)
    d[5] = 2 ** 15
    assert status(dims=d, work_doubles=2 ** 62) == UNSUPPORTED and b"S n_out" in nat.lib().ttsk_last_error()
    d = with_dim(1, 2 ** 20)
    d[3], d[6] = 2 ** 26, 2 ** 16
    assert status(dims=d, work_doubles=2 ** 62) == UNSUPPORTED and b"workgroups" in nat.lib().ttsk_last_error()
    out = nat.i64_array((-1, -1))
    assert nat.lib().ttsk_op_close_layout(nat.i64_array(with_dim(2, 0)), out) == nat.TTSK_ERR_ARG
    assert nat.lib().ttsk_op_close_layout(nat.i64_array(good), None) == nat.TTSK_ERR_ARG
    assert nat.lib().ttsk_op_close_layout(nat.i64_array(with_dim(4, 2 ** 31)), out) == UNSUPPORTED and list(out) == [-1, -1]


# ---- 3. op_close on both routes
def _spied(fn):
    """fn() with every library call recorded: (result, names of the calls)"""
    from tt_sketch_amd import _native as nat
    calls, real = [], nat.call
    try:
        nat.call = lambda entry, *args: (calls.append(entry), real(entry, *args))[1]
        return fn(), calls
    finally:
        nat.call = real


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", [c.name for c in ref.CASES if "_mixed_strides" in c.name or c.name.endswith(("_split", "_ragged_chunks"))])
def test_op_close_routes_vs_restatement(tsa, truth, name, route):
    from tt_sketch_amd.device import DevArray
    from tt_sketch_amd.operator_gram import op_close
    Wl, N, Y, out0, want, tol = truth[name]
    out = None if out0 is None else DevArray.from_host(out0)
    G, calls = _spied(lambda: op_close(DevArray.from_host(Wl), _upload(N), _upload(Y), out=out, accumulate=out0 is not None, route=route))
    assert calls.count("ttsk_op_close") == (1 if route == "kernel" else 0)
    assert (calls.count("ttsk_gemm") == 0) == (route == "kernel")
    if route == "composed":                                             # whatever n_in is
        launches = [c for c in calls if c in ("ttsk_gemm", "ttsk_copy_strided", "ttsk_axpby")]
        # five launches (four where Y is contiguous already), one more to accumulate, one more for an N with padding
        padded = "padded" in next(c for c in ref.CASES if c.name == name).n_layout
        assert calls.count("ttsk_gemm") == 2 and 4 <= len(launches) - int(out0 is not None) - int(padded) <= 5
    got = G.get()
    assert got.shape == want.shape and (out is None or G is out)
    miss = np.abs(got - want)
    print(f"{name}, {route}: max |G' - G'_ref| / bound = {np.max(miss / np.maximum(tol, 1e-300)):.3f}")
    assert (miss <= tol).all()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("view", ["stored", "mpo_T", "reversed"])
def test_op_close_packs_a_core_that_is_not_one_run(tsa, view, route):
    """a core as an MPO stores it and the mode-reversed view of ``OperatorProduct.T`` are packed (one strided copy); the view
    ``MPO.T`` hands out of a stored core is one run as it lies"""
    from tt_sketch_amd.device import DevArray
    from tt_sketch_amd.operator_gram import one_run, op_close
    S, S1, s, s1, n_in, n_out, P = 3, 2, 5, 4, 6, 4, 17
    rng = np.random.default_rng(11)
    if view == "stored":
        N = rng.standard_normal((S, n_in, n_out, S1))
    elif view == "mpo_T":
        N = rng.standard_normal((S, n_out, n_in, S1)).transpose(0, 2, 1, 3)
    else:
        N = rng.standard_normal((S1, n_in, n_out, S)).transpose(3, 1, 2, 0)
    Wl, Y = rng.standard_normal((s * S, n_out, P)), rng.standard_normal((s, n_in, s1))
    dN = _upload(N)
    assert one_run(dN) == ref.one_run(N) == (view == "mpo_T")
    G, calls = _spied(lambda: op_close(DevArray.from_host(Wl), dN, DevArray.from_host(Y), route=route))
    copies = calls.count("ttsk_copy_strided") - (2 if route == "composed" else 0)
    assert copies == (0 if view == "mpo_T" else 1)
    assert (np.abs(G.get() - ref.close_term(Wl, N, Y)) <= ref.bound(Wl, N, Y)).all()


def test_op_close_checks_its_operands(tsa):
    from tt_sketch_amd.device import DevArray
    from tt_sketch_amd.operator_gram import op_close
    Wl, N, Y = DevArray.zeros((6, 5, 4)), DevArray.zeros((2, 7, 5, 3)), DevArray.zeros((3, 7, 2))
    assert op_close(Wl, N, Y, route="kernel").shape == (4, 6)
    with pytest.raises(ValueError, match="does not act"):
        op_close(Wl, N, DevArray.zeros((3, 4, 2)))
    with pytest.raises(ValueError, match="W of shape"):
        op_close(DevArray.zeros((5, 5, 4)), N, Y)
    with pytest.raises(ValueError, match="out of shape"):
        op_close(Wl, N, Y, out=DevArray.zeros((6, 4)))
    with pytest.raises(ValueError, match="route"):
        op_close(Wl, N, Y, route="fastest")


# ---- 4. the surface on resident factors
OUT = {3: (4, 6, 3), 4: (5, 3, 4, 6), 5: (3, 4, 2, 5, 3)}
IN_X = {3: (5, 2, 6), 4: (3, 6, 2, 5), 5: (2, 5, 3, 4, 2)}          # x and y live on other mode sizes than the products
IN_Y = {3: (3, 4, 1), 4: (4, 2, 5, 3), 5: (4, 3, 3, 2, 5)}
TRAIN_RANKS = {3: dict(x=(3, 5), y=(4, 2), z=(5, 3), b=(2, 4), w=(3, 3)),
               4: dict(x=(3, 5, 2), y=(2, 4, 5), z=(3, 4, 4), b=(2, 3, 2), w=(4, 3, 2)),
               5: dict(x=(2, 3, 5, 2), y=(3, 2, 4, 3), z=(4, 5, 3, 2), b=(2, 2, 3, 2), w=(2, 4, 3, 2))}
OP_RANKS = {3: dict(M=(3, 2), N=(2, 3), A=((2, 3), (1, 2), (3, 1))),
            4: dict(M=(2, 3, 2), N=(3, 2, 3), A=((2, 3, 2), (1, 1, 2), (3, 2, 1))),
            5: dict(M=(2, 3, 2, 3), N=(3, 2, 3, 2), A=((2, 2, 3, 2), (1, 2, 1, 2), (3, 1, 2, 3)))}


def _cores(rng, shapes, rank):
    rank = (1,) + tuple(rank) + (1,)
    return [rng.standard_normal((rank[k],) + tuple(sh) + (rank[k + 1],)) for k, sh in enumerate(shapes)]


@pytest.fixture(scope="module")
def resident(tsa):
    """per d: resident trains and operators, the lazy products and every dense tensor, computed once.  h = M x and q = N y map
    other shapes onto the one of z and b; the A_p map that shape onto itself and act on w."""
    from tt_sketch_amd.tt_gmres import MPO, TTLinearMapSum
    out = {}
    for d, shape in OUT.items():
        rng = np.random.default_rng(60 + d)
        tr = dict(x=_cores(rng, [(n,) for n in IN_X[d]], TRAIN_RANKS[d]["x"]), y=_cores(rng, [(n,) for n in IN_Y[d]], TRAIN_RANKS[d]["y"]))
        for k in ("z", "b", "w"):
            tr[k] = _cores(rng, [(n,) for n in shape], TRAIN_RANKS[d][k])
        ops = dict(M=_cores(rng, zip(IN_X[d], shape), OP_RANKS[d]["M"]), N=_cores(rng, zip(IN_Y[d], shape), OP_RANKS[d]["N"]))
        As = [_cores(rng, zip(shape, shape), rk) for rk in OP_RANKS[d]["A"]]
        dense = dict(h=ref.dense_product(ops["M"], tr["x"]), q=ref.dense_product(ops["N"], tr["y"]),
                     Aw=[ref.dense_product(A, tr["w"]) for A in As])
        for k in ("z", "b", "w"):
            dense[k] = tsa.TensorTrain(tr[k]).to_numpy()
        t = {k: tsa.TensorTrain(v).to_device() for k, v in tr.items()}
        assert all(v.resident() for v in t.values())
        mpos = {k: MPO(v) for k, v in ops.items()}
        maps = [MPO(A) for A in As]
        for m in list(mpos.values()) + maps:
            m.dev_views()                                               # uploaded once, before the host is closed
            assert m.resident()
        out[d] = dict(t, h=tsa.OperatorProduct(mpos["M"], t["x"]), q=tsa.OperatorProduct(mpos["N"], t["y"]),
                      A=TTLinearMapSum(maps), dense=dense)
    return out


def _close(got, want, a, b):
    scale = 1e-12 * np.linalg.norm(a) * np.linalg.norm(b)
    print(f"got {got!r}, dense {want!r}: off by {abs(got - want) / scale:.3g} of the bar")
    return abs(got - want) <= scale


def _close_the_host(monkeypatch):
    """a fall-back to ``to_numpy()``, to the formed product or to the host cores fails the test"""
    from tt_sketch_amd import OperatorProduct, operator_gram as og, tensor as tmod
    from tt_sketch_amd.tt_gmres import MPO

    def closed(*a, **k):
        raise AssertionError("host detour: tensor._host, to_tt or an applied operator")
    monkeypatch.setattr(tmod, "_host", closed)
    monkeypatch.setattr(og, "_host", closed)
    monkeypatch.setattr(OperatorProduct, "to_tt", closed)
    monkeypatch.setattr(MPO, "__call__", closed)


@pytest.mark.parametrize("host", ["open", "closed"])
@pytest.mark.parametrize("route", ROUTES + (None,))
@pytest.mark.parametrize("d", sorted(OUT))
def test_dots_and_norm_against_dense(tsa, resident, d, route, host, monkeypatch):
    from tt_sketch_amd import operator_gram as og, paths
    e = resident[d]
    h, q, z, D = e["h"], e["q"], e["z"], e["dense"]
    if host == "closed":
        _close_the_host(monkeypatch)
    with paths.forced(route):
        assert _close(og.op_dot(h, q), np.vdot(D["h"], D["q"]), D["h"], D["q"])
        assert _close(h.dot(q), np.vdot(D["h"], D["q"]), D["h"], D["q"]) and _close(q.dot(h), np.vdot(D["h"], D["q"]), D["h"], D["q"])
        assert _close(og.op_tt_dot(h, z), np.vdot(D["h"], D["z"]), D["h"], D["z"])
        assert _close(h.dot(z), np.vdot(D["h"], D["z"]), D["h"], D["z"])
        assert _close(z.dot(h), np.vdot(D["h"], D["z"]), D["h"], D["z"])                     # from the train's side
        assert _close(h.norm() ** 2, np.vdot(D["h"], D["h"]), D["h"], D["h"])
        assert _close(q.norm() ** 2, np.vdot(D["q"], D["q"]), D["q"], D["q"])
        # .T operands: views of the cores, the chain runs from the other end and N is packed from a reversed view
        assert _close(h.T.dot(q.T), np.vdot(D["h"], D["q"]), D["h"], D["q"])
        assert _close(h.T.dot(z.T), np.vdot(D["h"], D["z"]), D["h"], D["z"])
    assert h.dot(q, route="kernel") == h.dot(q, route="kernel")                              # the same bits


@pytest.mark.parametrize("host", ["open", "closed"])
@pytest.mark.parametrize("d", sorted(OUT))
def test_fast_error_residual_and_sums_against_dense(tsa, resident, d, host, monkeypatch):
    from tt_sketch_amd import TensorSum
    e = resident[d]
    h, q, z, b, w, A, D = e["h"], e["q"], e["z"], e["b"], e["w"], e["A"], e["dense"]
    if host == "closed":
        _close_the_host(monkeypatch)
    for a, c, da, dc in ((z, h, D["z"], D["h"]), (h, q, D["h"], D["q"]), (h, z, D["h"], D["z"])):
        want = np.linalg.norm(da - dc) / np.linalg.norm(dc)
        assert want >= 0.1                                            # far above the floor of the fast formula
        got = a.error(c, fast=True, relative=True)
        print(f"d = {d}: fast relative error {got!r}, dense {want!r}")
        assert abs(got - want) <= 1e-10
    assert abs(z.error(h, fast=True) - np.linalg.norm(D["z"] - D["h"])) <= 1e-10 * np.linalg.norm(D["h"])
    assert abs(z.error(h, fast=True, rmse=True) * np.sqrt(D["h"].size) - np.linalg.norm(D["z"] - D["h"])) <= 1e-10 * np.linalg.norm(D["h"])
    # the true residual of a sum of three operators: nothing formed
    res = D["b"] - sum(D["Aw"])
    assert np.linalg.norm(res) / np.linalg.norm(D["b"]) >= 0.1
    got = A.residual(w, b)
    print(f"d = {d}: residual {got!r}, dense {np.linalg.norm(res)!r}")
    assert abs(got - np.linalg.norm(res)) <= 1e-10 * np.linalg.norm(res)
    assert abs(A.residual(w, b, relative=True) - np.linalg.norm(res) / np.linalg.norm(D["b"])) <= 1e-10 * np.linalg.norm(res) / np.linalg.norm(D["b"])
    # a sum of two products and a train arrives term by term
    both, dboth = TensorSum([h, q * -1.5, z]), D["h"] - 1.5 * D["q"] + D["z"]
    terms = np.linalg.norm(D["h"]) + 1.5 * np.linalg.norm(D["q"]) + np.linalg.norm(D["z"])     # each term's inner product has its own bar
    assert abs(h.dot(both) - np.vdot(D["h"], dboth)) <= 1e-12 * np.linalg.norm(D["h"]) * terms
    assert abs(both.dot(h) - np.vdot(D["h"], dboth)) <= 1e-12 * np.linalg.norm(D["h"]) * terms
    assert abs(both.dot(z) - np.vdot(D["z"], dboth)) <= 1e-12 * np.linalg.norm(D["z"]) * terms
    want = np.linalg.norm(D["b"] - dboth) / np.linalg.norm(dboth)
    assert want >= 0.1 and abs(b.error(both, fast=True, relative=True) - want) <= 1e-10


def test_the_operator_is_packed_once_and_host_factors_stay_on_the_host(tsa, resident):
    from tt_sketch_amd import OperatorProduct
    from tt_sketch_amd.tt_gmres import MPO
    e = resident[4]
    h, q, D = e["h"], e["q"], e["dense"]
    q.mpo._packed_key = None
    _, first = _spied(lambda: h.dot(q, route="kernel"))
    _, second = _spied(lambda: h.dot(q, route="kernel"))
    packed = sum(1 for c in q.mpo.dev_views() if c.shape[0] > 1 and c.shape[2] > 1)
    assert packed >= 2 and first.count("ttsk_copy_strided") - second.count("ttsk_copy_strided") == packed
    assert second.count("ttsk_op_close") == 4
    on_host = OperatorProduct(MPO([c.get() for c in h.mpo.dev_views()]), tsa.TensorTrain([c.get() for c in h.tt.cores]))
    got, calls = _spied(lambda: on_host.dot(on_host))
    assert not calls and _close(got, np.vdot(D["h"], D["h"]), D["h"], D["h"])
    mixed = OperatorProduct(on_host.mpo, h.tt)                        # one resident factor is enough
    assert _close(mixed.dot(q), np.vdot(D["h"], D["q"]), D["h"], D["q"])


def test_a_small_budget_cuts_a_mode_into_three_slices(tsa, resident, monkeypatch):
    """the second mode of d = 3 (n_out = 6) in slices of 2, 2 and 2, the later ones accumulated; the same inner product"""
    from tt_sketch_amd import _native as nat, hadamard_gram as hg
    e = resident[3]
    h, q, z, D = e["h"], e["q"], e["z"], e["dense"]
    seen, real = [], nat.call

    def spy(entry, *args):
        if entry == "ttsk_op_close":
            seen.append((int(args[3][5]), int(args[6])))               # n_out of the call, accumulate
        if entry == "ttsk_gemm":
            seen.append(("gemm", int(args[0]._obj.accumulate)))
        return real(entry, *args)
    whole = h.dot(q, route="kernel")
    P = OP_RANKS[3]["M"][1] * TRAIN_RANKS[3]["x"][1]                   # R' r' behind the second mode
    monkeypatch.setattr(hg, "W_BUDGET_BYTES", 8 * 2 * (OP_RANKS[3]["N"][0] * TRAIN_RANKS[3]["y"][0]) * P)
    try:
        nat.call = spy
        cut = h.dot(q, route="kernel")
    finally:
        nat.call = real
    closes = [c for c in seen if c[0] != "gemm"]
    assert closes[1:4] == [(2, 0), (2, 1), (2, 1)], closes
    assert _close(cut, np.vdot(D["h"], D["q"]), D["h"], D["q"]) and abs(cut - whole) <= 1e-13 * abs(whole)
    # the chain against a train, its `contract` accumulating
    monkeypatch.setattr(hg, "W_BUDGET_BYTES", 8 * 2 * TRAIN_RANKS[3]["z"][0] * P)
    seen.clear()
    try:
        nat.call = spy
        cut = h.dot(z)
    finally:
        nat.call = real
    assert [c[1] for c in seen if c[0] == "gemm"].count(1) >= 2
    assert _close(cut, np.vdot(D["h"], D["z"]), D["h"], D["z"])


# ---- 5. the routing rule
def test_unforced_calls_take_the_route_the_rule_names(tsa):
    from tt_sketch_amd import operator_gram as og
    from tt_sketch_amd.device import DevArray
    for dims in ((2, 3, 3, 4, 5, 4, 6), (3, 17, 5, 17, 4, 3, 40)):
        S, S1, s, s1, n_in, n_out, P = dims
        rng = np.random.default_rng(3)
        Wl, Y = rng.standard_normal((s * S, n_out, P)), rng.standard_normal((s, n_in, s1))
        N = rng.standard_normal((S, n_out, n_in, S1)).transpose(0, 2, 1, 3)
        kernel_ms, composed_ms = og.close_route_ms(*dims)
        named = "composed" if composed_ms < kernel_ms else "kernel"
        G, calls = _spied(lambda: og.op_close(DevArray.from_host(Wl), _upload(N), DevArray.from_host(Y)))
        assert calls.count("ttsk_op_close") == (1 if named == "kernel" else 0)
        assert (np.abs(G.get() - ref.close_term(Wl, N, Y)) <= ref.bound(Wl, N, Y)).all()
