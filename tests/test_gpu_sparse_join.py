"""The sorted-key join of sparse tensors on the device: ``ttsk_sparse_key_index`` / ``ttsk_sparse_join`` /
``ttsk_dense_join`` (csrc/sparse_join.hip) and the Python surface built on them (``SparseTensor.dot`` against a sparse or
a dense tensor, ``gather``, ``gather_dev``, sums with sparse terms).

Bars: the index arrays and ``out`` are copied, never computed: exact (``np.array_equal``) against the restatement of
tests/sparse_join_ref.py.  ``dot`` against the long-double truth inside ``(1 + D) 2^-53 sum |qval tval|`` with D the
longest chain of additions of the stated order, from the plan's own numbers (``ttsk_sparse_join_layout``)."""
import ctypes

import numpy as np
import pytest

from tests import sparse_join_ref as sj
from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

ARG, UNSUPPORTED = -2, -3
GUARD = 16
F_FILL, I_FILL = -777.25, -99


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ptr)


def c_layout(N_table, Nq, max_split=0):
    from tt_sketch_amd import _native as nat
    out = (ctypes.c_int64 * 8)()
    assert nat.lib().ttsk_sparse_join_layout(ctypes.c_size_t(N_table), ctypes.c_size_t(Nq), max_split, out) == 0
    lay = dict(zip(("max_split", "stride", "n_split", "lds_steps", "seg_steps", "grid", "run", "depth"), (int(v) for v in out)))
    cap = max_split or lay["max_split"]
    want = sj.layout(N_table, Nq, cap, max(lay["grid"], 1))        # every number but the grid follows from the sizes alone
    assert (lay["stride"], lay["n_split"], lay["lds_steps"], lay["seg_steps"]) == (want["stride"], want["n_split"], want["lds_steps"],
                                                                                  want["seg_steps"])
    assert lay["grid"] <= -(-Nq // sj.THREADS) and lay["run"] == (-(-Nq // lay["grid"]) if lay["grid"] else 0)
    assert lay["depth"] == -(-lay["run"] // sj.THREADS) + sj.BLOCK_SUMS + -(-lay["grid"] // 256) + sj.CLOSE_SUMS
    return lay


class Guarded:
    """A device array of n values with GUARD values of a fixed pattern on either side."""

    def __init__(self, n, dtype=np.float64, fill=None):
        from tt_sketch_amd.device import DevArray
        self.n, self.fill = n, (F_FILL if dtype == np.float64 else I_FILL) if fill is None else fill
        self.full = DevArray.from_host(np.full(n + 2 * GUARD, self.fill, dtype=dtype), dtype=dtype)
        self.ptr = self.full.ptr + GUARD * 8

    def get(self):
        h = self.full.get()
        assert (h[:GUARD] == self.fill).all() and (h[GUARD + self.n:] == self.fill).all(), "a guard band was written"
        return h[GUARD:GUARD + self.n]

    def untouched(self):
        return (self.get() == self.fill).all()


def dev_indices(idx, reverse_rows=False, pad=0):
    """(device index matrix, row stride, row order): rows stored in reverse order and addressed through ``row_order`` (what
    a ``.T`` view does) with ``reverse_rows``; row stride N + pad, the padding holding values that must never be read."""
    from tt_sketch_amd.device import DevArray
    d, N = idx.shape
    phys = np.full((d, N + pad), -7, dtype=np.int64)
    order = list(range(d))[::-1] if reverse_rows else list(range(d))
    for k in range(d):
        phys[order[k], :N] = idx[k]
    return DevArray.from_host(phys, dtype=np.int64), N + pad, (ctypes.c_int * d)(*order)


def c_index(shape, tidx, tval, reverse_rows=False, pad=0, max_split=0):
    """ttsk_sparse_key_index: (status, dict(keys, vals, splitters: Guarded; N))."""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    d, N = len(shape), tidx.shape[1]
    dev_idx, stride, order = dev_indices(tidx, reverse_rows, pad)
    val = DevArray.from_host(np.asarray(tval, dtype=np.float64))
    lay = c_layout(N, 0, max_split)
    ix = dict(keys=Guarded(N, np.int64), vals=Guarded(N), splitters=Guarded(lay["n_split"], np.int64), N=N, max_split=max_split)
    rc = nat.lib().ttsk_sparse_key_index((ctypes.c_int64 * d)(*shape), d, _ptr(dev_idx), stride, order, ctypes.c_size_t(N), _ptr(val), max_split,
                                         _ptr(ix["keys"]), _ptr(ix["vals"]), _ptr(ix["splitters"]), 0)
    nat.call("ttsk_sync", -1)
    return rc, ix


def c_join(shape, table, qidx, qval, want_out=True, want_dot=True, reverse_rows=False, pad=0):
    """ttsk_sparse_join (``table``: the dict of c_index) or ttsk_dense_join (``table``: a contiguous ndarray of ``shape``):
    (status, out (Nq,) or None, dot or None).  Guard bands around out and dot are checked."""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    d, Nq = len(shape), qidx.shape[1]
    dev_idx, stride, order = dev_indices(qidx, reverse_rows, pad)
    val = DevArray.from_host(np.asarray(qval, dtype=np.float64)) if qval is not None else None
    out, dot = (Guarded(Nq) if want_out else None), (Guarded(1) if want_dot else None)
    tail = ((ctypes.c_int64 * d)(*shape), d, _ptr(dev_idx), stride, order, ctypes.c_size_t(Nq), _ptr(val), _ptr(out), _ptr(dot), 0)
    if isinstance(table, dict):
        rc = nat.lib().ttsk_sparse_join(_ptr(table["keys"]), _ptr(table["vals"]), _ptr(table["splitters"]), ctypes.c_size_t(table["N"]),
                                        table["max_split"], *tail)
    else:
        x = DevArray.from_host(np.ascontiguousarray(table, dtype=np.float64))
        rc = nat.lib().ttsk_dense_join(_ptr(x), *tail)
    nat.call("ttsk_sync", -1)
    if rc:
        assert (out is None or out.untouched()) and (dot is None or dot.untouched())
        return rc, None, None
    return rc, (out.get() if want_out else None), (float(dot.get()[0]) if want_dot else None)


def check_dot(dot, qval, at, lay, what):
    truth, abs_sum = sj.dot_truth(qval, at)
    tol = sj.bound(lay["depth"], abs_sum)
    print(f"{what}: |dot - truth| = {float(abs(dot - truth)):.3e}, bound {tol:.3e} (D = {lay['depth']})")
    assert abs(dot - truth) <= tol, what


# ---- 1. the C entries against the restatement over the shared cases
SPECS = sj.case_list(8192)          # the names and their order do not depend on SJ_MAX_SPLIT; the sizes are read from the library


@pytest.mark.parametrize("i", range(len(SPECS)), ids=[s[0] for s in SPECS])
def test_c_entries_vs_restatement(tsa, i):
    ms = c_layout(0, 0)["max_split"]
    spec = sj.case_list(ms)[i]
    case = sj.make_case(spec)
    shape, name = case["shape"], case["name"]
    rev_t, rev_q, pad_t, pad_q = bool(i & 1), bool(i & 2), (0, 5)[i % 2], (0, 3, 11)[i % 3]
    ref = sj.build_index(case["tidx"], case["tval"], shape, ms)
    rc, ix = c_index(shape, case["tidx"], case["tval"], rev_t, pad_t)
    assert rc == 0
    assert np.array_equal(ix["keys"].get(), ref["keys"]) and np.array_equal(ix["vals"].get(), ref["vals"]), name
    assert np.array_equal(ix["splitters"].get(), ref["splitters"]), name
    qidx, qval = sj.case_queries(case, ref)
    want = sj.join(ref, sj.keys_of(qidx, shape))
    lay = c_layout(len(ref["keys"]), case["Nq"])
    rc, out, dot = c_join(shape, ix, qidx, qval, True, True, rev_q, pad_q)
    assert rc == 0 and np.array_equal(out, want), name
    check_dot(dot, qval, want, lay, name)
    rc2, _, dot2 = c_join(shape, ix, qidx, qval, False, True, rev_q, 0)
    rc3, out3, _ = c_join(shape, ix, qidx, None, True, False, rev_q, pad_q)
    assert rc2 == 0 and rc3 == 0 and np.array_equal(out3, want)
    assert np.float64(dot2).tobytes() == np.float64(dot).tobytes()           # the same bits with and without out
    if case["Nq"] == 0:
        assert dot == 0.0
    if len(ref["keys"]) == 0:
        assert dot == 0.0 and not out.any()
    # the other splitter count of the measurement through the same kernel
    other = 16384 if ms == 8192 else 8192
    rc, ix2 = c_index(shape, case["tidx"], case["tval"], rev_t, pad_t, max_split=other)
    assert rc == 0 and np.array_equal(ix2["splitters"].get(), sj.build_index(case["tidx"], case["tval"], shape, other)["splitters"])
    rc, out, dot4 = c_join(shape, ix2, qidx, qval, True, True, rev_q, pad_q)
    assert rc == 0 and np.array_equal(out, want) and np.float64(dot4).tobytes() == np.float64(dot).tobytes()
    # the dense pass on the same queries
    total = sj.mults(shape)[1]
    if total <= 10 ** 6:
        X = np.random.default_rng(i).standard_normal(shape)
        at = X.ravel()[sj.keys_of(qidx, shape)]
        rc, out, dot = c_join(shape, X, qidx, qval, True, True, rev_q, pad_q)
        assert rc == 0 and np.array_equal(out, at), name
        check_dot(dot, qval, at, lay, name + " dense")
        rc, _, dot2 = c_join(shape, X, qidx, qval, False, True, rev_q, 0)
        assert rc == 0 and np.float64(dot2).tobytes() == np.float64(dot).tobytes()


def test_cases_cover_every_row_order_combination():
    combos = {(bool(i & 1), bool(i & 2)) for i in range(len(SPECS))}
    assert combos == {(False, False), (True, False), (False, True), (True, True)}
    assert {(0, 5)[i % 2] for i in range(len(SPECS))} == {0, 5} and {(0, 3, 11)[i % 3] for i in range(len(SPECS))} == {0, 3, 11}


# ---- 2. the fixture recorded from the reference through the C entries
@pytest.mark.parametrize("case", sj.load_cases(), ids=lambda c: c["name"])
def test_c_entries_vs_reference_fixtures(tsa, case):
    shape = case["shape"]
    ia, va, ib, vb = case["idx_a"], case["val_a"], case["idx_b"], case["val_b"]
    tol = lambda x, y: 1e-12 * float(np.sum(np.abs(x * y))) + 1e-300
    rc, b_ix = c_index(shape, ib, vb)
    rc2, a_ix = c_index(shape, ia, va, reverse_rows=True, pad=2)
    assert rc == 0 and rc2 == 0
    rc, at_a, dot_ab = c_join(shape, b_ix, ia, va)
    assert rc == 0 and abs(dot_ab - case["dot_ab"]) <= tol(va, at_a)
    rc, at_b, dot_ba = c_join(shape, a_ix, ib, vb, reverse_rows=True)
    assert rc == 0 and abs(dot_ba - case["dot_ba"]) <= tol(vb, at_b)
    rc, got, _ = c_join(shape, b_ix, case["gather_idx"], None, True, False, pad=1)
    assert rc == 0 and np.array_equal(got, case["gather_b"])
    # the .T views: the same physical rows addressed in reverse order, keys in the reversed shape
    rc, bT = c_index(shape[::-1], ib[::-1], vb, reverse_rows=True)
    assert rc == 0
    rc, at, dot = c_join(shape[::-1], bT, ia[::-1], va, reverse_rows=True)
    assert rc == 0 and np.array_equal(at, at_a) and abs(dot - case["dot_abT"]) <= tol(va, at)
    if case["dup_a"] == 0:                                      # the reference densifies `a`: of a repeated index the last entry stays
        rc, at, dot = c_join(shape, case["dense"], ia, va)
        assert rc == 0 and abs(dot - case["dot_a_dense"]) <= tol(va, at) and abs(dot - case["dot_dense_a"]) <= tol(va, at)
        rc, at, dot = c_join(shape[::-1], np.ascontiguousarray(case["dense"].T), ia[::-1], va)
        assert rc == 0 and abs(dot - case["dot_aT_denseT"]) <= tol(va, at)


# ---- 3. refusals
def test_every_refusal_leaves_the_outputs_untouched_and_names_its_reason(tsa):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    lib = nat.lib()
    rng = np.random.default_rng(3)
    shape = (6, 7, 8)
    tidx, tval = sj.make_table(rng, shape, 50)
    rc, ix = c_index(shape, tidx, tval)
    assert rc == 0
    qidx, qval = sj.make_queries(rng, shape, sj.build_index(tidx, tval, shape, 8192), 40)
    dev_q, stride, order = dev_indices(qidx)
    val = DevArray.from_host(qval)
    out, dot = Guarded(40), Guarded(1)
    keys, vals, spl = Guarded(50, np.int64), Guarded(50), Guarded(50, np.int64)
    cshape = (ctypes.c_int64 * 3)(*shape)
    N, Nq = ctypes.c_size_t(50), ctypes.c_size_t(40)
    err = lambda: lib.ttsk_last_error().decode()

    def join(keys_=ix["keys"], vals_=ix["vals"], spl_=ix["splitters"], n=N, ms=0, shp=cshape, d=3, q=dev_q, st=stride, ro=order, nq=Nq,
             v=val, o=out, dt=dot):
        return lib.ttsk_sparse_join(_ptr(keys_), _ptr(vals_), _ptr(spl_), n, ms, shp, d, _ptr(q), st, ro, nq, _ptr(v), _ptr(o), _ptr(dt), 0)

    def dense(x=val, shp=cshape, d=3, q=dev_q, st=stride, ro=order, nq=Nq, v=val, o=out, dt=dot):
        return lib.ttsk_dense_join(_ptr(x), shp, d, _ptr(q), st, ro, nq, _ptr(v), _ptr(o), _ptr(dt), 0)

    def index(shp=cshape, d=3, q=dev_q, st=stride, ro=order, n=Nq, v=val, ms=0, k=keys, vs=vals, s=spl):
        return lib.ttsk_sparse_key_index(shp, d, _ptr(q), st, ro, n, _ptr(v), ms, _ptr(k), _ptr(vs), _ptr(s), 0)

    big = (ctypes.c_int64 * 3)(2 ** 31, 2 ** 31, 2)                # 2^63 entries
    for what, call, status, word in [
            ("join: NULL keys", lambda: join(keys_=None), ARG, "NULL"), ("join: NULL values", lambda: join(vals_=None), ARG, "NULL"),
            ("join: NULL splitters", lambda: join(spl_=None), ARG, "NULL"), ("join: NULL shape", lambda: join(shp=None), ARG, "NULL"),
            ("join: NULL queries", lambda: join(q=None), ARG, "NULL"), ("join: no output", lambda: join(o=None, dt=None), ARG, "neither"),
            ("join: dot without entries", lambda: join(v=None), ARG, "dev_qval"), ("join: negative stride", lambda: join(st=-40), ARG, "row_stride"),
            ("join: short stride", lambda: join(st=39), ARG, "row_stride"), ("join: d = 0", lambda: join(d=0), ARG, "positive"),
            ("join: oversize shape", lambda: join(shp=big), UNSUPPORTED, "2^63"),
            ("join: 2^31 nonzeros", lambda: join(n=ctypes.c_size_t(2 ** 31)), UNSUPPORTED, "2^31"),
            ("join: max_split", lambda: join(ms=16385), ARG, "max_split"),
            ("dense: NULL tensor", lambda: dense(x=None), ARG, "NULL"), ("dense: NULL queries", lambda: dense(q=None), ARG, "NULL"),
            ("dense: negative stride", lambda: dense(st=-1), ARG, "row_stride"), ("dense: oversize shape", lambda: dense(shp=big), UNSUPPORTED, "2^63"),
            ("dense: no output", lambda: dense(o=None, dt=None), ARG, "neither"),
            ("index: NULL indices", lambda: index(q=None), ARG, "NULL"), ("index: NULL entries", lambda: index(v=None), ARG, "NULL"),
            ("index: NULL keys", lambda: index(k=None), ARG, "NULL"), ("index: NULL splitters", lambda: index(s=None), ARG, "NULL"),
            ("index: negative stride", lambda: index(st=-40), ARG, "row_stride"), ("index: oversize shape", lambda: index(shp=big), UNSUPPORTED, "2^63"),
            ("index: 2^31 nonzeros", lambda: index(n=ctypes.c_size_t(2 ** 31), st=2 ** 31), UNSUPPORTED, "2^31"),
            ("index: 33 modes", lambda: index(shp=(ctypes.c_int64 * 33)(*[2] * 33), d=33), UNSUPPORTED, "33 modes")]:
        assert call() == status, (what, err())
        assert word in err(), (what, err())
    nat.call("ttsk_sync", -1)
    assert all(g.untouched() for g in (out, dot, keys, vals, spl))
    x = DevArray.from_host(rng.standard_normal(shape))
    assert join() == 0 and dense(x=x) == 0 and index() == 0      # the same calls, complete
    nat.call("ttsk_sync", -1)
    assert not out.untouched() and not dot.untouched() and not keys.untouched()


# ---- 4. the Python surface, with every way to the host closed
def test_api_stays_on_the_device(tsa, monkeypatch):
    from tt_sketch_amd import paths, tensor as tmod
    with paths.forced("kernel"):            # at a few hundred nonzeros the rule of tensor_sparse would keep the host path
        _api_on_the_device(tsa, monkeypatch, tmod)


def _api_on_the_device(tsa, monkeypatch, tmod):
    from tt_sketch_amd.device import DevArray
    rng = np.random.default_rng(11)
    shape = (6,) * 4
    total = 6 ** 4
    flat = rng.choice(total, 500, replace=False)
    i1, i2 = np.stack(np.unravel_index(flat[:300], shape)), np.stack(np.unravel_index(flat[150:500], shape))      # 150 shared
    v1, v2 = rng.standard_normal(300), rng.standard_normal(350)
    X1, X2, D = np.zeros(shape), np.zeros(shape), rng.standard_normal(shape)
    X1[tuple(i1)], X2[tuple(i2)] = v1, v2
    rk = (1, 3, 4, 2, 1)
    cores = [rng.standard_normal((rk[k], 6, rk[k + 1])) for k in range(4)]
    cores2 = [rng.standard_normal((rk[k], 6, rk[k + 1])) for k in range(4)]
    full = lambda cs: np.einsum("aib,bjc,ckd,dle->ijkl", *cs)
    T1, T2 = full(cores), full(cores2)
    gidx = np.concatenate([i1[:, :50], i2[:, -50:], np.stack([rng.integers(0, 6, 30) for _ in shape])], axis=1)

    sp, sp2, dense = tsa.SparseTensor(shape, i1, v1), tsa.SparseTensor(shape, i2, v2), tsa.DenseTensor(D)
    tt, tt2 = tsa.TensorTrain(cores).to_device(), tsa.TensorTrain(cores2).to_device()
    for t in (sp, sp2, dense):
        t.prepare_device()

    def closed(*a, **k):
        raise AssertionError("a host path was taken")
    monkeypatch.setattr(tmod, "_host", closed)
    monkeypatch.setattr(tsa.SparseTensor, "dict", property(closed))
    monkeypatch.setattr(tsa.SparseTensor, "to_numpy", closed)

    dotf = lambda a, b: float(np.dot(a.ravel(), b.ravel()))
    close = lambda got, want, scale: abs(got - want) <= 1e-12 * scale
    s12 = float(np.sum(np.abs(X1 * X2)))
    assert close(sp.dot(sp2), dotf(X1, X2), s12) and close(sp2.dot(sp), dotf(X1, X2), s12) and close(sp.T.dot(sp2.T), dotf(X1, X2), s12)
    assert sp.dot(sp2) == sp.dot(sp2)
    slots = [k for k in sp2._dev[2] if not isinstance(k, int)]                 # the mode permutations keep the integer keys
    assert slots and all(isinstance(k, tuple) and k[0] == "key_index" for k in slots)
    n_idx = len(sp2._dev[2])
    sp.dot(sp2)
    assert len(sp2._dev[2]) == n_idx                            # the index is built once per tensor and row order
    s1d = float(np.sum(np.abs(X1 * D)))
    assert close(sp.dot(dense), dotf(X1, D), s1d) and close(dense.dot(sp), dotf(X1, D), s1d)
    assert close(sp.T.dot(dense.T), dotf(X1, D), s1d)
    assert np.array_equal(sp.gather(gidx), X1[tuple(gidx)]) and np.array_equal(sp.gather(tuple(gidx)), X1[tuple(gidx)])
    got = sp.gather_dev(sp2)
    assert isinstance(got, DevArray) and np.array_equal(got.get(), X1[tuple(i2)])
    assert np.array_equal(sp.T.gather_dev(gidx[::-1]).get(), X1[tuple(gidx)])
    S = T1 + X1
    nrm = tsa.TensorSum([tt, sp]).norm()
    assert abs(nrm - np.linalg.norm(S)) <= 1e-11 * np.linalg.norm(S)
    R = T2 + X1 + X2
    aa, ab, bb = dotf(T1, T1), dotf(T1, R), dotf(R, R)
    want = np.sqrt(aa + bb) * np.sqrt(abs(1 - 2 * ab / (aa + bb))) / np.sqrt(bb)
    assert want > 0.1                                           # far above the floor of the fast formula
    got = tt.error(tsa.TensorSum([tt2, sp, sp2]), fast=True, relative=True)
    assert abs(got - want) <= 1e-10 * want
    s = tsa.TensorSum([tt2, sp, sp2])
    assert abs(s.dot(tsa.TensorSum([tt, sp2])) - dotf(R, T1 + X2)) <= 1e-11 * float(np.sum(np.abs(R * (T1 + X2))) + np.linalg.norm(R) * np.linalg.norm(T1 + X2))


# ---- 5. full size: the C4 shape, two tensors of 10^7 nonzeros that share a known subset of their indices
def test_full_size_dot_of_two_sparse_tensors(tsa):
    shape, N, K = (200,) * 5, 10 ** 7, 2 * 10 ** 6
    rng = np.random.default_rng(2027)
    # distinct keys by construction: odd numbers for a, even ones for what b does not share with it
    ka = 2 * np.cumsum(rng.integers(1, 20000, N, dtype=np.int64)) + 1
    kb = 2 * np.cumsum(rng.integers(1, 20000, N - K, dtype=np.int64))
    assert ka[-1] < 200 ** 5 and kb[-1] < 200 ** 5
    ka = ka[rng.permutation(N)]
    shared = rng.choice(N, K, replace=False)
    perm_b = rng.permutation(N)
    kb = np.concatenate([ka[shared], kb])[perm_b]
    va, vb = rng.standard_normal(N), rng.standard_normal(N)
    where_b = np.empty(N, dtype=np.int64)
    where_b[perm_b] = np.arange(N)                              # position in b of entry j of the concatenation
    at = np.zeros(N)
    at[shared] = vb[where_b[:K]]                                # what a's nonzeros meet in b: the sum over the known subset
    lay = c_layout(N, N)
    rc, ix = c_index(shape, sj.unravel(kb, shape), vb)
    assert rc == 0
    qidx = sj.unravel(ka, shape)
    rc, _, dot1 = c_join(shape, ix, qidx, va, False, True)
    rc2, _, dot2 = c_join(shape, ix, qidx, va, False, True)
    assert rc == 0 and rc2 == 0 and np.float64(dot1).tobytes() == np.float64(dot2).tobytes()
    check_dot(dot1, va, at, lay, "C4, 10^7 x 10^7")
