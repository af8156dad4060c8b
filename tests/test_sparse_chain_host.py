"""What the one-pass sparse path (sparse_fused.try_sparse_gauss_sketch) accepts now that it takes TensorTrainDRM, its route
and its cost rule, pinned without a device with the recorder of tests/test_fused_acceptance.py: the library is replaced,
allocations, uploads and memsets pass (nothing is dereferenced), and an entry either raises with its name or -- in the tests
that follow a whole ``stream_sketch`` -- is let through until one of the entries the test waits for is reached."""
import json
import os
import sys

import numpy as np
import pytest

import tt_sketch_amd as tsa
from tt_sketch_amd import _native as nat, device, operator_product, paths, sparse_fused

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (6, 5, 4, 7)
C4 = (200, 150, 100, 120, 300)
ACCEPTED = "ttsk_sparse_flat_mult"          # the first entry an accepted call reaches (after the tensor's upload)


class _Reached(Exception):
    """the path got as far as this library entry"""


class _SubTT(tsa.TensorTrainDRM):
    pass


@pytest.fixture
def recorder(monkeypatch):
    ptr, made_up = [1 << 20], set()
    state = dict(stop=None, seen=[])        # stop = None: every entry but the harmless three raises; else only those named

    def call(name, *args):
        state["seen"].append(name)
        if name == "ttsk_malloc":
            ptr[0] += 1 << 20
            made_up.add(ptr[0])
            args[0]._obj.value = ptr[0]
        elif name in ("ttsk_h2d", "ttsk_memset"):
            pass
        elif state["stop"] is None or name in state["stop"]:
            raise _Reached(name)

    class _Lib:
        def __getattr__(self, name):
            raise _Reached(name)

    monkeypatch.setattr(nat, "call", call)
    monkeypatch.setattr(nat, "lib", lambda: _Lib())
    monkeypatch.setattr(device, "_pool", {})
    monkeypatch.setattr(device, "_pool_bytes", {True: 0, False: 0})
    monkeypatch.setattr(operator_product, "_one", None)
    yield state
    monkeypatch.undo()
    held = [f"{name}.{key}" for name, mod in list(sys.modules.items()) if name.startswith("tt_sketch_amd") and mod is not None
            for key, val in vars(mod).items() if isinstance(val, device.DevArray) and val.buf.ptr in made_up]
    assert not held, held


def _tt(shape, rank, transpose, cls=tsa.TensorTrainDRM, cores=None, **kw):
    d = len(shape)
    walk = shape[::-1] if transpose else shape
    rank = rank if isinstance(rank, tuple) else (rank,) * (d - 1)
    rk = (1,) + tuple(kw.get("true_rank", rank))
    if transpose:
        rk = (1,) + tuple(kw.get("true_rank", rank))[::-1]
    if cores is None:
        cores = [np.ones((rk[k], walk[k], rk[k + 1])) for k in range(d - 1)]
    return cls(rank, shape, transpose, seed=1, cores=cores, **kw)


def _drm(kind, shape, rank, transpose):
    if kind == "tt":
        return _tt(shape, rank, transpose)
    if kind == "g":
        return tsa.SparseGaussianDRM(rank, shape, transpose=transpose, seed=2)
    return tsa.SparseSignDRM(rank, shape, transpose=transpose, seed=3)


def _sparse(shape, nnz=50, seed=0):
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.integers(0, n, nnz) for n in shape]).astype(np.int64)
    return tsa.SparseTensor(shape, idx, rng.standard_normal(nnz))


def _outcome(tensor, left, right, method="streaming"):
    try:
        out = sparse_fused.try_sparse_gauss_sketch(tensor, left, right, tsa.SketchMethod(method))
    except _Reached as e:
        return str(e)
    assert out is None
    return None


@pytest.mark.parametrize("route", ["kernel", None])
@pytest.mark.parametrize("lk", ["tt", "g", "s"])
@pytest.mark.parametrize("rk", ["tt", "g", "s"])
def test_every_pairing_of_the_three_kinds_is_accepted(recorder, lk, rk, route, monkeypatch):
    if route is None:                       # whatever the fitted rule says at this size: here it is asked and says "kernel"
        monkeypatch.setattr(sparse_fused, "chain_route_ms", lambda *a: (1.0, 2.0))
    with paths.forced(route):
        assert _outcome(_sparse(SHAPE), _drm(lk, SHAPE, 3, False), _drm(rk, SHAPE, 4, True)) == ACCEPTED


def test_the_route_is_asked_for_pairs_with_a_train_only(recorder, monkeypatch):
    asked = []
    monkeypatch.setattr(sparse_fused, "chain_route_ms", lambda *a: asked.append(a) or (2.0, 1.0))
    T = _sparse(SHAPE)
    assert _outcome(T, _drm("g", SHAPE, 3, False), _drm("s", SHAPE, 4, True)) == ACCEPTED and not asked
    assert _outcome(T, _drm("tt", SHAPE, 3, False), _drm("s", SHAPE, 4, True)) is None and len(asked) == 1     # the panels are cheaper
    (nnz, d, work, panels, panel_fma), = asked
    assert (nnz, d) == (50, 4) and work > 0 and panels == 3 * 3 + 3 * 4 and panel_fma == 3 + 9 + 9      # (the train's levels only)
    with paths.forced("composed"):
        assert _outcome(T, _drm("tt", SHAPE, 3, False), _drm("tt", SHAPE, 4, True)) is None
        assert _outcome(T, _drm("g", SHAPE, 3, False), _drm("g", SHAPE, 4, True)) == ACCEPTED          # not routed
    assert len(asked) == 1


def test_declines_before_anything_touches_the_device(recorder):
    T = _sparse(SHAPE)
    L, R = _tt(SHAPE, 3, False), _tt(SHAPE, 4, True)
    g = _drm("g", SHAPE, 4, True)
    big = (70000, 70000, 4, 3)              # the prefix of mode 2 has 4.9e9 entries: no 32-bit stream
    sliced = _tt(SHAPE, (9, 9, 9), True, rank_min=(2, 2, 2), rank_max=(6, 6, 6), true_rank=(9, 9, 9))
    with paths.forced("kernel"):
        for method in ("orthogonal", "hmt"):
            assert _outcome(T, L, R, method) is None
        declined = {
            "true rank 33": (T, _tt(SHAPE, 33, False), R),
            "true rank 33 on the right, beside a hashed DRM": (T, _drm("s", SHAPE, 3, False), _tt(SHAPE, 33, True)),
            "true rank 40 behind a slice of 4 columns": (T, L, _tt(SHAPE, (40,) * 3, True, rank_min=(2,) * 3, rank_max=(6,) * 3, true_rank=(40,) * 3)),
            "a core short": (T, _tt(SHAPE, 3, False, cores=[np.ones((1, 6, 3)), np.ones((3, 5, 3))]), R),
            "a core more": (T, L, _tt(SHAPE, 4, True, cores=[np.ones((1, 7, 4)), np.ones((4, 4, 4)), np.ones((4, 5, 4)), np.ones((4, 6, 4))])),
            "a core of another shape": (T, _tt(SHAPE, 3, False, cores=[np.ones((1, 6, 3)), np.ones((3, 5, 2)), np.ones((2, 4, 3))]), R),
            "a subclass": (T, L, _tt(SHAPE, 4, True, cls=_SubTT)),
            "a subclass beside a hashed DRM": (T, _tt(SHAPE, 3, False, cls=_SubTT), g),
            "a 64-bit stream": (_sparse(big, 10), _tt(big, 3, False), _tt(big, 4, True)),
            "a 64-bit stream, one train": (_sparse(big, 10), _tt(big, 3, False), _drm("g", big, 4, True)),
            "left transposed": (T, L.T, R),
        }
        for what, (tensor, left, right) in declined.items():
            assert _outcome(tensor, left, right) is None, what
        assert _outcome(T, L, sliced) == ACCEPTED                                  # a rank slice is taken
        assert _outcome(_sparse(big, 10), _drm("g", big, 3, False), _drm("g", big, 4, True)) == ACCEPTED     # hashed pairs keep their 64-bit streams
        assert _outcome(tsa.TensorSum([T, _sparse(SHAPE, 20, 1)]), L, R) == ACCEPTED
        assert _outcome(tsa.TensorSum([T, tsa.TensorTrain([np.ones((1, n, 1)) for n in SHAPE])]), L, R) is None


def test_default_drm_reaches_the_pass_or_the_panels_by_the_route(recorder):
    """stream_sketch(sparse, l, r) with no DRM argument is SparseTensor x TensorTrainDRM"""
    T = _sparse((9, 8, 7, 6), 500)
    for route, entry in (("kernel", "ttsk_sparse_gauss_pass_u32"), ("composed", "ttsk_sparse_ttdrm_step")):
        recorder["stop"], recorder["seen"] = {"ttsk_sparse_gauss_pass_u32", "ttsk_sparse_gauss_pass", "ttsk_sparse_ttdrm_step", "ttsk_sparse_psi"}, []
        with paths.forced(route), pytest.raises(_Reached, match=entry + "$"):
            tsa.stream_sketch(T, 3, 5, seed=7)
        assert "ttsk_fill_normal_many" in recorder["seen"]                        # the default DRMs: trains sampled on the device


def test_start_level_at_c4_is_level_1_on_both_sides():
    nnz = 10 ** 7
    L = sparse_fused._Side(_tt(C4, 10, False), C4, nnz)
    R = sparse_fused._Side(_tt(C4, 15, True), C4[::-1], nnz)
    for S in (L, R):
        assert [S.start_level(k) for k in range(4)] == [0, 1, 1, 1]
        assert S.cost(0) == S.cost(1) == 0 and S.cost(3) == 2 * S.full(0) ** 2 and all(S.covered(k) for k in range(4))
    small = sparse_fused._Side(_tt(C4, 10, False), C4, 300)                    # too few nonzeros for any table
    assert [small.start_level(k) for k in range(4)] == [-1] * 4 and small.cost(1) == 10 + 100


def test_cost_rule_gives_the_measured_winner_at_every_recorded_shape():
    with open(os.path.join(ROOT, "profiles", "sparse_tt_bench.json")) as f:
        rec = json.load(f)
    rows = [r for r in rec["cases"] if r.get("tt_kernel_ms") is not None]
    assert len(rows) >= 5
    for r in rows:
        k, c = sparse_fused.chain_route_ms(r["nnz"], len(r["shape"]), r["chain_fma"], r["panel_cols"], r["panel_fma"])
        want = "kernel" if r["tt_kernel_ms"] <= r["tt_composed_ms"] else "composed"
        print(f"{r['name']}: measured {r['tt_kernel_ms']:.3f} / {r['tt_composed_ms']:.3f} ms, rule {k:.3f} / {c:.3f} ms")
        assert paths.taken(None, k, c) == want, r["name"]
