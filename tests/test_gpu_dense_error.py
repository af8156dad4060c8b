"""A tensor train against a dense tensor in one device pass: ``ttsk_tt_dense_stats`` / ``ttsk_sumsq``
(csrc/tt_dense_stats.hip) and the Python surface on them (``dense_stats``, ``to_dense_dev``, ``error`` / ``dot`` against a
``DenseTensor``, ``DenseTensor.norm``, ``SketchedTensorTrain.error``).

Bars.  With t = L R in exact arithmetic and s = |L| |R| + |x| (``full(|cores|) + |x|``):
  * the stored tile, element by element: |t_dev - t| <= 1e-13 s_e;
  * the sums  x.t, t.t and x.x: within 1e-12 of the sum of the absolute values of their terms;
  * the residual: |sqrt(S2_dev) - sqrt(S2)| <= 1e-13 ||s||_2 + 1e-12 sqrt(S2).  The first term is what the element bar
    allows by the triangle inequality (|| (t_dev - x) - (t - x) ||_2 <= 1e-13 ||s||_2); it stands in for a bar on S2
    against the sum of its own terms, which an exact recovery (every term zero) could not meet with any rounding at all.
"""
import ctypes

import numpy as np
import pytest

from tests import dense_error_ref as dr
from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3
EXTENTS = (1, 15, 16, 17, 63, 64, 65, 200)
RHOS = (1, 3, 4, 5, 16, 100, 130)


def _ptr(a, off=0):
    return None if a is None else ctypes.c_void_p(a.ptr + 8 * off)


def c_dense(L, R, x=None, want_out=True, want_stats=True, pad=0, accumulate_onto=None):
    """One direct call of the C entry: (status, T (M, N) or None, sums (4,) or None).  ``pad`` > 0: through the entry with
    row strides, x and out being the first N columns of arrays N + pad wide whose other columns hold NaN."""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    (M, rho), N = L.shape, R.shape[1]
    dL, dR = DevArray.from_host(np.ascontiguousarray(L)), DevArray.from_host(np.ascontiguousarray(R))
    wide = lambda a: np.concatenate([a, np.full((M, pad), np.nan)], axis=1) if pad else a
    dx = DevArray.from_host(wide(np.asarray(x, dtype=np.float64).reshape(M, N))) if x is not None else None
    out = DevArray.from_host(np.full((M, N + pad), np.nan)) if want_out else None
    stats = DevArray.from_host(np.full(4, np.nan) if accumulate_onto is None else accumulate_onto) if want_stats else None
    if pad or accumulate_onto is not None:
        rc = nat.lib().ttsk_tt_dense_stats_ld(_ptr(dL), M, _ptr(dR), N, rho, _ptr(dx), N + pad, _ptr(out), N + pad, _ptr(stats),
                                              0 if accumulate_onto is None else 1, 0)
    else:
        rc = nat.lib().ttsk_tt_dense_stats(_ptr(dL), M, _ptr(dR), N, rho, _ptr(dx), _ptr(out), _ptr(stats), 0)
    nat.call("ttsk_sync", -1)
    T = None
    if want_out and rc == 0:
        T = out.get()
        if pad:
            assert np.isnan(T[:, N:]).all(), "columns beyond N were written"
            T = T[:, :N]
    return rc, T, (stats.get() if want_stats and rc == 0 else None)


def check(L, R, x, T, s4, what, quiet=False):
    t = L @ R
    scale = np.abs(L) @ np.abs(R) + np.abs(x)
    if T is not None:
        worst = float(np.max(np.abs(T - t) / np.maximum(scale, 1e-300)))
        if not quiet:
            print(f"{what}: max |t_dev - t| / s_e = {worst:.2e}")
        assert np.isfinite(T).all(), what
        assert (np.abs(T - t) <= 1e-13 * scale).all(), (what, worst)
    if s4 is not None:
        ref, terms = dr.stats(t, x)
        off = np.abs(s4 - ref) / np.maximum(terms, 1e-300)
        res = abs(np.sqrt(s4[2]) - np.sqrt(ref[2]))
        allowed = 1e-13 * np.linalg.norm(scale) + 1e-12 * np.sqrt(ref[2])
        if not quiet:
            print(f"{what}: sums off by {off[[0, 1, 3]]} of their |terms|; residual off by {res:.2e}, allowed {allowed:.2e}")
        assert np.isfinite(s4).all(), what
        for j in (0, 1, 3):
            assert abs(s4[j] - ref[j]) <= 1e-12 * terms[j], (what, j, s4, ref)
        assert res <= allowed, (what, s4[2], ref[2])


def _matricise(case):
    """L, R, x of a fixture case at the bond ``_dense_split`` picks, on the buffer the device would see."""
    from tt_sketch_amd.tensor_dense import _dense_split
    cores, x = case["cores"], case["x_buffer"]
    if case["transposed"]:
        cores = [np.transpose(c, (2, 1, 0)) for c in cores[::-1]]
    shape = tuple(c.shape[1] for c in cores)
    plan = _dense_split(shape, tuple(c.shape[2] for c in cores[:-1]))
    k, M, N, rho = plan["k"], plan["M"], plan["N"], plan["rho"]
    L = dr.full(cores[:k] + [np.eye(rho).reshape(rho, rho, 1)]).reshape(M, rho) if k else np.ones((1, 1))
    Rm = dr.full([np.eye(rho).reshape(1, rho, rho)] + cores[k:]).reshape(rho, N)
    return L, Rm, np.ascontiguousarray(x).reshape(M, N)


# ---- 1. the C entry against runs of the reference and against the restatement
@pytest.mark.parametrize("case", dr.load_cases(), ids=lambda c: c["name"])
def test_c_entry_vs_reference_fixtures(tsa, case):
    L, R, x = _matricise(case)
    rc, T, s4 = c_dense(L, R, x)
    assert rc == 0
    check(L, R, x, T, s4, case["name"])
    scale = np.linalg.norm(dr.scale(case["cores"], case["x"]))
    _, terms = dr.stats(L @ R, x)
    assert abs(np.sqrt(s4[2]) - case["error"]) <= 1e-13 * scale + 1e-12 * case["error"]
    assert abs(np.sqrt(s4[2] / s4[3]) - case["relative"]) <= (1e-13 * scale + 1e-12 * case["error"]) / case["norm"] + 1e-12 * case["relative"]
    assert abs(np.sqrt(s4[2] / x.size) - case["rmse"]) <= (1e-13 * scale + 1e-12 * case["error"]) / np.sqrt(x.size)
    assert abs(s4[0] - case["dot"]) <= 1e-12 * terms[0]
    assert abs(np.sqrt(s4[3]) - case["norm"]) <= 1e-12 * case["norm"]
    if not case["exact"]:
        assert abs(dr.fast_error(s4[1], s4[3], s4[0]) - case["fast"]) <= 1e-9 * case["fast"]


@pytest.mark.parametrize("rho", RHOS)
def test_c_entry_vs_restatement_over_the_edges(tsa, rho):
    rng = np.random.default_rng(1000 + rho)
    for M in EXTENTS:
        for N in EXTENTS:
            L, R = rng.standard_normal((M, rho)), rng.standard_normal((rho, N)) / np.sqrt(rho)
            x = L @ R + 0.1 * rng.standard_normal((M, N))
            pad = 3 if (M + N) % 3 == 0 else 0
            rc, T, s4 = c_dense(L, R, x, pad=pad)
            assert rc == 0
            check(L, R, x, T, s4, f"M={M} N={N} rho={rho} pad={pad}", quiet=True)
    # exact recovery at an edge shape, and the sums alone / the tensor alone
    L, R = rng.standard_normal((65, rho)), rng.standard_normal((rho, 200))
    x = L @ R
    rc, T, s4 = c_dense(L, R, x)
    assert rc == 0
    check(L, R, x, T, s4, f"exact rho={rho}")
    rc, T0, s0 = c_dense(L, R, None, True, True)
    assert rc == 0 and T0.tobytes() == T.tobytes()
    assert s0[0] == 0.0 and s0[3] == 0.0 and s0[2] == s0[1] == s4[1]                 # x = NULL reads as zeros


def test_sumsq(tsa):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    rng = np.random.default_rng(3)
    out = DevArray.from_host(np.full(1, np.nan))
    for n in (0, 1, 63, 2048, 2049, 1_000_003, 9_000_000):
        x = rng.standard_normal(n)
        dx = DevArray.from_host(x) if n else None
        got = []
        for _ in range(2):
            nat.call("ttsk_sumsq", _ptr(dx), ctypes.c_size_t(n), _ptr(out), 0)
            got.append(out.get()[0])
        assert got[0] == got[1]
        assert abs(got[0] - float(x @ x)) <= 1e-12 * float(x @ x)
    assert nat.lib().ttsk_sumsq(None, ctypes.c_size_t(5), _ptr(out), 0) == nat.TTSK_ERR_ARG
    assert nat.lib().ttsk_sumsq(_ptr(out), ctypes.c_size_t(1), None, 0) == nat.TTSK_ERR_ARG


def test_argument_errors(tsa):
    from tt_sketch_amd import _native as nat
    rng = np.random.default_rng(1)
    L, R = rng.standard_normal((5, 3)), rng.standard_normal((3, 7))
    x = rng.standard_normal((5, 7))
    assert c_dense(L, R, x, False, False)[0] == UNSUPPORTED                         # no output at all
    assert b"dev_out" in nat.lib().ttsk_last_error()
    from tt_sketch_amd.device import DevArray
    a = DevArray.zeros((64,))
    for M, N, rho in ((0, 7, 3), (5, 0, 3), (5, 7, 0), (-1, 7, 3)):
        assert nat.lib().ttsk_tt_dense_stats(_ptr(a), M, _ptr(a), N, rho, None, _ptr(a), None, 0) == nat.TTSK_ERR_ARG
    assert nat.lib().ttsk_tt_dense_stats(None, 2, _ptr(a), 2, 2, None, _ptr(a), None, 0) == nat.TTSK_ERR_ARG
    assert nat.lib().ttsk_tt_dense_stats_ld(_ptr(a), 2, _ptr(a), 4, 2, _ptr(a), 3, None, 4, _ptr(a), 0, 0) == nat.TTSK_ERR_ARG


# ---- 2. reproducibility
def test_same_bits_every_call_with_and_without_out(tsa, monkeypatch):
    rng = np.random.default_rng(7)
    L, R = rng.standard_normal((1000, 37)), rng.standard_normal((37, 3001))
    x = L @ R + rng.standard_normal((1000, 3001))
    runs = [c_dense(L, R, x, want_out=bool(i % 2)) for i in range(3)] + [c_dense(L, R, x, pad=5)]
    assert all(r[0] == 0 for r in runs)
    for r in runs[1:]:
        assert np.array_equal(r[2], runs[0][2])
    assert runs[1][1].tobytes() == runs[3][1].tobytes()
    # a slabbed run through the public API, repeated
    from tt_sketch_amd import tensor_dense as tmod
    from tt_sketch_amd.device import DevArray
    shape, rank = (30, 50, 40), (9, 30)
    tt = tsa.TensorTrain.random(shape, rank, seed=5).to_device()
    X = tsa.DenseTensor(DevArray.from_host(rng.standard_normal(shape)))
    monkeypatch.setattr(tmod, "_PANEL_BYTES", 8 * (30 * 9 + 7 * 40 * 9 + 30 * 40))
    assert len(tmod._dense_split(shape, rank, tmod._PANEL_BYTES)["slabs"]) == 8       # 7 x 7 + 1
    a, b = tt.dense_stats(X), tt.dense_stats(X)
    assert np.array_equal(a, b)


# ---- 3. slabs
def test_slabbed_runs_agree_with_the_plain_run(tsa, monkeypatch):
    from tt_sketch_amd import tensor_dense as tmod
    from tt_sketch_amd.device import DevArray
    rng = np.random.default_rng(8)
    shape, rank = (12, 7, 33, 9, 5), (6, 14, 10, 4)
    tt_host = tsa.TensorTrain.random(shape, rank, seed=6)
    cores = [np.asarray(c) for c in tt_host.cores]
    t = dr.full(cores)
    x = t + 0.05 * rng.standard_normal(shape)
    tt, X = tt_host.to_device(), tsa.DenseTensor(DevArray.from_host(x))
    scale = dr.scale(cores, x)
    ref, terms = dr.stats(t, x)
    plain = tmod._dense_split(shape, rank)
    k, M, rho = plain["k"], plain["M"], plain["rho"]
    Np = plain["N"] // shape[k]
    rk = (1,) + rank + (1,)
    seen = set()
    for width in (None, shape[k], 5, 4, 1):                       # 5 and 4 do not divide 33
        if width is not None:
            monkeypatch.setattr(tmod, "_PANEL_BYTES", 8 * (M * rho + width * Np * rho + rk[k + 1] * Np))
        plan = tmod._dense_split(shape, rank, tmod._PANEL_BYTES)
        assert plan["k"] == k
        seen.add(len(plan["slabs"]))
        s4 = tt.dense_stats(X)
        T = tt.to_dense_dev().data.get()
        assert (np.abs(T - t) <= 1e-13 * scale).all(), width
        for j in (0, 1, 3):
            assert abs(s4[j] - ref[j]) <= 1e-12 * terms[j], (width, j)
        assert abs(np.sqrt(s4[2]) - np.sqrt(ref[2])) <= 1e-13 * np.linalg.norm(scale) + 1e-12 * np.sqrt(ref[2])
    assert seen == {1, 7, 9, 33}


# ---- 4. the API end to end, with the host detour closed
def test_api_end_to_end_without_host_detour(tsa, monkeypatch):
    from tt_sketch_amd.device import DevArray
    rng = np.random.default_rng(11)
    shape, rank = (24, 20, 18, 22), (5, 7, 6)
    host_tt = tsa.TensorTrain.random(shape, rank, seed=9)
    cores = [np.asarray(c) for c in host_tt.cores]
    t = dr.full(cores)
    x = t + 0.2 * np.sqrt(np.mean(t * t)) * rng.standard_normal(shape)
    scale = np.linalg.norm(dr.scale(cores, x))
    ref, terms = dr.stats(t, x)
    want = dr.errors(ref, t.size)
    res_bar = 1e-13 * scale + 1e-12 * want["error"]
    tt = host_tt.to_device()
    X = tsa.DenseTensor(DevArray.from_host(x))
    XT = tsa.DenseTensor(DevArray.from_host(x)).T                   # reversed strides on a C-ordered buffer
    assert not XT.data.is_contiguous() and XT.shape == shape[::-1]
    uploaded = tsa.DenseTensor(x.copy())
    uploaded.dev_data()                                              # a host tensor with a current device copy
    l, r = 8, 10                                                     # both above the TT ranks: the recovery is exact
    stt = tsa.stream_sketch(tsa.DenseTensor(DevArray.from_host(t)), (l,) * 3, (r,) * 3,
                            left_drm=tsa.TensorTrainDRM(l, shape, False, seed=1), right_drm=tsa.TensorTrainDRM(r, shape, True, seed=2))
    Tdev = tsa.DenseTensor(DevArray.from_host(t))
    real_get = DevArray.get

    def small_get(self, stream=0):
        assert self.size <= 2048, f"host detour: a device array of {self.size} numbers was downloaded"
        return real_get(self, stream)

    got = {}
    with monkeypatch.context() as mp:
        mp.setattr(DevArray, "get", small_get)
        for tag, a, b in (("dev", tt, X), ("T", tt.T, XT), ("host_tt", host_tt, X), ("uploaded", tt, uploaded),
                          ("host_tt_uploaded", tsa.TensorTrain([c.copy() for c in cores]), uploaded)):
            got[tag] = dict(error=a.error(b), relative=a.error(b, relative=True), rmse=a.error(b, rmse=True),
                            both=a.error(b, relative=True, rmse=True), fast=a.error(b, fast=True),
                            fast_rel=a.error(b, fast=True, relative=True), dot=a.dot(b), rdot=b.dot(a), norm=b.norm(),
                            stats=a.dense_stats(b))
        got["ndarray"] = tt.error(x, relative=True)                  # an ndarray against a resident train
        dense = tt.dense()
        assert isinstance(dense.data, DevArray) and dense.shape == shape
        got["self_error"] = tt.error(dense)
        got["stt"] = stt.error(Tdev, relative=True)
        got["stt_abs"] = stt.error(Tdev)
        # a host-only pair under the same closed door: today's NumPy path, exactly
        fresh_tt, fresh_x = tsa.TensorTrain([c.copy() for c in cores]), tsa.DenseTensor(x.copy())
        host_val = fresh_tt.error(fresh_x, relative=True)
        assert fresh_tt._dev is None and fresh_x._dev is None
    assert host_val == np.linalg.norm(fresh_tt.to_numpy() - x) / float(np.sqrt(abs(np.dot(x.ravel(), x.ravel()))))
    for tag in ("dev", "T", "host_tt", "uploaded", "host_tt_uploaded"):
        g = got[tag]
        print(tag, {k: v for k, v in g.items() if k != "stats"})
        assert abs(g["error"] - want["error"]) <= res_bar, tag
        assert abs(g["relative"] - want["relative"]) <= res_bar / want["norm"] + 1e-12 * want["relative"], tag
        assert abs(g["rmse"] - want["rmse"]) <= res_bar / np.sqrt(t.size), tag
        assert abs(g["both"] - want["relative"] / np.sqrt(t.size)) <= (res_bar / want["norm"] + 1e-12 * want["relative"]) / np.sqrt(t.size), tag
        assert abs(g["fast"] - want["fast"]) <= 1e-9 * want["fast"], tag
        assert abs(g["fast_rel"] - want["fast"] / want["norm"]) <= 1e-9 * want["fast"] / want["norm"], tag
        assert abs(g["dot"] - ref[0]) <= 1e-12 * terms[0] and g["dot"] == g["rdot"] == g["stats"][0], tag
        assert abs(g["norm"] - want["norm"]) <= 1e-12 * want["norm"], tag
        assert g["error"] == np.sqrt(g["stats"][2])
    assert got["dev"]["stats"].tobytes() == got["uploaded"]["stats"].tobytes() == got["host_tt"]["stats"].tobytes()
    assert abs(got["ndarray"] - want["relative"]) <= res_bar / want["norm"] + 1e-12 * want["relative"]
    assert got["self_error"] == 0.0                                  # the same kernel formed both: the same bits
    # the sketched train recovers t exactly (sketch ranks above the TT ranks): host figure of the same assembled cores
    rec = dr.full([c.get() for c in stt.to_tt().cores])
    host_err = np.linalg.norm(rec - t)
    bar = 1e-13 * np.linalg.norm(dr.scale([c.get() for c in stt.to_tt().cores], t)) + 1e-12 * host_err
    print("stt.error", got["stt"], got["stt_abs"], "host", host_err)
    assert abs(got["stt_abs"] - host_err) <= bar
    assert abs(got["stt"] - host_err / np.linalg.norm(t)) <= bar / np.linalg.norm(t) + 1e-12 * got["stt"]
    assert got["stt"] < 1e-9


# ---- 5. full size
def test_c2_full_size(tsa):
    """C2 (dense d = 5, n = 64, 8.59 GB).  X is ``to_dense_dev()`` of a rank-3 train with entries of order 1, so the pass
    over it reproduces every tile bit for bit and the residual is exactly what is planted: about 100 entries are
    overwritten with x + delta_i through one-number device copies, and ``error(X)`` must be sqrt(sum delta_i^2) within the
    residual bar -- with ||s||_2 replaced by its lower bound ||full(|cores|)||_2 (s >= full(|cores|) >= 0 entry by
    entry; a Gram chain on small matrices), which only tightens the bar.  Before that, while X is still an exact rank-3 tensor, it
    is sketched and the recovered train's relative error over all of it -- the figure no test had -- is printed and held,
    like the same figure from spot sums over 10^5 entries, against the recovery bar 1e-9."""
    import time
    from oracle import ttsk_oracle as orc
    from tt_sketch_amd.device import DevArray, copy_into, sync
    rng = np.random.default_rng(2)
    d, n, s = 5, 64, 3
    shape = (n,) * d
    cores = [c * 8.0 for c in orc.random_tt(shape, s, rng)]
    tt = tsa.TensorTrain([DevArray.from_host(c) for c in cores])
    X = tt.to_dense_dev()
    assert isinstance(X.data, DevArray) and X.data.size == n ** d and X.data.is_contiguous()
    probe = X.data[17, 5, 63, 0].get()
    want = (cores[0][0, 17] @ cores[1][:, 5] @ cores[2][:, 63] @ cores[3][:, 0]) @ cores[4][:, :, 0]
    assert probe.shape == (64,) and np.linalg.norm(probe - want) <= 1e-13 * np.linalg.norm(want)
    probe = X.data[0, 63, 1, :, 33].get()
    want = np.einsum("a,anb,b->n", cores[0][0, 0] @ cores[1][:, 63] @ cores[2][:, 1], cores[3], cores[4][:, 33, 0])
    assert np.linalg.norm(probe - want) <= 1e-13 * np.linalg.norm(want)
    s0 = tt.dense_stats(X)
    assert s0[2] == 0.0 and s0[0] == s0[1] == s0[3]
    nrm = tt.norm()
    print(f"\n[C2 full size] t.t = {s0[1]:.17g}, norm()^2 = {nrm ** 2:.17g}")
    assert abs(s0[1] - nrm ** 2) <= 1e-12 * nrm ** 2
    # the recovered train at full size (before anything is planted: X is an exact rank-3 tensor here)
    l, r = 20, 40
    rec = tsa.stream_sketch(X, (l,) * 4, (r,) * 4, left_drm=tsa.TensorTrainDRM(l, shape, False, seed=1),
                            right_drm=tsa.TensorTrainDRM(r, shape, True, seed=2)).to_tt()
    full_err = rec.error(X, relative=True)
    spot = _spot_relative_error(X, [c.get() for c in rec.cores], rng, n)            # 25 faces = 102 400 entries
    print(f"[C2 full size] recovered train: relative error over all 64^5 entries {full_err:.3e}, over 102400 spot entries {spot:.3e}")
    assert full_err < 1e-9 and spot < 1e-9
    del rec
    # plant the residual
    K = 100
    where = np.stack([rng.integers(0, n, K) for _ in range(d)], axis=1)
    where = np.unique(where, axis=0)
    delta = rng.uniform(0.5, 1.5, len(where)) * 1e-4 * rng.choice([-1.0, 1.0], len(where))
    dxx = 0.0
    for idx, dl in zip(where, delta):
        cell = X.data[int(idx[0]), int(idx[1]), int(idx[2]), int(idx[3]), int(idx[4]):int(idx[4]) + 1]
        old = float(cell.get()[0])
        new = old + dl
        copy_into(cell, DevArray.from_host(np.array([new])))
        delta[np.all(where == idx, axis=1)] = new - old              # the delta that was representable
        dxx += new * new - old * old
    planted = float(np.sqrt(np.sum(delta ** 2)))
    gram = np.ones((1, 1))
    for c in cores:
        gram = np.einsum("ij,ika,jkb->ab", gram, np.abs(c), np.abs(c), optimize=True)
    s_low = float(np.sqrt(gram[0, 0]))
    sync()
    t0 = time.perf_counter()
    err = tt.error(X)
    t_err = time.perf_counter() - t0
    s1 = tt.dense_stats(X)
    print(f"[C2 full size] error(X) = {err:.17g}, planted {planted:.17g}, off by {abs(err - planted):.2e}, allowed "
          f"{1e-13 * s_low + 1e-12 * planted:.2e}; error() took {t_err * 1e3:.1f} ms including the panels")
    assert abs(err - planted) <= 1e-13 * s_low + 1e-12 * planted
    assert s1[1] == s0[1]
    assert abs(s1[3] - (s0[3] + dxx)) <= 1e-12 * s1[3]               # the closed form of x.x
    assert abs(X.norm() ** 2 - s1[3]) <= 1e-12 * s1[3]
    assert abs(tt.error(X, relative=True) - planted / np.sqrt(s1[3])) <= (1e-13 * s_low + 1e-12 * planted) / np.sqrt(s1[3])


def _spot_relative_error(X, rec_cores, rng, n, faces=25):
    """sqrt(sum (t - x)^2 / sum x^2) over ``faces`` random (n x n) faces of the last two modes."""
    num = den = 0.0
    for _ in range(faces):
        i0, i1, i2 = (int(v) for v in rng.integers(0, n, 3))
        face = X.data[i0, i1, i2].get()
        left = rec_cores[0][0, i0] @ rec_cores[1][:, i1] @ rec_cores[2][:, i2]
        got = np.einsum("a,anb,bm->nm", left, rec_cores[3], rec_cores[4][:, :, 0])
        num += float(np.sum((got - face) ** 2))
        den += float(np.sum(face ** 2))
    return float(np.sqrt(num / den))
