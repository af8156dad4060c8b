"""Evaluation of TT / CP tensors at index lists on the device: ``ttsk_tt_gather`` / ``ttsk_cp_gather`` (csrc/tt_gather.hip)
and the Python surface built on them (``gather_dev``, ``gather``, ``SparseTensor.dot``, ``support_error``).

Bars (the DRM contractions' arithmetic): ||t_dev - t_ref|| <= 1e-12 ||t_ref||, element by element
|t_dev - t_ref| <= 1e-13 s_e with s_e the same chain on |cores|, each sum within 1e-12 of the sum of its |terms|.
"""
import ctypes

import numpy as np
import pytest

from tests import gather_ref as gr
from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3
MAX_RANK = 256          # the widest TT rank ttsk_tt_gather covers


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ptr)


def c_gather(kind, parts, shape, idx, val=None, want_out=True, want_stats=False, reverse_rows=False, pad=0):
    """One direct call of the C entry: (status, t (N,) or None, sums (3,) or None).  ``reverse_rows``: the index matrix
    is stored with its rows in reverse order and addressed through ``row_order`` (what a ``.T`` view does); ``pad``:
    row stride N + pad."""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    d, N = len(shape), idx.shape[1]
    phys = np.full((d, N + pad), -7, dtype=np.int64)        # the padding must never be read as an index
    order = list(range(d))[::-1] if reverse_rows else list(range(d))
    for k in range(d):
        phys[order[k], :N] = idx[k]
    dev_idx = DevArray.from_host(phys, dtype=np.int64)
    dev = [DevArray.from_host(np.ascontiguousarray(p, dtype=np.float64)) for p in parts]
    dev_val = DevArray.from_host(np.asarray(val, dtype=np.float64)) if val is not None else None
    out = DevArray.from_host(np.full(N, np.nan)) if want_out else None
    stats = DevArray.from_host(np.full(3, np.nan)) if want_stats else None
    cptr = (ctypes.c_void_p * d)(*[p.ptr for p in dev])
    tail = (_ptr(dev_idx), N + pad, (ctypes.c_int * d)(*order), ctypes.c_size_t(N), _ptr(dev_val), _ptr(out), _ptr(stats), 0)
    cshape = (ctypes.c_int64 * d)(*shape)
    if kind == "tt":
        ranks = (ctypes.c_int64 * (d + 1))(*([p.shape[0] for p in parts] + [parts[-1].shape[2]]))
        rc = nat.lib().ttsk_tt_gather(cptr, ranks, cshape, d, *tail)
    else:
        rc = nat.lib().ttsk_cp_gather(cptr, parts[0].shape[1], cshape, d, *tail)
    nat.call("ttsk_sync", -1)
    return rc, (out.get() if want_out and rc == 0 else None), (stats.get() if want_stats and rc == 0 else None)


def check_values(t, ref, scale, what):
    nrm = np.linalg.norm(t - ref)
    worst = float(np.max(np.abs(t - ref) / scale, initial=0.0)) if t.size else 0.0
    print(f"{what}: ||d|| / ||ref|| = {nrm / max(np.linalg.norm(ref), 1e-300):.2e}, max |d_e| / s_e = {worst:.2e}")
    assert np.isfinite(t).all(), what
    assert nrm <= 1e-12 * np.linalg.norm(ref), what
    assert (np.abs(t - ref) <= 1e-13 * scale).all(), what


def check_stats(s, t_ref, val, what):
    ref, terms = gr.stats(t_ref, val)
    print(f"{what}: sums off by {np.abs(s - ref) / np.maximum(terms, 1e-300)} of their |terms|")
    assert (np.abs(s - ref) <= 1e-12 * terms).all(), (what, s, ref)


def random_tt(rng, shape, ranks):
    rk = (1,) + tuple(ranks) + (1,)
    return [rng.standard_normal((rk[k], n, rk[k + 1])) / np.sqrt(rk[k]) for k, n in enumerate(shape)]


def random_idx(rng, shape, N, repeats=0.0):
    idx = np.stack([rng.integers(0, n, N) for n in shape]).astype(np.int64).reshape(len(shape), N)
    m = int(repeats * N)
    if m:
        idx[:, N - m:] = idx[:, rng.integers(0, N - m, m)]
    return idx


# ---- 1. the C entries against runs of the reference
@pytest.mark.parametrize("case", gr.load_cases(), ids=lambda c: c["name"])
def test_c_entries_vs_reference_fixtures(tsa, case):
    idx, val = case["idx"], case["entries"]
    for kind, parts, ref, dot, scale in (
            ("tt", case["cores"], case["tt_gather"], case["dot_tt"], gr.tt_gather(case["cores"], idx, absolute=True)),
            ("cp", case["factors"], case["cp_gather"], case["dot_cp"], gr.cp_gather(case["factors"], idx, absolute=True))):
        rc, t, s = c_gather(kind, parts, case["shape"], idx, val, True, True)
        assert rc == 0
        check_values(t, ref, scale, f"{case['name']} {kind}")
        check_stats(s, ref, val, f"{case['name']} {kind}")
        assert abs(s[0] - dot) <= 1e-12 * np.sum(np.abs(ref * val))


# ---- 2./3. the C entries against the NumPy restatement over a fixed list of shapes
def _shape_list():
    """(name, shape, TT ranks, N, repeats, reverse_rows, pad); seeded, the same on every run."""
    rng = np.random.default_rng(20260)
    out = []
    edge_n = [1, 63, 64, 65]
    for i, r in enumerate([1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 100, MAX_RANK]):      # every edge of the lane-group choice
        small = tuple(int(x) for x in rng.integers(1, 9 if r > 65 else 40, 4))
        out.append((f"rank{r}_uniform", small, (r, r, r), edge_n[i % 4], 0.0, False, 0))
        out.append((f"rank{r}_unequal", small, (max(1, r // 3), r, max(1, r - 1)), 700 if r <= 65 else 130, 0.1, i % 2 == 1, 3))
    out.append(("d1", (300,), (), 1000, 0.3, False, 0))
    out.append(("d1_n0", (5,), (), 0, 0.0, False, 0))
    out.append(("d2", (300, 1), (7,), 65, 0.0, True, 5))
    out.append(("d2_n0", (4, 6), (3,), 0, 0.0, False, 0))
    out.append(("d5_c4_like", (200, 150, 100, 120, 300), (10, 10, 10, 10), 100_000, 0.05, False, 0))
    out.append(("d5_c4_like_T", (300, 120, 100, 150, 200), (10, 12, 9, 10), 100_000, 0.0, True, 17))
    out.append(("d5_unit_modes", (1, 33, 1, 1, 20), (1, 5, 5, 1), 64, 0.0, False, 1))
    out.append(("d12", tuple(int(x) for x in rng.integers(1, 12, 12)), tuple(int(x) for x in rng.integers(1, 20, 11)), 1000, 0.2, True, 1))
    out.append(("d12_wide", tuple(int(x) for x in rng.integers(1, 6, 12)), tuple(int(x) for x in rng.integers(30, 70, 11)), 63, 0.0, False, 0))
    return out


@pytest.mark.parametrize("spec", _shape_list(), ids=lambda s: s[0])
def test_c_entries_vs_restatement(tsa, spec):
    name, shape, ranks, N, repeats, rev, pad = spec
    rng = np.random.default_rng(sum(map(ord, name)))
    cores = random_tt(rng, shape, ranks)
    idx = random_idx(rng, shape, N, repeats)
    val = rng.standard_normal(N)
    ref, scale = gr.tt_gather(cores, idx), gr.tt_gather(cores, idx, absolute=True)
    rc, t, s = c_gather("tt", cores, shape, idx, val, True, True, rev, pad)
    assert rc == 0                                          # in cover: the kernel itself, no fallback in between
    check_values(t, ref, scale, f"{name} tt")
    check_stats(s, ref, val, f"{name} tt")
    R = max(ranks) if ranks else 3
    factors = [rng.standard_normal((n, R)) for n in shape]
    ref, scale = gr.cp_gather(factors, idx), gr.cp_gather(factors, idx, absolute=True)
    rc, t, s = c_gather("cp", factors, shape, idx, val, True, True, rev, pad)
    assert rc == 0
    check_values(t, ref, scale, f"{name} cp")
    check_stats(s, ref, val, f"{name} cp")


def test_rank_out_of_cover_is_refused_by_c_and_composed_by_python(tsa):
    rng = np.random.default_rng(9)
    shape, ranks, N = (6, 5, 7, 4), (40, MAX_RANK + 44, 20), 3000
    cores, idx, val = random_tt(rng, shape, ranks), random_idx(rng, shape, N, 0.1), rng.standard_normal(N)
    rc, _, _ = c_gather("tt", cores, shape, idx, val, True, True)
    assert rc == UNSUPPORTED
    ref, scale = gr.tt_gather(cores, idx), gr.tt_gather(cores, idx, absolute=True)
    tt = tsa.TensorTrain(cores).to_device()
    check_values(tt.gather_dev(idx).get(), ref, scale, "composed gather_dev")
    from tt_sketch_amd import tensor_gather as tmod
    sp = tsa.SparseTensor(shape, idx, val)
    old = tmod._PANEL_BYTES
    try:
        tmod._PANEL_BYTES = 16 * (MAX_RANK + 44) * 1000          # three chunks and a remainder
        check_values(tt.gather(sp), ref, scale, "composed, chunked")
        rs, terms = gr.stats(ref, val)
        assert abs(sp.dot(tt) - rs[0]) <= 1e-12 * terms[0]
        assert abs(tt.support_error(sp) ** 2 - rs[2]) <= 1e-12 * terms[2]
    finally:
        tmod._PANEL_BYTES = old


def test_argument_errors(tsa):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    rng = np.random.default_rng(1)
    shape = (4, 5, 6)
    cores, idx, val = random_tt(rng, shape, (2, 3)), random_idx(rng, shape, 10), rng.standard_normal(10)
    assert c_gather("tt", cores, shape, idx, val, False, False)[0] == nat.TTSK_ERR_ARG          # no output at all
    assert c_gather("tt", cores, shape, idx, None, True, True)[0] == nat.TTSK_ERR_ARG           # sums without entries
    assert c_gather("cp", [rng.standard_normal((n, 2)) for n in shape], shape, idx, None, False, True)[0] == nat.TTSK_ERR_ARG
    bad = [np.concatenate([cores[0], cores[0]], axis=0)] + cores[1:]                              # r_0 = 2
    assert c_gather("tt", bad, shape, idx, val, True, False)[0] == nat.TTSK_ERR_ARG
    assert b"rank" in nat.lib().ttsk_last_error()
    one = DevArray.zeros((8,))
    z = (ctypes.c_int64 * 2)(1, 1)
    assert nat.lib().ttsk_tt_gather(None, z, z, 1, _ptr(one), 8, None, ctypes.c_size_t(1), None, _ptr(one), None, 0) == nat.TTSK_ERR_ARG
    assert nat.lib().ttsk_tt_gather((ctypes.c_void_p * 1)(one.ptr), z, z, 0, _ptr(one), 8, None, ctypes.c_size_t(1), None,
                                    _ptr(one), None, 0) == nat.TTSK_ERR_ARG
    d = 33
    many = (ctypes.c_void_p * d)(*[one.ptr] * d)
    ones = (ctypes.c_int64 * (d + 1))(*[1] * (d + 1))
    assert nat.lib().ttsk_tt_gather(many, ones, ones, d, _ptr(one), 8, None, ctypes.c_size_t(1), None, _ptr(one), None,
                                    0) == UNSUPPORTED


# ---- 4. determinism
@pytest.mark.parametrize("kind", ["tt", "cp"])
def test_same_bits_every_call_with_and_without_out(tsa, kind):
    rng = np.random.default_rng(77)
    shape, N = (50, 40, 30, 20, 60), 300_001
    parts = random_tt(rng, shape, (10, 17, 33, 9)) if kind == "tt" else [rng.standard_normal((n, 21)) for n in shape]
    idx, val = random_idx(rng, shape, N, 0.2), rng.standard_normal(N)
    rc1, t1, s1 = c_gather(kind, parts, shape, idx, val, True, True)
    rc2, t2, s2 = c_gather(kind, parts, shape, idx, val, True, True, pad=9)
    rc3, _, s3 = c_gather(kind, parts, shape, idx, val, False, True)
    rc4, t4, _ = c_gather(kind, parts, shape, idx, None, True, False, reverse_rows=True)
    assert rc1 == rc2 == rc3 == rc4 == 0
    assert t1.tobytes() == t2.tobytes() == t4.tobytes()
    assert s1.tobytes() == s2.tobytes() == s3.tobytes()


# ---- 5. the API end to end, with the host detour closed
def test_api_end_to_end_without_host_detour(tsa, monkeypatch):
    from tt_sketch_amd import tensor as tmod
    from tt_sketch_amd.device import DevArray
    shape, nnz, l, r = (200,) * 5, 200_000, 10, 15
    rng = np.random.default_rng(5)
    idx, val = random_idx(rng, shape, nnz), rng.standard_normal(nnz)
    sp = tsa.SparseTensor(shape, idx, val)
    stt = tsa.stream_sketch(sp, (l,) * 4, (r,) * 4, left_drm=tsa.SparseGaussianDRM(l, shape, False, seed=3),
                            right_drm=tsa.SparseGaussianDRM(r, shape, True, seed=4))
    tt = stt.to_tt()
    assert tt.resident()
    cp_host = [rng.standard_normal((n, 7)) / np.sqrt(n) for n in shape]
    cp = tsa.CPTensor([DevArray.from_host(f) for f in cp_host])

    def closed(a):
        raise AssertionError("host detour: tensor._host was called")

    got = {}
    with monkeypatch.context() as mp:
        mp.setattr(tmod, "_host", closed)
        for tag, t, s in (("tt", tt, sp), ("tt.T", tt.T, sp.T), ("cp", cp, sp), ("cp.T", cp.T, sp.T)):
            got[tag] = dict(gather=t.gather(s), dot=s.dot(t), support=t.support_error(s, relative=True),
                            support_abs=t.support_error(s))
        got["tt"]["error"] = tt.error(sp, fast=True)
        got["tt.T"]["error"] = tt.T.error(sp.T, fast=True)
        got["stt"] = dict(gather=stt.gather(sp), support=stt.support_error(sp, relative=True))
    cores = [c.get() for c in tt.cores]
    xnorm = np.linalg.norm(val)
    for kind, parts, fn in (("tt", cores, gr.tt_gather), ("cp", cp_host, gr.cp_gather)):
        ref, scale = fn(parts, idx), fn(parts, idx, absolute=True)
        rs, terms = gr.stats(ref, val)
        for tag in (kind, kind + ".T"):
            g = got[tag]
            assert isinstance(g["gather"], np.ndarray) and g["gather"].dtype == np.float64 and g["gather"].shape == (nnz,)
            check_values(g["gather"], ref, scale, f"api {tag}")
            assert abs(g["dot"] - rs[0]) <= 1e-12 * abs(rs[0]), (tag, g["dot"], rs[0])
            assert abs(g["support_abs"] - np.sqrt(rs[2])) <= 1e-12 * np.sqrt(rs[2])
            assert abs(g["support"] - np.sqrt(rs[2]) / xnorm) <= 1e-12 * np.sqrt(rs[2]) / xnorm
    ref = gr.tt_gather(cores, idx)
    # the SketchedTensorTrain forwards assemble the train again: the same figures up to that assembly's rounding
    assert np.linalg.norm(got["stt"]["gather"] - got["tt"]["gather"]) <= 1e-9 * np.linalg.norm(got["tt"]["gather"])
    assert abs(got["stt"]["support"] - got["tt"]["support"]) <= 1e-9 * got["tt"]["support"]
    # error(fast=True): norm (QR sweep on the device), ||entries|| and the device dot in the reference's formula
    want = gr.fast_error(tt.norm(), xnorm, gr.stats(ref, val)[0][0], relative=False)
    # (the error is of the order of the norms here, so the formula amplifies nothing; .T repeats the QR sweep on other data)
    for tag in ("tt", "tt.T"):
        assert abs(got[tag]["error"] - want) <= 1e-9 * want, (got[tag]["error"], want)
    # a host train with a resident SparseTensor takes the device path too, an all-host pair stays on the host
    host_tt = tsa.TensorTrain(cores)
    assert abs(sp.dot(host_tt) - got["tt"]["dot"]) <= 1e-12 * abs(got["tt"]["dot"])
    fresh = tsa.SparseTensor(shape, idx[:, :1000], val[:1000])
    assert abs(fresh.dot(tsa.TensorTrain(cores)) - float(ref[:1000] @ val[:1000])) <= 1e-12 * np.sum(np.abs(ref[:1000] * val[:1000]))
    assert fresh._dev is None


# ---- 6. full size
def test_c4_full_size(tsa):
    """The C4 tensor (10^7 nonzeros, shape (200, 150, 100, 120, 300)) against a random resident TT of ranks 10: all three
    sums against the chunked host helper, 10^5 seeded positions element by element.  The host helper takes 3.5 s for
    the 10^7 tuples (chunks of 2^14 tuples, one NumPy thread; 12 s on a slower host), the device pass 3 ms."""
    import time
    shape, nnz = (200, 150, 100, 120, 300), 10_000_000
    rng = np.random.default_rng(44)
    idx = random_idx(rng, shape, nnz)
    val = rng.standard_normal(nnz)
    cores = random_tt(rng, shape, (10,) * 4)
    sp = tsa.SparseTensor(shape, idx, val)
    tt = tsa.TensorTrain(cores).to_device()
    t_dev = tt.gather_dev(sp)
    t0 = time.perf_counter()
    ref = gr.tt_gather(cores, idx)
    print(f"\n[C4 full size] host helper {time.perf_counter() - t0:.1f} s")
    pick = np.random.default_rng(45).choice(nnz, 100_000, replace=False)
    t = t_dev.get()
    check_values(t[pick], ref[pick], gr.tt_gather(cores, idx[:, pick], absolute=True), "C4 10^5 positions")
    assert np.linalg.norm(t - ref) <= 1e-12 * np.linalg.norm(ref)
    rs, terms = gr.stats(ref, val)
    dot, support = sp.dot(tt), tt.support_error(sp)
    assert abs(dot - rs[0]) <= 1e-12 * terms[0]
    assert abs(support ** 2 - rs[2]) <= 1e-12 * terms[2]
    rc, _, s = c_gather("tt", cores, shape, idx, val, False, True)
    assert rc == 0
    check_stats(s, ref, val, "C4 sums")
    assert s[0] == dot and np.sqrt(s[2]) == support
    direct = np.linalg.norm(tt.gather(sp) - val)
    assert abs(support - direct) <= 1e-12 * direct
    assert abs(tt.support_error(sp, relative=True) - direct / np.linalg.norm(val)) <= 1e-12 * direct / np.linalg.norm(val)
