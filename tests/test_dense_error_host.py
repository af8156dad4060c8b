"""The error of a tensor train against a dense tensor, the host side: the NumPy restatement (tests/dense_error_ref.py)
against runs of the reference (tests/golden/dense_error_cases.npz), today's host path unchanged, the split plan of the
device pass (``_dense_split``: pure arithmetic) and the argument checks of ``dense_stats``, which must fail before
anything reaches the device."""
import itertools

import numpy as np
import pytest

from tests import dense_error_ref as dr

CASES = dr.load_cases()
IDS = [c["name"] for c in CASES]
TOL = 1e-12


def _close(a, b, tol=TOL):
    assert abs(a - b) <= tol * abs(b), (a, b)


def test_fixture_covers_what_it_should():
    assert {len(c["shape"]) for c in CASES} == {2, 3, 4, 5, 6}
    assert any(1 in c["shape"] for c in CASES) and any(1 in c["rank"] for c in CASES)
    assert any(all(n % 16 for n in c["shape"]) for c in CASES)
    assert sum(c["exact"] for c in CASES) == 1 and sum(c["transposed"] for c in CASES) == 1
    for c in CASES:
        if c["transposed"]:
            assert not c["x"].flags.c_contiguous and c["x_buffer"].flags.c_contiguous
        assert c["exact"] or c["relative"] > 1e-2


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_reproduces_the_reference(case):
    t = dr.full(case["cores"])
    assert t.shape == case["shape"]
    s, terms = dr.stats(t, case["x"])
    got = dr.errors(s, t.size)
    _close(got["dot"], case["dot"])
    _close(got["norm"], case["norm"])
    if case["exact"]:
        # X is the reference's own to_numpy(): the restatement's full() differs from it by rounding only
        assert np.sqrt(s[2]) <= 1e-13 * np.linalg.norm(dr.scale(case["cores"], case["x"]))
        assert case["error"] == 0.0
    else:
        for key in ("error", "relative", "rmse"):
            _close(got[key], case[key])
        _close(got["fast"], case["fast"], 1e-9)             # the formula cancels: relative errors are >= 0.1 here
    assert (terms >= np.abs(s)).all() and (dr.scale(case["cores"], case["x"]) >= np.abs(t - case["x"])).all()
    assert abs(s[2] - (s[1] - 2 * s[0] + s[3])) <= 1e-12 * (terms[1] + 2 * terms[0] + terms[3])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_pair_is_unchanged(case):
    """A host train against a host array: the NumPy path, exactly the reference's figures and nothing uploaded."""
    import tt_sketch_amd as tsa
    tt = tsa.TensorTrain([np.array(c) for c in case["cores"]])
    X = tsa.DenseTensor(case["x"])
    for kw, key in ((dict(), "error"), (dict(relative=True), "relative"), (dict(rmse=True), "rmse")):
        if case["exact"]:
            assert tt.error(X, **kw) <= 1e-13 * case["norm"]
        else:
            _close(tt.error(X, **kw), case[key])
            _close(tt.error(case["x"], **kw), case[key])
    if not case["exact"]:
        _close(tt.error(X, fast=True), case["fast"], 1e-9)
    _close(tt.dot(X), case["dot"])
    _close(X.dot(tt), case["dot"])
    _close(X.norm(), case["norm"])
    assert isinstance(tt.dense().data, np.ndarray)
    assert tt._dev is None and X._dev is None


# ---- the split plan
def _brute(shape, rk):
    d = len(shape)
    best = None
    for k in range(1, d):
        cost = (int(np.prod(shape[:k], dtype=object)) + int(np.prod(shape[k:], dtype=object))) * rk[k - 1]
        if best is None or cost < best[0]:
            best = (cost, k)
    return best


def _random_plans(n, seed):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        d = int(rng.integers(2, 8))
        shape = tuple(int(x) for x in rng.integers(1, 70, d))
        rank = tuple(int(x) for x in rng.integers(1, 130, d - 1))
        yield shape, rank


def test_split_minimises_the_panels():
    from tt_sketch_amd.tensor_dense import _dense_split
    for shape, rank in _random_plans(300, 1):
        plan = _dense_split(shape, rank, 1 << 62)
        cost, k = _brute(shape, rank)
        assert (plan["M"] + plan["N"]) * plan["rho"] == cost and plan["k"] == k, (shape, rank, plan)
        assert plan["M"] * plan["N"] == int(np.prod(shape, dtype=object)) and plan["rho"] == rank[k - 1]
        assert plan["slabs"] == [(0, shape[k])]
    one = _dense_split((37,), (), 1 << 30)
    assert (one["k"], one["M"], one["N"], one["rho"], one["slabs"]) == (0, 1, 37, 1, [(0, 37)])
    c2 = _dense_split((64,) * 5, (40,) * 4, 256 << 20)
    assert (c2["k"], c2["M"], c2["N"], c2["slabs"]) == (2, 64 ** 2, 64 ** 3, [(0, 64)])


def test_split_stays_under_the_budget_and_tiles_the_mode():
    from tt_sketch_amd.tensor_dense import _dense_split
    slabbed = 0
    for shape, rank in _random_plans(400, 2):
        rk = (1,) + rank + (1,)
        cost, k = _brute(shape, rank)
        Np = int(np.prod(shape[k + 1:], dtype=object))
        one_slice = 8 * (int(np.prod(shape[:k], dtype=object)) * rk[k] + Np * rk[k] + rk[k + 1] * Np)
        for budget in (8 * cost, max(one_slice, 8 * cost - 1), max(one_slice, (8 * cost) // 3), one_slice):
            plan = _dense_split(shape, rank, budget)
            M, N, rho, slabs = plan["M"], plan["N"], plan["rho"], plan["slabs"]
            assert plan["k"] == k
            # the slabs tile mode k exactly, in order
            assert slabs[0][0] == 0 and slabs[-1][1] == shape[k]
            assert all(a < b for a, b in slabs) and all(p[1] == q[0] for p, q in zip(slabs, slabs[1:]))
            if len(slabs) == 1 and 8 * (M + N) * rho <= budget:
                continue
            slabbed += 1
            assert 8 * (M + N) * rho > budget                   # slabs only when the plain plan does not fit
            widths = {b - a for a, b in slabs[:-1]} | {slabs[-1][1] - slabs[-1][0]}
            assert len({b - a for a, b in slabs[:-1]}) <= 1 and slabs[-1][1] - slabs[-1][0] <= max(widths)
            for a, b in slabs:
                assert 8 * (M * rho + (b - a) * Np * rho + rk[k + 1] * Np) <= budget
    assert slabbed > 100
    plan = _dense_split((2048,) * 3, (100, 100), 256 << 20)     # the measured d = 3 case: slabs of mode 1
    assert plan["k"] == 1 and len(plan["slabs"]) > 1 and (plan["slabs"][-1][1] - plan["slabs"][-1][0]) <= 2048


def test_split_refuses_what_cannot_fit():
    from tt_sketch_amd.tensor_dense import _dense_split
    with pytest.raises(ValueError, match=r"1000.*budget|budget"):
        _dense_split((1000, 1000, 1000), (50, 50), 1 << 20)
    for shape, rank in itertools.islice(_random_plans(50, 3), 50):
        rk = (1,) + rank + (1,)
        cost, k = _brute(shape, rank)
        Np = int(np.prod(shape[k + 1:], dtype=object))
        one_slice = 8 * (int(np.prod(shape[:k], dtype=object)) * rk[k] + Np * rk[k] + rk[k + 1] * Np)
        if one_slice - 1 >= 8 * cost:
            continue
        with pytest.raises(ValueError) as e:
            _dense_split(shape, rank, one_slice - 1)
        assert str(one_slice) in str(e.value) and str(one_slice - 1) in str(e.value)
    with pytest.raises(ValueError):
        _dense_split((4, 5), (2, 3), 1 << 20)                   # ranks that do not belong to the shape


def test_dense_stats_checks_its_argument_before_any_device_call(monkeypatch):
    import tt_sketch_amd as tsa
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray

    def no_device(*a, **k):
        raise AssertionError("device call before the argument checks")

    monkeypatch.setattr(nat, "call", no_device)
    monkeypatch.setattr(nat, "lib", no_device)
    monkeypatch.setattr(DevArray, "from_host", classmethod(no_device))
    monkeypatch.setattr(DevArray, "empty", classmethod(no_device))
    case = CASES[5]
    tt = tsa.TensorTrain([np.array(c) for c in case["cores"]])
    x = case["x"]
    with pytest.raises(ValueError):
        tt.dense_stats(x[1:])
    with pytest.raises(ValueError):
        tt.dense_stats(tsa.DenseTensor(x.T))
    with pytest.raises(ValueError):
        tt.dense_stats(tsa.DenseTensor(x.reshape(-1)))
    idx = np.zeros((len(case["shape"]), 3), dtype=np.int64)
    with pytest.raises(TypeError):
        tt.dense_stats(tsa.SparseTensor(case["shape"], idx, np.ones(3)))
    with pytest.raises(TypeError):
        tt.dense_stats(tt)
    with pytest.raises(TypeError):
        tt.dense_stats(x.astype(np.float32))
    assert tt._dev is None
