"""Evaluation at index lists, the host side: the NumPy restatement (tests/gather_ref.py) and today's host ``gather`` /
``SparseTensor.dot`` / ``error(fast=True)`` against runs of the reference (tests/golden/gather_cases.npz), and the
argument checks of ``gather_dev``, which must fail before anything reaches the device."""
import numpy as np
import pytest

from tests import gather_ref as gr

CASES = gr.load_cases()
IDS = [c["name"] for c in CASES]
TOL = 1e-13


def _close(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.max(np.abs(a - b), initial=0.0) <= TOL * np.max(np.abs(b), initial=0.0), (a, b)


def test_fixture_covers_what_it_should():
    assert {c["idx"].shape[1] for c in CASES} >= {1, 63, 64, 65}
    assert {len(c["shape"]) for c in CASES} == {2, 3, 4, 5, 6, 7}
    assert any(1 in c["shape"] for c in CASES) and any(c["cores"][1].shape[0] == 1 for c in CASES)
    assert any(len({tuple(col) for col in c["idx"].T}) < c["idx"].shape[1] for c in CASES)      # repeated tuples
    assert all(c["error"] > 1e-2 for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_reproduces_the_reference(case):
    t = gr.tt_gather(case["cores"], case["idx"], chunk=50)          # several chunks
    _close(t, case["tt_gather"])
    _close(gr.tt_gather(case["cores"], case["idx"]), case["tt_gather"])
    c = gr.cp_gather(case["factors"], case["idx"], chunk=50)
    _close(c, case["cp_gather"])
    _close(gr.stats(t, case["entries"])[0][0], case["dot_tt"])
    _close(gr.stats(c, case["entries"])[0][0], case["dot_cp"])
    norm = gr.tt_norm(case["cores"])
    _close(norm, case["norm"])
    _close(gr.fast_error(norm, np.linalg.norm(case["entries"]), case["dot_tt"]), case["error"])
    # the scale of the element-wise bound dominates the values
    assert (gr.tt_gather(case["cores"], case["idx"], absolute=True) >= np.abs(t)).all()
    # sum (t - x)^2 is the expansion of the other two sums
    s, _ = gr.stats(t, case["entries"])
    assert abs(s[2] - (s[1] - 2 * s[0] + case["entries"] @ case["entries"])) <= 1e-12 * (s[1] + abs(s[0]) + s[2])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_gather_is_unchanged(case):
    import tt_sketch_amd as tsa
    tt = tsa.TensorTrain([np.array(c) for c in case["cores"]])
    cp = tsa.CPTensor([np.array(f) for f in case["factors"]])
    sp = tsa.SparseTensor(case["shape"], case["idx"], case["entries"])
    _close(tt.gather(case["idx"]), case["tt_gather"])
    _close(tt.gather(tuple(case["idx"])), case["tt_gather"])
    _close(cp.gather(tuple(case["idx"])), case["cp_gather"])
    _close(sp.dot(tt), case["dot_tt"])
    _close(sp.dot(cp), case["dot_cp"])
    _close(tt.norm(), case["norm"])
    _close(tt.error(sp, fast=True, relative=True), case["error"])
    assert sp._dev is None and tt._dev is None and cp._dev is None          # nothing was uploaded on the way


def test_gather_dev_checks_indices_before_any_device_call(monkeypatch):
    import tt_sketch_amd as tsa
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray

    def no_device(*a, **k):
        raise AssertionError("device call before the index checks")

    monkeypatch.setattr(nat, "call", no_device)
    monkeypatch.setattr(nat, "lib", no_device)
    monkeypatch.setattr(DevArray, "from_host", classmethod(no_device))
    monkeypatch.setattr(DevArray, "empty", classmethod(no_device))
    case = CASES[3]
    shape = case["shape"]
    for t in (tsa.TensorTrain([np.array(c) for c in case["cores"]]), tsa.CPTensor([np.array(f) for f in case["factors"]])):
        for mode in range(len(shape)):
            bad = case["idx"].copy()
            bad[mode, 7] = shape[mode]
            with pytest.raises(IndexError):
                t.gather_dev(bad)
            with pytest.raises(IndexError):
                t.gather_dev(tuple(bad))
            bad[mode, 7] = -1
            with pytest.raises(IndexError):
                t.gather_dev(bad)
        with pytest.raises(ValueError):
            t.gather_dev(case["idx"][:-1])
        with pytest.raises(ValueError):
            t.gather_dev(tuple(case["idx"]) + (case["idx"][0],))
        with pytest.raises(ValueError):
            t.gather_dev(case["idx"][0])
        with pytest.raises(ValueError):                                   # a SparseTensor of another shape
            t.gather_dev(tsa.SparseTensor(shape[::-1], case["idx"][::-1], case["entries"]))
        with pytest.raises(IndexError):                                   # an index outside the SparseTensor's own shape
            bad = case["idx"].copy()
            bad[0, 0] = shape[0]
            t.support_error(tsa.SparseTensor(shape, bad, case["entries"]))
        assert t._dev is None
