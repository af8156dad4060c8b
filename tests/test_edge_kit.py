"""The shared checks of tests/edge_kit.py on arrays of a few dozen elements (no GPU): each must reject exactly what it is
there to reject.  The seeded-defect tests of the cover modules exercise the same functions through each family's
check_results."""
import numpy as np
import pytest

from tests import edge_kit as kit

PRE, POST = 4, 3


def test_exact_rejects_one_element_and_ignores_the_sign_of_zero():
    want = np.arange(12.0).reshape(3, 4)
    kit.exact(want.copy(), want, "same")
    got = want.copy()
    got[0, 0] = -0.0
    kit.exact(got, want, "-0.0 against 0.0")
    got[2, 1] = np.nextafter(got[2, 1], np.inf)
    with pytest.raises(AssertionError, match=r"1 of 12 elements differ.*\(2, 1\)"):
        kit.exact(got, want, "one element")


def test_bounded_at_over_and_nan():
    hi = np.arange(1.0, 13.0).reshape(3, 4)
    lo = np.full((3, 4), 2.0 ** -60)
    tol = np.full((3, 4), 2.0 ** -40 - 2.0 ** -60)
    got = hi.copy()
    got[1, 2] = hi[1, 2] + 2.0 ** -40                        # a multiple of the ulp of 7: (got - hi) - lo == tol, every step exact
    assert kit.bounded(got, hi, lo, tol, "at tol", 1e-6) == 1.0
    tol[1, 2] = np.nextafter(tol[1, 2], 0.0)                 # the same error, one ulp over its bound
    with pytest.raises(AssertionError, match=r"1 of 12 elements outside the bound.*\(1, 2\)"):
        kit.bounded(got, hi, lo, tol, "just over", 1e-6)
    tol[1, 2] = 2.0 ** -40
    got = hi.copy()
    got[0, 3] = np.nan
    with pytest.raises(AssertionError, match=r"1 of 12 elements outside the bound.*\(0, 3\)"):
        kit.bounded(got, hi, lo, tol, "NaN", 1e-6)
    with pytest.raises(AssertionError, match="outside the bound"):
        kit.bounded(got, hi, lo, np.full((3, 4), np.inf), "NaN under an infinite bound", 1e-6)


def test_bounded_enforces_the_frobenius_bar():
    hi = np.ones((4, 5))
    lo = np.zeros((4, 5))
    got = hi + 1e-3                                           # every element inside its bound, the ratio is 1e-3 (up to rounding)
    tol = np.full((4, 5), 1e-2)
    assert kit.bounded(got, hi, lo, tol, "under the bar", 2e-3) == pytest.approx(0.1)
    with pytest.raises(AssertionError, match="Frobenius ratio"):
        kit.bounded(got, hi, lo, tol, "over the bar", 5e-4)
    kit.bounded(np.full((2, 2), 1e-3), np.zeros((2, 2)), np.zeros((2, 2)), np.full((2, 2), 1e-2), "a zero reference has no ratio", 0.0)


def _two_views():
    """a buffer with two 3 x 2 views of row stride 4, three elements apart: guards before, after, between and inside the rows"""
    views = [(PRE, (3, 2), (4, 1)), (PRE + 13, (3, 2), (4, 1))]
    buf = kit.sentinel_buffer(23, PRE, POST)
    return buf, views


def test_assert_guards_before_after_between_and_inside():
    buf, views = _two_views()
    assert buf.size == PRE + 23 + POST and (buf.view(np.uint64) == kit.SENT).all()
    inside = kit.inside_mask(buf.size, views)
    assert inside.sum() == 12 and inside[PRE] and inside[PRE + 9] and not inside[PRE + 2] and inside[PRE + 13] and inside[PRE + 22]
    kit.assert_guards(buf, views, "fresh")
    for off, shape, strides in views:
        kit.strided(buf, off, shape, strides)[...] = 7.0     # only the inside is written
    kit.assert_guards(buf, views, "inside written")
    for where, i in (("before", PRE - 1), ("first", 0), ("after", PRE + 23), ("last", buf.size - 1), ("between the views", PRE + 11),
                     ("row padding", PRE + 2)):
        bad = buf.copy()
        bad[i] = 0.0
        with pytest.raises(AssertionError, match=r"1 guard / padding elements overwritten, first at buffer index \[%d\]" % i):
            kit.assert_guards(bad, views, where)
    same_value = buf.copy()
    same_value[0] = kit.SENT_F                                # the sentinel written again is no change
    kit.assert_guards(same_value, views, "sentinel rewritten")


def test_guarded_places_the_array_and_fills_the_rest():
    arr = np.arange(6.0).reshape(2, 3)
    b = kit.guarded(arr, PRE, POST, off=1)
    assert b.size == PRE + 1 + 6 + POST and np.array_equal(b[PRE + 1:PRE + 7], arr.reshape(-1))
    kit.assert_guards(b, [(PRE + 1, (6,), (1,))], "guarded")
    p = kit.guarded(arr, PRE, POST, fill=kit.PAD)
    assert (p[:PRE] == kit.PAD).all() and (p[PRE + 6:] == kit.PAD).all() and np.array_equal(p[PRE:PRE + 6], arr.reshape(-1))


def test_assert_untouched_catches_one_element():
    bufs = {"Z": kit.sentinel_buffer(10, PRE, POST), "U": kit.sentinel_buffer(5, PRE, POST)}
    kit.assert_untouched(bufs, "fresh")
    kit.assert_untouched(list(bufs.values()), "fresh, as a list")
    bufs["U"][PRE + 2] = 1.0
    with pytest.raises(AssertionError, match=r"\[U\] was written"):
        kit.assert_untouched(bufs, "one element")
    with pytest.raises(AssertionError, match=r"\[1\] was written"):
        kit.assert_untouched(list(bufs.values()), "one element")


def test_same_bits_tells_the_zeros_apart_and_walks_containers():
    a, b = np.zeros(5), np.zeros(5)
    kit.same_bits(a, b, "zeros")
    b[3] = -0.0
    assert np.array_equal(a, b)
    with pytest.raises(AssertionError, match="differs in its bits"):
        kit.same_bits(a, b, "0.0 against -0.0")
    nan = np.full(3, np.nan)
    kit.same_bits(nan, nan.copy(), "the same NaN")
    kit.same_bits(([a], None), ([a.copy()], None), "nested, no T")
    with pytest.raises(AssertionError, match=r"out\[1\]\[Z\] differs"):
        kit.same_bits(([a], {"Z": a}), ([a], {"Z": b}), "out")
    with pytest.raises(AssertionError, match="2 against 1 pieces"):
        kit.same_bits([a, a], [a], "lengths")
    with pytest.raises(AssertionError, match="missing"):
        kit.same_bits(([a], None), ([a], [a]), "T on one side only")
    with pytest.raises(AssertionError):
        kit.same_bits(np.zeros((2, 3)), np.zeros(6), "shapes")
