"""The cases, operands and references of the three vector entry points -- ttsk_copy_strided, ttsk_sum_slices, ttsk_axpby
(csrc/vector_ops.hip, host plans in csrc/vector_plan.h).  tests/test_gpu_vector_ops.py runs them on the device;
tests/test_vector_plan.py checks without one that every case meets the condition it is named for (route, cap, trip count)
and that every refusal is the plan's.  Plain module: NumPy only.

The cap constants are read from csrc/vector_plan.h: a constant that moves takes the shapes built from it along.

- copy: the expected image of the WHOLE destination buffer (guards and gaps included) is the sentinel buffer with the view
  assigned by NumPy; elements are random 64-bit patterns, so the comparison is of bits.
- sum_slices: acc = dst or +0.0, then acc += src[b] for ascending b, in NumPy float64 -- the order include/ttsk.h states.  Values
  are m * 2^e, e uniform in [-30, 30]: every case with nb >= 3 must give other bits when summed in descending order
  (sum_reference asserts it), or it could not tell the orders apart.
- axpby: per element one of the three legal roundings of a x + b y (no contraction flag is set: the compiler may fuse either
  product), each computed exactly in fractions.Fraction and rounded once."""
import itertools
import os
import re
import zlib
from collections import namedtuple
from fractions import Fraction

import numpy as np

from tests.edge_kit import PAD, sentinel_buffer, strided

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_H = os.path.join(ROOT, "tt_sketch_amd", "csrc", "vector_plan.h")
GUARD = 64                                   # guard elements in front of and behind every buffer
FAKE_BASE = 0x7F0000000000                   # where the CPU plan test pretends an allocation starts (256-byte aligned, as the device's)


def constants():
    """{name: value} of the integer constants of csrc/vector_plan.h"""
    with open(PLAN_H) as f:
        found = dict(re.findall(r"^constexpr \w+ (\w+) = (\d+);", f.read(), re.M))
    return {k: int(v) for k, v in found.items()}


K = constants()
T = K["VEC_THREADS"]
COPY_STRIDE = T * K["COPY_BLOCKS_MAX"]       # elements of one trip of the copy's grid-stride loop
AXPBY_STRIDE = T * K["AXPBY_BLOCKS_MAX"]
SUM_STRIDE = T * K["SUM_SLICES_BLOCKS_MAX"]  # of the slice sum, in the route's unit (pairs on the vector route)


def c_strides(shape):
    st, acc = [], 1
    for n in reversed(shape):
        st.append(acc)
        acc *= int(n)
    return tuple(reversed(st))


def extent(shape, strides):
    """elements from the first to the last one a view with non-negative strides addresses, 0 for an empty view"""
    if any(n == 0 for n in shape):
        return 0
    return 1 + sum((n - 1) * s for n, s in zip(shape, strides))


def prod(shape):
    return int(np.prod([int(n) for n in shape], dtype=object)) if len(shape) else 1


# ====================================================================================================== ttsk_copy_strided
# shape; element strides and offset (behind the guard) of the source and the destination view
CopyCase = namedtuple("CopyCase", "id shape ss ds soff doff")


def _perm_case(id, base, perm, soff=0, doff=0):
    """a contiguous `base` array read through the permutation `perm`, written contiguously"""
    shape = tuple(base[p] for p in perm)
    return CopyCase(id, shape, tuple(c_strides(base)[p] for p in perm), c_strides(shape), soff, doff)


PRIMES = (2, 3, 5, 7, 11)


def gap_strides(shape):
    """row-major strides with room to spare in every dimension: 2 innermost, one element behind every run further out"""
    ds, acc = [], 2
    for n in reversed(shape):
        ds.append(acc)
        acc = acc * n + 1
    return tuple(reversed(ds))


def copy_cases():
    c = []
    # ndim 0 .. 5, each read through the reversal of a contiguous array
    for nd, base in enumerate(((), (7,), (3, 5), (2, 3, 4), (2, 3, 2, 3), (2, 3, 2, 3, 2))):
        c.append(_perm_case("ndim%d" % nd, base, tuple(reversed(range(nd)))))
    # every digit of the decomposition carries its own prime: all 120 orders
    for perm in itertools.permutations(range(5)):
        c.append(_perm_case("perm-" + "".join(map(str, perm)), PRIMES, perm))
    # identity order into a destination whose every stride leaves a gap (the innermost too), then a reversed read into one
    c.append(CopyCase("dst-gaps", PRIMES, c_strides(PRIMES), gap_strides(PRIMES), 0, 0))
    c.append(CopyCase("dst-gaps-perm", PRIMES[::-1], c_strides(PRIMES)[::-1], gap_strides(PRIMES[::-1]), 1, 1))
    # unit extents at the front, in the middle, at the end (their strides are arbitrary: never multiplied by anything but 0)
    c.append(CopyCase("unit-front", (1, 6, 7), (999, 1, 6), (777, 7, 1), 0, 0))
    c.append(CopyCase("unit-middle", (6, 1, 7), (1, 999, 6), (7, 777, 1), 0, 0))
    c.append(CopyCase("unit-end", (6, 7, 1), (1, 6, 999), (7, 1, 777), 0, 0))
    # bases that are 8-byte aligned only
    c.append(_perm_case("odd-offsets", (9, 13), (1, 0), soff=1, doff=3))
    # a broadcast source
    c.append(CopyCase("broadcast", (3, 5), (0, 1), (5, 1), 0, 0))
    c.append(CopyCase("broadcast-inner", (5, 3), (1, 0), (3, 1), 0, 0))
    # one workgroup short of full, full, one element into the second
    c.append(_perm_case("total%d" % (T - 1), (T - 1,), (0,)))
    c.append(_perm_case("total%d" % T, (T // 16, 16), (1, 0)))
    c.append(_perm_case("total%d" % (T + 1), (T + 1,), (0,)))
    # the cap: exactly one trip of the grid-stride loop, one row more, a partial third trip
    side = int(round(COPY_STRIDE ** 0.5))
    assert side * side == COPY_STRIDE
    c.append(_perm_case("cap", (side, side), (1, 0)))
    c.append(_perm_case("cap+", (side + 1, side), (1, 0)))
    c.append(_perm_case("cap-third-trip", (2 * side + 1, side), (1, 0)))
    return c


def copy_trips(c):
    """trips of the grid-stride loop the busiest thread makes"""
    total = prod(c.shape)
    blocks = min(-(-total // T), K["COPY_BLOCKS_MAX"])
    return -(-total // (blocks * T)) if total else 0


SPECIAL_BITS = (0x7FF0000000000001, 0xFFF0000000000001, 0x7FF8000000000123, 0xFFFFFFFFFFFFFFFF,      # signalling, quiet NaNs with payloads
                0x8000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x7FF0000000000000)      # -0.0, subnormals, +inf


def copy_operands(c, seed):
    """-> (source buffer, fresh destination buffer, expected destination buffer), all uint64 bit patterns viewed as float64"""
    rng = np.random.default_rng(seed)
    sn, dn = extent(c.shape, c.ss), extent(c.shape, c.ds)
    src = rng.integers(0, 1 << 64, size=GUARD + c.soff + sn + GUARD, dtype=np.uint64)
    at = rng.permutation(sn)[:len(SPECIAL_BITS)] + GUARD + c.soff
    src[at] = np.array(SPECIAL_BITS[:len(at)], dtype=np.uint64)
    dst = sentinel_buffer(c.doff + dn, GUARD, GUARD)
    want = dst.copy()
    if prod(c.shape):
        strided(want.view(np.uint64), GUARD + c.doff, c.shape, c.ds)[...] = strided(src, GUARD + c.soff, c.shape, c.ss)
    return src.view(np.float64), dst, want


# refusals and empty calls, the same lists for the plan test and the device.  null: the arguments passed as NULL
Refusal = namedtuple("Refusal", "id args null status fragment")          # status: "arg", "unsupported" or "ok" (nothing to do, no launch)


def copy_refusals():
    r = lambda id, ndim, shape, null, status, fragment: Refusal(id, (ndim, tuple(shape)), frozenset(null), status, fragment)
    return [
        r("ndim-1", -1, (3, 4), (), "arg", "ttsk_copy_strided: ndim = -1"),
        r("ndim6", 6, (2, 2, 2, 2, 2, 2), (), "arg", "ttsk_copy_strided: ndim = 6"),
        r("null-shape", 2, (3, 4), ("shape",), "arg", "ttsk_copy_strided: NULL shape or strides"),
        r("null-dst-strides", 2, (3, 4), ("ds",), "arg", "ttsk_copy_strided: NULL shape or strides"),
        r("null-src-strides", 2, (3, 4), ("ss",), "arg", "ttsk_copy_strided: NULL shape or strides"),
        r("negative-extent", 2, (3, -1), (), "arg", "ttsk_copy_strided: negative extent"),
        r("negative-beside-zero", 3, (0, -2, 3), (), "arg", "ttsk_copy_strided: negative extent"),
        r("null-dst", 2, (3, 4), ("dst",), "arg", "ttsk_copy_strided: NULL dst or src"),
        r("null-src", 1, (5,), ("src",), "arg", "ttsk_copy_strided: NULL dst or src"),
        r("null-dst-ndim0", 0, (), ("dst",), "arg", "ttsk_copy_strided: NULL dst or src"),
        r("overflow-2", 2, (1 << 32, 1 << 31), (), "unsupported", "ttsk_copy_strided: the product of the extents"),
        r("overflow-3", 3, (1 << 21, 1 << 21, 1 << 21), (), "unsupported", "ttsk_copy_strided: the product of the extents"),
        r("overflow-margin", 1, ((1 << 63) - 1,), (), "unsupported", "ttsk_copy_strided: the product of the extents"),
        r("empty", 2, (0, 3), (), "ok", ""),
        r("empty-null", 3, (4, 0, 3), ("dst", "src"), "ok", ""),
        r("empty-huge", 3, (1 << 40, 1 << 40, 0), (), "ok", ""),
    ]


# ======================================================================================================== ttsk_sum_slices
SumCase = namedtuple("SumCase", "id nb n stride acc doff soff")


def sum_vector_route(c):
    """the four conditions of the 16-byte route, as a tuple of booleans: even n, even stride, dst base, src base (the buffers
    themselves start 256-byte aligned, the views GUARD + off elements behind)"""
    return (c.n % 2 == 0, c.stride % 2 == 0, (8 * (GUARD + c.doff)) % 16 == 0, (8 * (GUARD + c.soff)) % 16 == 0)


NBS = (1, 2, 7, 8, 9, 15, 16, 17, 25)


def sum_cases():
    c = []
    for nb in NBS:                                              # the unrolled eight and its tail, on both routes
        for acc in (0, 1):
            c.append(SumCase("v-nb%d-acc%d" % (nb, acc), nb, 514, 514, acc, 0, 0))
            c.append(SumCase("s-nb%d-acc%d" % (nb, acc), nb, 513, 513, acc, 0, 0))
    for n in (2, 2 * T - 2, 2 * T, 2 * T + 2):                  # one pair; a workgroup of pairs short of full, full, one more
        c.append(SumCase("v-n%d" % n, 9, n, n, 0, 0, 0))
    n = 2 * T
    c.append(SumCase("s-odd-n", 9, n + 1, n + 2, 1, 0, 0))      # each condition broken alone
    c.append(SumCase("s-odd-stride", 9, n, n + 1, 0, 0, 0))
    c.append(SumCase("s-dst-off8", 9, n, n, 1, 1, 0))
    c.append(SumCase("s-src-off8", 9, n, n, 0, 0, 1))
    c.append(SumCase("s-n1", 9, 1, 1, 0, 0, 0))
    c.append(SumCase("s-n1-acc", 17, 1, 7, 1, 0, 0))
    c.append(SumCase("v-stride+6", 9, n, n + 6, 1, 0, 0))       # slices with a gap between them (the gap holds 1e300)
    c.append(SumCase("s-stride+6", 9, n - 1, n + 5, 0, 0, 0))
    c.append(SumCase("s-both-off8", 16, n, n, 1, 1, 1))
    return c


def sum_cap_cases():
    """either side of the grid cap on both routes: the last element of a full grid, then a second trip of the loop"""
    c = []
    for nb in (1, 9):
        for n in (2 * SUM_STRIDE, 2 * SUM_STRIDE + 2):
            c.append(SumCase("v-cap-n%d-nb%d" % (n, nb), nb, n, n, nb == 1, 0, 0))
        for n in (SUM_STRIDE - 1, SUM_STRIDE + 1):
            c.append(SumCase("s-cap-n%d-nb%d" % (n, nb), nb, n, n, nb == 9, 0, 0))
    return [x._replace(acc=int(x.acc)) for x in c]


def sum_trips(c):
    n = c.n // 2 if all(sum_vector_route(c)) else c.n
    blocks = min(-(-n // T), K["SUM_SLICES_BLOCKS_MAX"])
    return -(-n // (blocks * T))


def sum_values(rng, size):
    """m * 2^e: m a signed 31-bit integer, e uniform in [-30, 30]"""
    m = rng.integers(-(1 << 30), 1 << 30, size=size, dtype=np.int64).astype(np.float64)
    return np.ldexp(m, rng.integers(-30, 31, size=size, dtype=np.int32))


def sum_operands(c, seed):
    """-> (source buffer, destination buffer as it is before the call, the nb x n slices, the prior dst values or None).
    Around the slices and between them the source holds 1e300; dst holds NaN where accumulate = 0 will write."""
    rng = np.random.default_rng(seed)
    slices = sum_values(rng, (c.nb, c.n))
    prior = sum_values(rng, c.n) if c.acc else None
    if c.n >= 4:                                                # a column of -0.0: +0.0 from a fresh accumulator, -0.0 onto a -0.0
        slices[:, c.n - 1] = -0.0
        if c.acc:
            prior[c.n - 1] = -0.0
    src = np.full(GUARD + c.soff + (c.nb - 1) * c.stride + c.n + GUARD, PAD)
    strided(src, GUARD + c.soff, (c.nb, c.n), (c.stride, 1))[...] = slices
    dst = sentinel_buffer(c.doff + c.n, GUARD, GUARD)
    dst[GUARD + c.doff:GUARD + c.doff + c.n] = prior if c.acc else np.nan
    return src, dst, slices, prior


def sum_reference(c, slices, prior):
    """the stated order; where nb >= 3 the descending order must give other bits somewhere"""
    acc = prior.copy() if c.acc else np.zeros(c.n)
    for b in range(c.nb):
        acc += slices[b]
    if c.nb >= 3:
        rev = prior.copy() if c.acc else np.zeros(c.n)
        for b in reversed(range(c.nb)):
            rev += slices[b]
        assert not np.array_equal(acc.view(np.uint64), rev.view(np.uint64)), "%s cannot tell ascending from descending" % c.id
    return acc


def sum_seed(c):
    """the seed of a case: from its name; a case of one or two elements takes the first seed behind it whose values tell the
    two orders apart (with so few sums that is not a given)"""
    seed = zlib.crc32(c.id.encode())
    while c.n < 4 and c.nb >= 3:
        _, _, slices, prior = sum_operands(c, seed)
        try:
            sum_reference(c, slices, prior)
            break
        except AssertionError:
            seed += 1
    return seed


def sum_refusals():
    r = lambda id, nb, acc, n, null, status, fragment: Refusal(id, (nb, acc, n), frozenset(null), status, fragment)
    return [
        r("null-dst", 3, 0, 8, ("dst",), "arg", "ttsk_sum_slices: NULL dst or src"),
        r("null-src", 3, 0, 8, ("src",), "arg", "ttsk_sum_slices: NULL dst or src"),
        r("null-dst-n0", 3, 0, 0, ("dst",), "arg", "ttsk_sum_slices: NULL dst or src"),
        r("nb0", 0, 0, 8, (), "arg", "ttsk_sum_slices: nb = 0"),
        r("nb-1", -1, 1, 8, (), "arg", "ttsk_sum_slices: nb = -1"),
        r("acc2", 3, 2, 8, (), "arg", "ttsk_sum_slices: accumulate = 2"),
        r("acc-1", 3, -1, 8, (), "arg", "ttsk_sum_slices: accumulate = -1"),
        r("n0", 3, 0, 0, (), "ok", ""),
        r("n0-acc", 3, 1, 0, (), "ok", ""),
    ]


# ============================================================================================================= ttsk_axpby
# alias: x is y.  yfill: what y holds before the call where b == 0 (None: ordinary values)
AxCase = namedtuple("AxCase", "id n a b alias yoff xoff yfill exact")
PI, E = float(np.pi), float(np.e)


def axpby_cases():
    A = lambda id, n, a, b, alias=False, yoff=0, xoff=0, yfill=None, exact=False: AxCase(id, n, a, b, alias, yoff, xoff, yfill, exact)
    c = [A("ab-%d" % i, 4096, a, b) for i, (a, b) in enumerate(((1.0, 1.0), (1.0, -1.0), (1.75, -0.5), (PI, E), (0.0, 1.0)))]
    c += [A("n%d" % n, n, PI, E) for n in (1, T - 1, T, T + 1)]
    for name, b in (("p0", 0.0), ("m0", -0.0)):                 # b == 0 of either sign never reads y
        for fname, fill in (("nan", np.nan), ("pinf", np.inf), ("minf", -np.inf)):
            c.append(A("b%s-y%s" % (name, fname), T + 1, PI, b, yfill=fill))
    c.append(A("alias-b0", 1000, PI, 0.0, alias=True))          # tensor.py: axpby(core, core, c, 0.0)
    c.append(A("alias-2-3", 1000, 2.0, 3.0, alias=True))
    c.append(A("y-off8", 1000, PI, E, yoff=1))
    c.append(A("x-off8", 1000, PI, E, xoff=1))
    c.append(A("both-off8", 1000, 1.75, -0.5, yoff=1, xoff=3))
    for n in (AXPBY_STRIDE, AXPBY_STRIDE + 1, 2 * AXPBY_STRIDE + 3):      # the cap: every rounding exact, NumPy is the reference
        c.append(A("cap-n%d" % n, n, 1.75, -0.5, exact=True))
    return c


def axpby_trips(c):
    blocks = min(-(-c.n // T), K["AXPBY_BLOCKS_MAX"])
    return -(-c.n // (blocks * T))


def axpby_operands(c, seed):
    """-> (x values, y values before the call).  exact: multiples of 1/8 below 2^7; else +-[1, 2) * 2^e, e in [-8, 8]: with the
    coefficients of the table every product and sum stays far inside the normal range, nothing underflows."""
    rng = np.random.default_rng(seed)

    def vals():
        if c.exact:
            return rng.integers(-1023, 1024, size=c.n).astype(np.float64) / 8.0
        v = np.ldexp(1.0 + rng.random(c.n), rng.integers(-8, 9, size=c.n, dtype=np.int32))
        return np.where(rng.random(c.n) < 0.5, -v, v)

    x = vals()
    y = x.copy() if c.alias else (np.full(c.n, c.yfill) if c.yfill is not None else vals())
    return x, y


def _fl(q):
    return float(q)              # Fraction -> float rounds once, to nearest even


def axpby_candidates(a, b, x, y):
    """the legal results per element, as a (k, n) array: fl(fl(a x) + fl(b y)), fma(a, x, fl(b y)), fma(b, y, fl(a x)); with
    b == 0 the one result fl(a x) (y is not read)"""
    if b == 0.0:
        return (a * x)[None, :]
    Fa, Fb = Fraction(a), Fraction(b)
    out = np.empty((3, x.size))
    for i, (xi, yi) in enumerate(zip(x.tolist(), y.tolist())):
        ax, by = Fa * Fraction(xi), Fb * Fraction(yi)
        fax, fby = _fl(ax), _fl(by)
        out[0, i] = fax + fby
        out[1, i] = _fl(ax + Fraction(fby))
        out[2, i] = _fl(by + Fraction(fax))
    return out


def axpby_check(c, got, x, y):
    if c.exact:
        want = c.a * x + c.b * y
        ok = got == want
    else:
        cand = axpby_candidates(c.a, c.b, x, y)
        assert np.isfinite(cand).all() and (np.abs(cand[cand != 0]) > 1e-290).all(), c.id
        ok = (got[None, :] == cand).any(axis=0)
    bad = np.flatnonzero(~ok)
    assert bad.size == 0, "%s: %d of %d elements are none of the legal roundings, first at %d: got %r" % (c.id, bad.size, got.size, bad[0], got[bad[0]])


def axpby_refusals():
    r = lambda id, n, null, status, fragment: Refusal(id, (n,), frozenset(null), status, fragment)
    return [
        r("null-y", 5, ("y",), "arg", "ttsk_axpby: NULL y or x"),
        r("null-x", 5, ("x",), "arg", "ttsk_axpby: NULL y or x"),
        r("n0", 0, (), "ok", ""),
        r("n0-null", 0, ("y", "x"), "ok", ""),
    ]
