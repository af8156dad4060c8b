"""The builders of a mode's stream (ttsk_sparse_mode_order, ttsk_sparse_mode_stream, ttsk_sparse_mode_stream_u32 of
csrc/sparse_fused.hip) and the panel form of the sparse Psi (ttsk_sparse_psi, csrc/sparse.hip), each called directly.

The builders move integers, so their outputs equal a NumPy restatement exactly: the flat index of make_index_map
(csrc/sampler_dev.h: mult[0] = 1, mult[i] the running product kept in 32 bits and sign-extended, all modulo 2^64), the sort
key (j << 40) | (suffix & (2^40 - 1)) and a stable argsort of it.

ttsk_sparse_psi flushes run sums with fp64 atomics in no fixed order; with integer data (entries in [-3, 3], rows in [-4, 4],
at most 2^17 terms of at most 48) every partial sum is an exact double whatever the order, so the result equals the int64
reference bit for bit."""
import ctypes

import numpy as np
import pytest

from tests import sparse_cases as sc
from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
STRUCTURES = sc.structures()


# ------------------------------------------------------------------ the restatement
def _wrap32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


def flat_mult(shape):
    """make_index_map: the multipliers as uint64"""
    mult, prod = [1], _wrap32(int(shape[0])) if len(shape) else 0
    for n in shape[1:]:
        mult.append(prod & M64)                              # the 32-bit product, sign-extended
        prod = _wrap32(((prod & M64) * int(n)) & M64)
    return mult[:len(shape)]


def flat_index(idx, rows, shape):
    f = np.zeros(idx.shape[1], dtype=np.uint64)
    for row, m in zip(rows, flat_mult(shape)):
        f += idx[row].astype(np.uint64) * np.uint64(m)       # wraps modulo 2^64, as the device's uint64 arithmetic
    return f


def _ints(v):
    return (ctypes.c_int * max(len(v), 1))(*v)


def _u64(v):
    v = list(v) or [1]
    return (ctypes.c_uint64 * len(v))(*[int(x) for x in v])


def test_flat_mult_restatement_is_the_librarys(tsa):
    from tt_sketch_amd.sparse_fused import _flat_mult
    for shape in ((5,), (3, 4, 5), (46341, 46341, 3), (70000, 70000, 3, 2), (65536, 65536, 4, 7), (40000, 50000, 7, 6)):
        assert flat_mult(shape) == _flat_mult(shape), shape
    assert flat_mult((46341, 46341, 3))[2] == (46341 * 46341 - (1 << 32)) & M64        # negative in 32 bits, sign-extended


# ------------------------------------------------------------------ ttsk_sparse_mode_order
def _order(idx, r_rows, r_shape, mode_row, n):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    N = idx.shape[1]
    perm = DevArray.from_host(np.full(N, -1, dtype=np.int64))
    nat.call("ttsk_sparse_mode_order", DevArray.from_host(idx), N, N, _ints(r_rows), _u64(r_shape), len(r_rows), mode_row, n, perm, 0)
    return perm.get()


def _order_ref(idx, r_rows, r_shape, mode_row):
    suffix = flat_index(idx, r_rows, r_shape)
    key = (idx[mode_row].astype(np.uint64) << np.uint64(40)) | (suffix & np.uint64((1 << 40) - 1))
    return np.argsort(key, kind="stable")


# (name, seed, shape by physical row, N, mode_row, r_rows)
ORDER_CASES = [
    ("duplicates", 1, (6, 4, 3), 5001, 1, [2]),                    # 12 distinct keys over 5001 records: ties keep input order
    ("no-suffix", 2, (6, 40, 3), 777, 1, []),                      # r_m = 0: the last mode
    ("one-record", 3, (6, 4, 3), 1, 0, [2, 1]),
    ("odd", 4, (9, 300, 7, 5), 1237, 1, [3, 2]),
    ("transposed", 5, (9, 300, 7, 5), 1237, 2, [0, 1]),            # reversed row order: the suffix of the transposed tensor
    ("suffix-beyond-40-bits", 6, (70000, 1100, 70000, 70000), 2049, 1, [3, 2, 0]),      # wrapped multipliers, key keeps the low 40 bits
    ("mode-of-2^24", 7, (5, 1 << 24, 9), 3000, 1, [2, 0]),         # the longest mode the key holds
]


@pytest.mark.parametrize("case", ORDER_CASES, ids=[c[0] for c in ORDER_CASES])
def test_mode_order_is_the_stable_argsort_of_the_key(tsa, case):
    name, seed, shape, N, mode_row, r_rows = case
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.integers(0, n, N) for n in shape]).astype(np.int64)
    if name == "mode-of-2^24":
        idx[mode_row, ::7] = (1 << 24) - 1 - rng.integers(0, 3, idx[mode_row, ::7].size)       # indices that need all 24 bits
    got = _order(idx, r_rows, [shape[r] for r in r_rows], mode_row, shape[mode_row])
    want = _order_ref(idx, r_rows, [shape[r] for r in r_rows], mode_row)
    assert np.array_equal(got, want), (name, np.flatnonzero(got != want)[:5])


def test_mode_order_refuses_a_mode_beyond_the_key(tsa):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    idx = DevArray.from_host(np.zeros((2, 8), dtype=np.int64))
    perm = DevArray.from_host(np.full(8, -1, dtype=np.int64))
    with pytest.raises(nat.TtskUnsupported):
        nat.call("ttsk_sparse_mode_order", idx, 8, 8, _ints([1]), _u64([4]), 1, 0, (1 << 24) + 1, perm, 0)
    assert np.all(perm.get() == -1)


# ------------------------------------------------------------------ ttsk_sparse_mode_stream, _u32
def _stream(idx, val, perm, l_rows, l_shape, r_rows, r_shape, mode_row, w32):
    """(fl, fr, jj, vv) of one entry point; the buffers are pre-filled so that a write past record N - 1 shows"""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    N = idx.shape[1]
    half = (N + 1) // 2
    words = half if w32 else N
    fl, fr = (DevArray.from_host(np.full(words, -1, dtype=np.int64)) for _ in range(2))
    jj = DevArray.from_host(np.full(half, -1, dtype=np.int64))
    vv = DevArray.from_host(np.full(N, np.nan))
    nat.call("ttsk_sparse_mode_stream_u32" if w32 else "ttsk_sparse_mode_stream", DevArray.from_host(idx), N,
             None if perm is None else DevArray.from_host(perm.astype(np.int64)), N, _ints(l_rows), _u64(l_shape), len(l_rows),
             _ints(r_rows), _u64(r_shape), len(r_rows), mode_row, DevArray.from_host(val), fl, fr, jj, vv, 0)
    j32 = jj.get().view(np.int32)
    assert N % 2 == 0 or j32[N] == -1, "the int32 record behind the last one was written"
    if w32:
        f = [a.get().view(np.uint32) for a in (fl, fr)]
        assert N % 2 == 0 or all(a[N] == 0xFFFFFFFF for a in f), "the uint32 record behind the last one was written"
        f = [a[:N].astype(np.uint64) for a in f]
    else:
        f = [a.get().view(np.uint64) for a in (fl, fr)]
    return f[0], f[1], j32[:N], vv.get()


# (name, seed, shape by physical row, N, l_rows, mode_row, r_rows, with a permutation, 32-bit records possible)
STREAM_CASES = [
    ("identity", 11, (9, 30, 7, 5), 1000, [0], 1, [3, 2], False, True),
    ("permuted-odd", 12, (9, 30, 7, 5), 1237, [0], 1, [3, 2], True, True),          # odd N: the packed int32 / uint32 tail
    ("first-mode", 13, (9, 30, 7, 5), 515, [], 0, [3, 2, 1], True, True),           # l_m = 0
    ("last-mode", 14, (9, 30, 7, 5), 515, [0, 1, 2], 3, [], False, True),           # r_m = 0
    ("transposed", 15, (9, 30, 7, 5), 301, [3, 2], 1, [0], True, True),
    ("one-record", 16, (9, 30, 7, 5), 1, [0, 1], 2, [3], False, True),
    ("prefix-2^31", 17, (46341, 46341, 3, 5), 901, [0, 1], 2, [3], True, False),    # 46341^2 = 2^31 + 4633 prefixes
    ("wrapped-multiplier", 18, (46341, 46341, 3, 5), 901, [0, 1, 2], 3, [], True, False),     # mult[2] is negative in 32 bits
    ("suffix-2^32", 19, (4, 3, 65536, 65536, 7), 640, [0], 1, [3, 2, 4], False, False),      # 65536^2 wraps to a multiplier of 0
]


@pytest.mark.parametrize("case", STREAM_CASES, ids=[c[0] for c in STREAM_CASES])
def test_mode_stream_records_equal_the_restatement(tsa, case):
    from tt_sketch_amd import _native as nat
    name, seed, shape, N, l_rows, mode_row, r_rows, permuted, small = case
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.integers(0, n, N) for n in shape]).astype(np.int64)
    idx[:, 0] = np.array(shape) - 1                          # the largest flat index of either side
    val = rng.standard_normal(N)
    perm = rng.permutation(N) if permuted else None
    l_shape, r_shape = [shape[r] for r in l_rows], [shape[r] for r in r_rows]
    e = perm if permuted else np.arange(N)
    want = (flat_index(idx, l_rows, l_shape)[e], flat_index(idx, r_rows, r_shape)[e], idx[mode_row, e].astype(np.int32), val[e])
    got = _stream(idx, val, perm, l_rows, l_shape, r_rows, r_shape, mode_row, False)
    for g, w, what in zip(got, want, ("fl", "fr", "jj", "vv")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, what)
    if small:
        got32 = _stream(idx, val, perm, l_rows, l_shape, r_rows, r_shape, mode_row, True)
        for g, w, what in zip(got32, want, ("fl", "fr", "jj", "vv")):
            assert np.array_equal(g, w), (name, "u32", what)
    else:
        with pytest.raises(nat.TtskUnsupported):
            _stream(idx, val, perm, l_rows, l_shape, r_rows, r_shape, mode_row, True)


# ------------------------------------------------------------------ ttsk_sparse_psi
def _psi(idx, perm, val, L, R, l, r, n):
    """ttsk_sparse_psi on a zeroed Psi; idx / perm / L / R None = NULL"""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    dev = lambda a, t: None if a is None else DevArray.from_host(np.ascontiguousarray(a, dtype=t))
    psi = DevArray.zeros((l, n, r))
    nat.call("ttsk_sparse_psi", dev(val, np.float64), dev(idx, np.int64), dev(perm, np.int64), len(val), dev(L, np.float64), l,
             dev(R, np.float64), r, n, psi, 0)
    return psi.get()


def _psi_data(rng, N, l, r, with_l=True, with_r=True):
    val = rng.integers(-3, 4, N)
    L = rng.integers(-4, 5, (N, l)) if with_l else None
    R = rng.integers(-4, 5, (N, r)) if with_r else None
    return val, L, R


def _psi_ref(j, n, val, L, R, l, r):
    N = len(val)
    A = L if L is not None else np.ones((N, l), dtype=np.int64)
    B = R if R is not None else np.ones((N, r), dtype=np.int64)
    return sc.segmented_outer(np.zeros(N, dtype=np.int64) if j is None else j, n, val[:, None] * A, B)


def _assert_psi(got, want, what):
    assert want.dtype == np.int64
    bad = np.argwhere(got != want)
    assert np.array_equal(got, want), (what, len(bad), bad[:4].tolist())


# the scatter kernel takes what the matrix-core kernel does not: a rank beyond 32, or several slices without a permutation
@pytest.mark.parametrize("ranks", [(17, 16), (40, 40), (33, 94)], ids=lambda r: "l%d-r%d" % r)
def test_psi_scatter_kernel_on_the_slice_catalogue(tsa, ranks):
    """Sorted index rows without a permutation.  (17, 16) is 272 output pairs and (40, 40) 1600: the loop over the pairs of a
    workgroup of 256 repeats; (33, 94) is the staging buffer's limit l + r = 127 (there only structures of at most 64 slices:
    Psi has 3102 cells per slice)."""
    l, r = ranks
    for k, st in enumerate(STRUCTURES):
        if (l, r) == (33, 94) and st.n > 64:
            continue
        if (l, r) == (17, 16) and st.n == 1:
            continue                                          # one slice of these ranks is the matrix-core kernel's: below
        rng = np.random.default_rng(2000 + 100 * l + k)
        j = st.j.astype(np.int64)
        val, L, R = _psi_data(rng, j.size, l, r)
        got = _psi(None if st.null_j else j, None, val, L, R, l, r, st.n)
        _assert_psi(got, _psi_ref(j, st.n, val, L, R, l, r), (ranks, st.name))


def test_psi_scatter_kernel_unsorted_and_missing_panels(tsa):
    """N = 2 * 4096 + 65 (three workgroups, the last one short) of unsorted indices over n = 9 slices with perm = NULL;
    Rv = NULL (r = 1) and Lv = NULL (l = 1); l + r beyond the staging buffer is refused and leaves Psi alone."""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    N, n = 2 * 4096 + 65, 9
    for k, (l, r, with_l, with_r) in enumerate(((17, 16, True, True), (40, 1, True, False), (1, 40, False, True), (40, 40, True, True))):
        rng = np.random.default_rng(3000 + k)
        j = rng.integers(0, n, N)
        val, L, R = _psi_data(rng, N, l, r, with_l, with_r)
        _assert_psi(_psi(j, None, val, L, R, l, r, n), _psi_ref(j, n, val, L, R, l, r), (l, r, with_l, with_r))
    fill = np.full((64, 2, 64), 7.0)
    psi = DevArray.from_host(fill)
    ones = DevArray.from_host(np.ones((8, 64)))
    with pytest.raises(ValueError):
        nat.call("ttsk_sparse_psi", DevArray.from_host(np.ones(8)), DevArray.from_host(np.zeros(8, dtype=np.int64)), None, 8, ones, 64, ones, 64,
                 2, psi, 0)
    assert np.array_equal(psi.get(), fill)


@pytest.mark.parametrize("ranks", [(16, 16), (17, 32), (32, 1)], ids=lambda r: "l%d-r%d" % r)
def test_psi_matrix_core_kernel(tsa, ranks):
    """Ranks of one and of two 16-column tiles per side.  One slice (NULL index row, and n = 1 with an index row) at N = 1, 2,
    3, 5 (a k-block short of records) and 257 (a second wave of one record); permuted input whose slices are exactly 32
    long, and N = 257 over 8 slices, through a real permutation."""
    l, r = ranks
    for k, N in enumerate((1, 2, 3, 5, 257)):
        rng = np.random.default_rng(4000 + 100 * l + k)
        val, L, R = _psi_data(rng, N, l, r, True, r > 1)
        want = _psi_ref(None, 1, val, L, R, l, r)
        _assert_psi(_psi(None, None, val, L, R, l, r, 1), want, (ranks, N, "NULL index row"))
        _assert_psi(_psi(np.zeros(N, dtype=np.int64), None, val, L, R, l, r, 1), want, (ranks, N, "n = 1"))
    for k, (N, n, js) in enumerate(((32 * 37, 37, np.repeat(np.arange(37), 32)), (257, 8, np.arange(257) * 8 // 257))):
        rng = np.random.default_rng(4500 + 100 * l + k)
        perm = rng.permutation(N)
        j = np.empty(N, dtype=np.int64)
        j[perm] = js                                        # record pos of the sorted walk is nonzero perm[pos]
        val, L, R = _psi_data(rng, N, l, r, True, r > 1)
        _assert_psi(_psi(j, perm, val, L, R, l, r, n), _psi_ref(j, n, val, L, R, l, r), (ranks, N, n, "permuted"))


def test_psi_single_slice_over_more_than_256_partial_blocks(tsa):
    """N = 70 000 in one slice: 274 waves of 256 records leave a partial block each, sparse_part_reduce_kernel's loop over
    them takes a second trip."""
    rng = np.random.default_rng(5000)
    N, l, r = 70000, 4, 4
    val, L, R = _psi_data(rng, N, l, r)
    _assert_psi(_psi(None, None, val, L, R, l, r, 1), _psi_ref(None, 1, val, L, R, l, r), "NULL index row")
