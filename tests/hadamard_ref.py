"""NumPy restatement of ``ttsk_hadamard_apply`` (csrc/hadamard_apply.hip): with the cores X (R, n, R') and Y (r, n, r') of
the two factors and the chain L (R, r, l),

    T1[b, i, l, c] = sum_a L[b, a, l] Y[a, i, c]
    W[l, i, k, c]  = sum_b X[b, i, k] T1[b, i, l, c]          -> (l, n, R' r'), columns in (k, c) order

in float64, or in any other dtype for a check of the bound.

The same on |operands| gives W_abs, the sum of the absolute values of all terms of W.  Every term passes through two
nested sums, of r and of R terms, and two products, so a float64 computation in any order of those sums satisfies, to
first order in u = 2^-53, |W - W_exact| <= (r + R + 2) u W_abs; the bound used is twice that for the second-order terms.
tests/test_hadamard_host.py holds float64 NumPy against np.longdouble inside it for every case below.
"""
from typing import NamedTuple

import numpy as np

# of csrc/hadamard_plan.h (tests/test_hadamard_host.py holds them against the header)
COLS_PER_WORKGROUP = 64        # HD_COLS: values of beta' one workgroup accumulates
BETA_CHUNK = 32                # HD_KC: beta per LDS stage
TILE = 16                      # the (l, a') tile of a workgroup, and a beta' tile: the 16 x 16 matrix instruction
KBLOCK = 4                     # its k extent

# the extents that reach each edge: tiles of 16 and k-blocks of 4 for r, r', l; the chunk edges for R; the beta' tiles,
# half a workgroup's columns and the grid split past them for R'
EDGES_SMALL = (1, KBLOCK - 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
EDGES_R = (1, BETA_CHUNK - 1, BETA_CHUNK, BETA_CHUNK + 1, 2 * BETA_CHUNK + 1)
EDGES_R1 = (1, TILE - 1, TILE, TILE + 1, COLS_PER_WORKGROUP // 2, COLS_PER_WORKGROUP // 2 + 1, COLS_PER_WORKGROUP + 1)
EDGES_N = (1, 2, 5)

# how a core lies in memory: contiguous, the transposed view `TensorTrain.T` hands out, mode-major storage, a column slice
# of a wider array
LAYOUTS = ("c", "flipped", "mode_major", "padded")


class Case(NamedTuple):
    name: str
    R: int
    R1: int
    r: int
    r1: int
    n: int
    l: int
    x_layout: str = "c"
    y_layout: str = "c"
    gap: int = 0               # untouched columns of W before the block
    tail: int = 0              # and after it


def _case(R, R1, r, r1, n, l, tag="", **kw):
    return Case(f"R{R}_cols{R1}_r{r}_{r1}_n{n}_l{l}" + tag, R, R1, r, r1, n, l, **kw)


S, ER, E1 = EDGES_SMALL, EDGES_R, EDGES_R1
CASES = [
    _case(ER[0], E1[0], S[0], S[0], 1, S[0]),
    _case(ER[1], E1[1], S[1], S[1], 2, S[1]),
    _case(ER[2], E1[2], S[2], S[3], 5, S[3]),
    _case(ER[3], E1[3], S[3], S[4], 2, S[4]),
    _case(ER[4], E1[4], S[4], S[2], 1, S[2]),
    _case(ER[0], E1[5], S[5], S[5], 2, S[5]),
    _case(3, E1[6], S[1], S[0], 5, S[1], "_split"),
    _case(3, 2, 4, 7, 5, 5, "_flipped_views", x_layout="flipped", y_layout="flipped"),
    _case(5, TILE + 2, 6, TILE + 1, 2, 4, "_mixed_strides", x_layout="mode_major", y_layout="padded"),
    _case(BETA_CHUNK + 1, 3, 2, 5, 5, TILE + 1, "_mixed_strides", x_layout="padded", y_layout="flipped"),
    _case(2, 3, 3, TILE + 1, 2, TILE, "_gaps_around", gap=2, tail=3),
    _case(BETA_CHUNK + 2, COLS_PER_WORKGROUP + 2, 5, 3, 2, 3, "_gaps_flipped_split", x_layout="flipped", gap=1, tail=1),
]
del S, ER, E1


def _core(rng, shape, layout):
    """a core of `shape` (rank, n, rank') lying in memory as `layout` says; a view of a contiguous base unless "c" """
    a, n, b = shape
    if layout == "c":
        return rng.standard_normal(shape)
    if layout == "flipped":
        return rng.standard_normal((b, n, a)).transpose(2, 1, 0)
    if layout == "mode_major":
        return rng.standard_normal((n, a, b)).transpose(1, 0, 2)
    if layout == "padded":
        return rng.standard_normal((a, n, b + 3))[:, :, 1:1 + b]
    raise ValueError(layout)


def case_arrays(case: Case):
    """(L, X, Y, w_off, w_cols)"""
    rng = np.random.default_rng(sum(map(ord, case.name)))
    L = rng.standard_normal((case.R, case.r, case.l)) / np.sqrt(case.R * case.r)
    X = _core(rng, (case.R, case.n, case.R1), case.x_layout)
    Y = _core(rng, (case.r, case.n, case.r1), case.y_layout)
    return L, X, Y, case.gap, case.gap + case.R1 * case.r1 + case.tail


def w_term(L, X, Y, absolute=False, dtype=np.float64):
    """W (or W_abs), (l, n, R' r') of `dtype`"""
    L, X, Y = (np.asarray(a, dtype=dtype) for a in (L, X, Y))
    if absolute:
        L, X, Y = np.abs(L), np.abs(X), np.abs(Y)
    T1 = np.einsum("bal,aic->bilc", L, Y)
    W = np.einsum("bik,bilc->likc", X, T1)
    return W.reshape(W.shape[0], W.shape[1], -1)


def depth(L, X, Y) -> int:
    """summation depth: r + R + 2"""
    return Y.shape[0] + X.shape[0] + 2


def bound(L, X, Y):
    """the entrywise tolerance 2 (r + R + 2) 2^-53 W_abs"""
    return 2.0 * depth(L, X, Y) * 2.0 ** -53 * w_term(L, X, Y, absolute=True)


def w_from_product(L, X, Y):
    """the same W through the explicit Kronecker core P[(b a), i, (k c)] ("bik,aic->baikc")"""
    P = np.einsum("bik,aic->baikc", X, Y)
    return np.einsum("bal,baikc->likc", L, P).reshape(L.shape[2], X.shape[1], -1)
