"""NumPy restatement of ``ttsk_op_apply`` (csrc/op_apply.hip): per term, with operator core M (R, n_in, n_out, R'), train
core C (r, n_in, r') and chain L (R, r, l),

    T1[b, j, l, c] = sum_a    L[b, a, l] C[a, j, c]
    W[l, i, k, c]  = sum_{b,j} M[b, j, i, k] T1[b, j, l, c]          -> (l, n_out, R' r'), columns in (k, c) order

in float64, or in any other dtype for a check of the bound; a term without operator is W[l, i, c] = sum_a L[0, a, l] C[a, i, c].

The same on |operands| gives W_abs, the sum of the absolute values of all terms of W.  Every term passes through two
nested sums, of r and of R n_in terms, and two products, so a float64 computation in any order of those sums satisfies, to
first order in u = 2^-53, |W - W_exact| <= (r + R n_in + 2) u W_abs; the bound used is twice that for the second-order
terms.  tests/test_operator_product_host.py holds float64 NumPy against np.longdouble inside it for every case below.
"""
from typing import NamedTuple, Tuple

import numpy as np

COLS_PER_WORKGROUP = 128       # OP_COLS of csrc/op_apply_plan.h: columns (i, beta') one workgroup accumulates
ROW_CHUNK = 32                 # OP_KC: rows (beta, j) per LDS stage
MAX_TERMS = 24                 # OP_MAX_TERMS


class Term(NamedTuple):
    R: int
    R1: int
    r: int
    r1: int
    n_in: int
    plain: bool = False        # no operator: R = R' = 1, n_in = n_out
    flipped: bool = False      # operator and train core are the transposed views of the mode-reversed product
    gap: int = 0               # untouched columns of W before the term's block


class Case(NamedTuple):
    name: str
    l: int
    n_out: int
    terms: Tuple[Term, ...]
    tail: int = 0              # untouched columns after the last block


# the smallest shapes that reach each edge: r, r', l in {1, 3, 15, 16, 17, 33} (16-tiles, k-blocks of 4), R n_in in
# {1, 31, 32, 33, 65} (chunk edges), n_out R' in {1, 15, 16, 17, 64, 65, 129} and 257 (column tiles; 129 and 257 are past the
# columns of one workgroup: the grid split), n_in != n_out, R != R', the transposed-view strides, terms without operator
# (one of them wider than a column block), three ragged terms with untouched columns between and around them
CASES = [
    Case("ones", 1, 1, (Term(1, 1, 1, 1, 1),)),
    Case("rows31_cols15", 3, 5, (Term(1, 3, 3, 3, 31),)),
    Case("rows32_cols16", 16, 8, (Term(2, 2, 15, 16, 16),)),
    Case("rows33_cols17", 17, 17, (Term(3, 1, 16, 17, 11),)),
    Case("rows65_cols64", 15, 16, (Term(5, 4, 17, 15, 13),)),
    Case("r33_cols65", 33, 13, (Term(1, 5, 33, 33, 7),)),
    Case("cols129_split", 3, 43, (Term(2, 3, 3, 1, 4),)),
    Case("cols257_split", 17, 257, (Term(1, 1, 1, 3, 2),)),
    Case("flipped_views", 5, 6, (Term(3, 2, 4, 7, 5, flipped=True),)),
    Case("plain", 17, 33, (Term(1, 1, 17, 3, 33, plain=True),)),
    Case("plain_cols130_split", 3, 130, (Term(1, 1, 2, 2, 130, plain=True),)),
    Case("ragged3_gaps", 16, 7, (Term(2, 3, 3, 17, 5, gap=2), Term(1, 1, 4, 5, 7, plain=True, gap=3),
                                 Term(4, 1, 16, 1, 9, flipped=True, gap=1)), tail=2),
]


def case_arrays(case: Case):
    """([(L, M or None, C)], column offsets, w_cols): M and C of a flipped term are non-contiguous views"""
    rng = np.random.default_rng(sum(map(ord, case.name)))
    terms, offs, off = [], [], 0
    for t in case.terms:
        L = rng.standard_normal((t.R, t.r, case.l)) / np.sqrt(t.R * t.r)
        if t.flipped:
            C = (rng.standard_normal((t.r1, t.n_in, t.r)) / np.sqrt(t.n_in)).transpose(2, 1, 0)
            M = None if t.plain else rng.standard_normal((t.R1, t.n_in, case.n_out, t.R)).transpose(3, 1, 2, 0)
        else:
            C = rng.standard_normal((t.r, t.n_in, t.r1)) / np.sqrt(t.n_in)
            M = None if t.plain else rng.standard_normal((t.R, t.n_in, case.n_out, t.R1))
        off += t.gap
        terms.append((L, M, C))
        offs.append(off)
        off += t.R1 * t.r1
    return terms, offs, off + case.tail


def w_term(L, M, C, absolute=False, dtype=np.float64):
    """W (or W_abs) of one term, (l, n_out, R' r') of `dtype`"""
    L, C = np.asarray(L, dtype=dtype), np.asarray(C, dtype=dtype)
    if absolute:
        L, C = np.abs(L), np.abs(C)
    if M is None:
        return np.einsum("al,aic->lic", L[0], C)
    M = np.asarray(M, dtype=dtype)
    if absolute:
        M = np.abs(M)
    T1 = np.einsum("bal,ajc->bjlc", L, C)
    W = np.einsum("bjik,bjlc->likc", M, T1)
    return W.reshape(W.shape[0], W.shape[1], -1)


def depth(L, M, C) -> int:
    """summation depth of a term: r + R n_in + 2"""
    return C.shape[0] + L.shape[0] * C.shape[1] + 2


def bound(L, M, C):
    """the entrywise tolerance 2 (r + R n_in + 2) 2^-53 W_abs"""
    return 2.0 * depth(L, M, C) * 2.0 ** -53 * w_term(L, M, C, absolute=True)


def w_from_product(L, M, C):
    """the same W through the explicit product core P[(b a), i, (k c)] of MPO.__call__ ("ijkl,ajb->iaklb")"""
    if M is None:
        return np.einsum("al,aic->lic", L[0], C)
    P = np.einsum("ijkl,ajb->iaklb", M, C)
    return np.einsum("bal,baikc->likc", L, P).reshape(L.shape[2], M.shape[2], -1)
