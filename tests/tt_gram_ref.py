"""NumPy restatement of the Gram matrix of tensor trains, G[p, q] = <A_p, B_q>: the left-to-right chain of
TensorTrain.dot (reference tensor.py:542-557), ``acc <- einsum("ab,aic,bid->cd", acc, A_k, B_k)`` from acc = 1 -- the mode
index i is shared by the two cores -- in float64, or in any other dtype for a check of the bound.

The same chain on |cores| gives G_abs, the sum of the absolute values of all terms of G.  Every term passes through a
summation of depth
    L = sum_k (ra_k + n_k rb_k) + sum_k chunks_k
(product 1 of a mode sums over ra_k, product 2 over the n_k slices and rb_k, the chunk partials of a mode are added one by
one), so a computation in float64 with any order of those sums satisfies, to first order in u = 2^-53,
    |G - G_exact| <= L u G_abs,
and the bound used is twice that for the second-order terms.  tests/test_tt_gram_plan.py holds float64 NumPy against
np.longdouble inside this bound for every case of the GPU test.
"""
from typing import NamedTuple, Optional, Tuple

import numpy as np

MAX_RANK = 128          # the widest rank ttsk_tt_gram covers
MAX_CHUNKS = 64         # tt_gram_plan.h: GRAM_MAX_CHUNKS


class Case(NamedTuple):
    name: str
    shape: Tuple[int, ...]
    ranks_a: Tuple[Tuple[int, ...], ...]     # interior ranks of each train A_p
    ranks_b: Optional[Tuple[Tuple[int, ...], ...]]     # None: B = A (tt_gram(As))


def _u(r, d):
    return (r,) * (d - 1)


# the smallest shapes that reach each edge: ranks 1, 3, 15, 16, 17, 33, 64, 65, 128 per side, unequal pairs, ragged lists,
# modes 1, 2, 7 and one of 37 with a single pair (several chunks), mixed sizes, d = 1, 2, 5, batches 1 x 1, 3 x 2, 1 x 16
CASES = [
    Case("d1_n7", (7,), ((),), ((),)),
    Case("d1_n37_chunks", (37,), ((),), ((),)),
    Case("d2_r1", (2, 7), ((1,),), ((1,),)),
    Case("d2_r3_r17", (7, 2), ((3,),), ((17,),)),
    Case("d2_r15_r16", (1, 7), ((15,),), ((16,),)),
    Case("d5_r3_r17_mixed", (2, 7, 1, 7, 2), (_u(3, 5),), (_u(17, 5),)),
    Case("d5_r16_r65", (2, 2, 7, 2, 2), (_u(16, 5),), (_u(65, 5),)),
    Case("d5_r17_r15", (7, 2, 1, 2, 7), (_u(17, 5),), (_u(15, 5),)),
    Case("d5_r33_r64", (2, 2, 2, 7, 2), (_u(33, 5),), (_u(64, 5),)),
    Case("d5_r65_r33", (2, 1, 2, 2, 7), ((8, 65, 65, 4),), ((4, 33, 33, 2),)),
    Case("d5_r50_r100", (2, 7, 2, 2, 2), ((2, 50, 50, 4),), ((2, 100, 100, 4),)),
    Case("d2_r128_r128", (7, 2), ((128,),), ((128,),)),
    Case("d5_r128_r1", (1, 2, 2, 2, 1), ((1, 128, 128, 1),), ((1, 1, 1, 1),)),
    Case("d5_r64_n37_chunks", (2, 37, 2, 37, 2), ((2, 64, 17, 2),), ((2, 33, 16, 2),)),
    Case("d5_r3_n37_chunks", (37, 2, 37, 2, 37), (_u(3, 5),), (_u(15, 5),)),
    Case("ragged_3x2", (2, 7, 2, 7, 2), ((1, 3, 3, 1), (2, 17, 33, 2), (2, 16, 15, 2)), ((2, 65, 16, 2), (1, 1, 1, 1))),
    Case("ragged_1x16", (7, 2, 7), ((16, 17),), tuple(((1 + 5 * i) % 34 + 1, (3 + 7 * i) % 20 + 1) for i in range(16))),
    Case("sym_4", (2, 7, 2, 7), ((3, 17, 3), (16, 16, 16), (1, 33, 2), (2, 15, 2)), None),
]


def random_cores(rng, shape, ranks):
    """cores (r_k, n_k, r_{k+1}) of a train with the interior ranks given, entries of both signs, O(1) products"""
    rk = (1,) + tuple(ranks) + (1,)
    return [rng.standard_normal((rk[k], n, rk[k + 1])) / np.sqrt(rk[k]) for k, n in enumerate(shape)]


def case_cores(case: Case):
    rng = np.random.default_rng(sum(map(ord, case.name)))
    A = [random_cores(rng, case.shape, r) for r in case.ranks_a]
    B = A if case.ranks_b is None else [random_cores(rng, case.shape, r) for r in case.ranks_b]
    return A, B


def dot(a, b, absolute=False, dtype=np.float64):
    acc = np.ones((1, 1), dtype=dtype)
    for x, y in zip(a, b):
        x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
        if absolute:
            x, y = np.abs(x), np.abs(y)
        t = np.einsum("ab,aic->bic", acc, x)
        acc = np.einsum("bic,bid->cd", t, y)
    return acc[0, 0]


def gram(A, B, absolute=False, dtype=np.float64):
    """(G or G_abs) as a (K, M) array of `dtype`"""
    return np.array([[dot(a, b, absolute, dtype) for b in B] for a in A], dtype=dtype)


def chunks(shape, pairs, n_cu):
    """chunks per pair and mode as tt_gram_plan.h chooses them (held against the header by tests/test_tt_gram_plan.py)"""
    c = min(-(-n_cu // pairs), MAX_CHUNKS)
    return [max(1, min(c, n)) for n in shape]


def depth(A, B, n_cu):
    """(K, M) array of the summation depths L of the pairs"""
    shape = [c.shape[1] for c in A[0]]
    ch = sum(chunks(shape, len(A) * len(B), n_cu))
    return np.array([[sum(x.shape[0] + x.shape[1] * y.shape[0] for x, y in zip(a, b)) + ch for b in B] for a in A], dtype=np.float64)


def bound(A, B, n_cu):
    """the entrywise tolerance 2 L 2^-53 G_abs"""
    return 2.0 * depth(A, B, n_cu) * 2.0 ** -53 * gram(A, B, absolute=True)
