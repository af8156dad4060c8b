"""NumPy restatement of ``ttsk_op_close`` (csrc/op_close.hip): with the cores N (S, n_in, n_out, S') of the operator and
Y (s, n_in, s') of the train of the second product and Wl ((c gamma), i, p), what ``ttsk_op_apply`` made of the chain,

    T1[c, j, p, gamma'] = sum_{gamma, i} Wl[(c S + gamma), i, p] N[gamma, j, i, gamma']
    G'[p, c', gamma']   = sum_j sum_c Y[c, j, c'] T1[c, j, p, gamma']                  -> (P, s' S'), columns in (c', gamma') order

in float64, or in any other dtype for a check of the bound.

The same on |operands| gives G'_abs, the sum of the absolute values of all terms of G' (with ``accumulate``, of what ``out``
held as well).  The argument is that of tests/hadamard_close_ref.py: every term passes through three nested sums -- of
S n_out terms (the pair (gamma, i), one contracted index), of s and of n_in terms -- and three products (Wl N, times Y, and the
rounding of the product T1 Y counted with them), and under ``accumulate`` one more addition.  A sum of m terms in any order
carries at most (m - 1) u per term to first order in u = 2^-53, a product u, so a float64 computation in any order of those
sums satisfies |G' - G'_exact| <= (S n_out + s + n_in + 3) u G'_abs to first order; the bound used is twice that for the
second-order terms.  tests/test_op_close_host.py holds float64 NumPy against np.longdouble inside it for every case below.
"""
from typing import NamedTuple

import numpy as np

from tests.hadamard_close_ref import FILL, TAIL, TRIES
from tests.hadamard_ref import BETA_CHUNK, COLS_PER_WORKGROUP, KBLOCK, LAYOUTS, TILE, _core

# the extents that reach each edge: tiles of 16 for P, S' and s'; s' past one workgroup's columns; the chunk edges of HD_KC
# for s; the k-blocks of four for S n_out
EDGES_TILE = (1, KBLOCK - 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
EDGES_S = (1, BETA_CHUNK - 1, BETA_CHUNK, BETA_CHUNK + 1, 2 * BETA_CHUNK + 1)
EDGES_K = (1, KBLOCK - 1, KBLOCK, KBLOCK + 1)
N_LAYOUTS = ("packed", "padded")


class Case(NamedTuple):
    name: str
    S: int
    S1: int
    s: int
    s1: int
    n_in: int
    n_out: int
    P: int
    n_layout: str = "packed"
    y_layout: str = "c"
    accumulate: int = 0


def _case(S, S1, s, s1, n_in, n_out, P, tag="", **kw):
    return Case(f"S{S}_{S1}_s{s}_{s1}_in{n_in}_out{n_out}_P{P}" + tag, S, S1, s, s1, n_in, n_out, P, **kw)


E, ES = EDGES_TILE, EDGES_S
CASES = [
    _case(1, E[0], ES[0], E[0], 1, 1, E[0]),                                                      # S n_out = 1
    _case(3, E[1], ES[1], E[1], 2, 1, E[1], accumulate=1),                                        # 3
    _case(2, E[2], ES[2], E[2], 5, 2, E[2]),                                                      # 4
    _case(5, E[3], ES[3], E[3], 2, 1, E[3], accumulate=1),                                        # 5
    _case(1, E[4], ES[4], E[4], 1, 3, E[4]),                                                      # n_in = 1
    _case(2, E[5], ES[0], E[5], 2, 2, E[5], accumulate=1),
    _case(3, 1, 3, COLS_PER_WORKGROUP + 1, 5, 1, 3, "_split"),                                    # s' past one workgroup's columns
    _case(3, 2, 4, 7, 5, 3, 5, "_flipped_views", n_layout="padded", y_layout="flipped", accumulate=1),
    _case(2, TILE + 2, 6, TILE + 1, 2, 3, 4, "_mixed_strides", y_layout="mode_major"),
    _case(3, 3, BETA_CHUNK + 1, 5, 4, 2, TILE + 1, "_mixed_strides", n_layout="padded", y_layout="padded", accumulate=1),
    _case(2, 3, 3, COLS_PER_WORKGROUP + 1, 239, 2, TILE + 1, "_ragged_chunks", y_layout="mode_major"),   # 120 chunks of two j, the last of one
    _case(5, 4 * TILE + 2, BETA_CHUNK + 2, 3, 2, 1, 1, "_one_row_flipped", y_layout="flipped", accumulate=1),
]
del E, ES


def dims(case: Case):
    """S, S', s, s', n_in, n_out, P as the entry takes them"""
    return tuple(case[1:8])


def layout(S, S1, s, s1, n_in, n_out, P):
    """the plan's split of the in-index, restated: (jchunks, j per chunk, doubles of the slab, workgroups)"""
    groups = -(-P // TILE) * -(-S1 // TILE) * -(-s1 // COLS_PER_WORKGROUP)
    want = -(-FILL // groups)
    for tries in range(TRIES + 1):
        want = min(want, n_in)
        jper = -(-n_in // want)
        jchunks = -(-n_in // jper)
        blocks = groups * jchunks
        if TAIL[1] * blocks >= TAIL[0] * -(-blocks // FILL) * FILL or want >= n_in:      # the last round nine tenths full
            break
        want += 1
    return jchunks, jper, jchunks * P * S1 * s1, blocks


def operator_core(rng, shape, layout_):
    """an operator core (S, n_in, n_out, S') whose (gamma, i) is one run: a view of a (S, n_out, n_in, S') base, contiguous
    ("packed") or cut out of a wider one ("padded": the runs of S' are apart, and those of n_in)"""
    S, n_in, n_out, S1 = shape
    if layout_ == "packed":
        return rng.standard_normal((S, n_out, n_in, S1)).transpose(0, 2, 1, 3)
    if layout_ == "padded":
        return rng.standard_normal((S, n_out, n_in + 2, S1 + 3))[:, :, 1:1 + n_in, 1:1 + S1].transpose(0, 2, 1, 3)
    raise ValueError(layout_)


def case_arrays(case: Case):
    """(Wl, N, Y, out0): out0 is what `out` holds before an accumulating call, None otherwise"""
    rng = np.random.default_rng(sum(map(ord, case.name)))
    Wl = rng.standard_normal((case.s * case.S, case.n_out, case.P)) / np.sqrt(case.s * case.S * case.n_out)
    N = operator_core(rng, (case.S, case.n_in, case.n_out, case.S1), case.n_layout)
    Y = _core(rng, (case.s, case.n_in, case.s1), case.y_layout)
    out0 = rng.standard_normal((case.P, case.s1 * case.S1)) if case.accumulate else None
    return Wl, N, Y, out0


def one_run(N) -> bool:
    """the stride condition of the entry, on a NumPy array"""
    S, _, n_out, _ = N.shape
    return S == 1 or n_out == 1 or N.strides[0] == n_out * N.strides[2]


def close_term(Wl, N, Y, out0=None, absolute=False, dtype=np.float64):
    """G' (or G'_abs), (P, s' S') of `dtype`; with out0 added"""
    Wl, N, Y = (np.asarray(a, dtype=dtype) for a in (Wl, N, Y))
    if absolute:
        Wl, N, Y = np.abs(Wl), np.abs(N), np.abs(Y)
    S, s = N.shape[0], Y.shape[0]
    T1 = np.einsum("cgip,gjih->cjph", Wl.reshape(s, S, Wl.shape[1], Wl.shape[2]), N)
    G = np.einsum("cjd,cjph->pdh", Y, T1)
    G = G.reshape(G.shape[0], -1)
    if out0 is not None:
        out0 = np.asarray(out0, dtype=dtype)
        G = G + (np.abs(out0) if absolute else out0)
    return G


def depth(Wl, N, Y) -> int:
    """summation depth: S n_out + s + n_in + 3"""
    return N.shape[0] * N.shape[2] + Y.shape[0] + Y.shape[1] + 3


def bound(Wl, N, Y, out0=None):
    """the entrywise tolerance 2 (S n_out + s + n_in + 3) 2^-53 G'_abs"""
    return 2.0 * depth(Wl, N, Y) * 2.0 ** -53 * close_term(Wl, N, Y, out0, absolute=True)


def dense_product(op_cores, tt_cores):
    """the dense tensor of an operator (cores (S, n_in, n_out, S')) applied to a train, through the explicit product cores"""
    acc = np.ones((1, 1))
    for M, C in zip(op_cores, tt_cores):
        Q = np.einsum("ijkl,ajb->iaklb", M, C)
        Q = Q.reshape(Q.shape[0] * Q.shape[1], Q.shape[2], -1)
        acc = np.tensordot(acc, Q, axes=(acc.ndim - 1, 0))
    return acc.reshape(acc.shape[1:-1])


def close_from_product(Wl, N, Y):
    """the same G' through the explicit product core Q[(g c), i, (h d)] ("ijkl,ajb->iaklb" of N and Y, operator rank major),
    contracted with Wl, whose rows are (c, g)"""
    Q = np.einsum("ijkl,ajb->iaklb", N, Y)
    S, s = N.shape[0], Y.shape[0]
    G = np.einsum("cgkp,gcklb->pbl", Wl.reshape(s, S, Wl.shape[1], Wl.shape[2]), Q)
    return G.reshape(Wl.shape[2], -1)
