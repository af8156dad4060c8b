"""NumPy restatement of ``ttsk_hadamard_close`` (csrc/hadamard_close.hip): with the cores U (S, n, S') and V (s, n, s') of the
two factors of the second product and Wl ((gamma c), i, p), what ``ttsk_hadamard_apply`` made of the chain,

    T1[gamma, i, p, c'] = sum_c Wl[(gamma s + c), i, p] V[c, i, c']
    G'[p, gamma', c']   = sum_i sum_gamma U[gamma, i, gamma'] T1[gamma, i, p, c']      -> (P, S' s'), columns in (gamma', c') order

in float64, or in any other dtype for a check of the bound.

The same on |operands| gives G'_abs, the sum of the absolute values of all terms of G' (with ``accumulate``, of what ``out``
held as well).  Every term passes through three nested sums, of s, of S and of n terms, and three products, and under
``accumulate`` one more addition, so a float64 computation in any order of those sums satisfies, to first order in
u = 2^-53, |G' - G'_exact| <= (s + S + n + 3) u G'_abs; the bound used is twice that for the second-order terms.
tests/test_hadamard_close_host.py holds float64 NumPy against np.longdouble inside it for every case below.
"""
from typing import NamedTuple

import numpy as np

from tests.hadamard_ref import BETA_CHUNK, COLS_PER_WORKGROUP, KBLOCK, LAYOUTS, TILE, _core

# of csrc/hadamard_close_plan.h (tests/test_hadamard_close_host.py holds them against the header)
FILL = 512                     # HC_FILL: workgroups the plan cuts the mode for
TAIL = (9, 10)                 # HC_TAIL_NUM / HC_TAIL_DEN: how full the last round of FILL has to be
TRIES = 16                     # HC_TRIES: further cuts tried for that

# the extents that reach each edge: tiles of 16 and k-blocks of 4 for s, s', P; the chunk edges for S; the gamma' tiles, half
# a workgroup's columns and the grid split past them for S'
EDGES_SMALL = (1, KBLOCK - 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
EDGES_S = (1, BETA_CHUNK - 1, BETA_CHUNK, BETA_CHUNK + 1, 2 * BETA_CHUNK + 1)
EDGES_S1 = (1, TILE - 1, TILE, TILE + 1, COLS_PER_WORKGROUP // 2, COLS_PER_WORKGROUP // 2 + 1, COLS_PER_WORKGROUP + 1)
EDGES_N = (1, 2, 5)


class Case(NamedTuple):
    name: str
    S: int
    S1: int
    s: int
    s1: int
    n: int
    P: int
    u_layout: str = "c"
    v_layout: str = "c"
    accumulate: int = 0


def _case(S, S1, s, s1, n, P, tag="", **kw):
    return Case(f"S{S}_cols{S1}_s{s}_{s1}_n{n}_P{P}" + tag, S, S1, s, s1, n, P, **kw)


E, ES, E1 = EDGES_SMALL, EDGES_S, EDGES_S1
CASES = [
    _case(ES[0], E1[0], E[0], E[0], 1, E[0]),
    _case(ES[1], E1[1], E[1], E[1], 2, E[1], accumulate=1),
    _case(ES[2], E1[2], E[2], E[3], 5, E[3]),
    _case(ES[3], E1[3], E[3], E[4], 2, E[4], accumulate=1),
    _case(ES[4], E1[4], E[4], E[2], 1, E[2]),
    _case(ES[0], E1[5], E[5], E[5], 2, E[5], accumulate=1),
    _case(3, E1[6], E[1], E[0], 5, E[1], "_split"),
    _case(3, 2, 4, 7, 5, 5, "_flipped_views", u_layout="flipped", v_layout="flipped", accumulate=1),
    _case(5, TILE + 2, 6, TILE + 1, 2, 4, "_mixed_strides", u_layout="mode_major", v_layout="padded"),
    _case(BETA_CHUNK + 1, 3, 2, 5, 5, TILE + 1, "_mixed_strides", u_layout="padded", v_layout="flipped", accumulate=1),
    _case(2, COLS_PER_WORKGROUP + 1, 3, 3, 239, TILE + 1, "_ragged_chunks", v_layout="mode_major"),     # 120 chunks of two i, the last of one
    _case(BETA_CHUNK + 2, COLS_PER_WORKGROUP + 2, 5, 3, 2, 1, "_one_row_flipped_split", u_layout="flipped", accumulate=1),
]
del E, ES, E1


def layout(S, S1, s, s1, n, P):
    """the plan's split of the mode, restated: (ichunks, i per chunk, doubles of the slab, workgroups)"""
    groups = -(-P // TILE) * -(-s1 // TILE) * -(-S1 // COLS_PER_WORKGROUP)
    want = -(-FILL // groups)
    for tries in range(TRIES + 1):
        want = min(want, n)
        iper = -(-n // want)
        ichunks = -(-n // iper)
        blocks = groups * ichunks
        if TAIL[1] * blocks >= TAIL[0] * -(-blocks // FILL) * FILL or want >= n:       # the last round nine tenths full
            break
        want += 1
    return ichunks, iper, ichunks * P * S1 * s1, blocks


def case_arrays(case: Case):
    """(Wl, U, V, out0): out0 is what `out` holds before an accumulating call, None otherwise"""
    rng = np.random.default_rng(sum(map(ord, case.name)))
    Wl = rng.standard_normal((case.S * case.s, case.n, case.P)) / np.sqrt(case.S * case.s)
    U = _core(rng, (case.S, case.n, case.S1), case.u_layout)
    V = _core(rng, (case.s, case.n, case.s1), case.v_layout)
    out0 = rng.standard_normal((case.P, case.S1 * case.s1)) if case.accumulate else None
    return Wl, U, V, out0


def close_term(Wl, U, V, out0=None, absolute=False, dtype=np.float64):
    """G' (or G'_abs), (P, S' s') of `dtype`; with out0 added"""
    Wl, U, V = (np.asarray(a, dtype=dtype) for a in (Wl, U, V))
    if absolute:
        Wl, U, V = np.abs(Wl), np.abs(U), np.abs(V)
    S, s = U.shape[0], V.shape[0]
    T1 = np.einsum("gcip,cid->gipd", Wl.reshape(S, s, Wl.shape[1], Wl.shape[2]), V)
    G = np.einsum("gih,gipd->phd", U, T1)
    G = G.reshape(G.shape[0], -1)
    if out0 is not None:
        out0 = np.asarray(out0, dtype=dtype)
        G = G + (np.abs(out0) if absolute else out0)
    return G


def depth(Wl, U, V) -> int:
    """summation depth: s + S + n + 3"""
    return V.shape[0] + U.shape[0] + U.shape[1] + 3


def bound(Wl, U, V, out0=None):
    """the entrywise tolerance 2 (s + S + n + 3) 2^-53 G'_abs"""
    return 2.0 * depth(Wl, U, V) * 2.0 ** -53 * close_term(Wl, U, V, out0, absolute=True)


def close_from_product(Wl, U, V):
    """the same G' through the explicit Kronecker core Q[(g c), i, (h d)] ("gih,cid->gcihd")"""
    Q = np.einsum("gih,cid->gcihd", U, V)
    S, s = U.shape[0], V.shape[0]
    return np.einsum("gcip,gcihd->phd", Wl.reshape(S, s, Wl.shape[1], Wl.shape[2]), Q).reshape(Wl.shape[2], -1)
