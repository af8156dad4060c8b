"""NumPy restatement of the inner product of two CP tensors,
    <a, b> = sum_{j < N, j' < M} prod_k (A_k^T B_k)[j, j'],       A_k (n_k x N), B_k (n_k x M),
in float64, or in any other dtype for a check of the bound, and of <tt, cp> by the left-to-right chain
``L <- einsum("ja,ij,aib->jb", L, V_k, C_k)`` from L = 1, closed by the sum over j.

The same formulas on |factors| give G_abs, the sum of the absolute values of all terms.  In ``ttsk_cp_gram`` every term
passes through a summation of depth
    L = sum_k n_k + (d - 1) + 24 + run + ceil(G / 256) + 8
(per mode a sum over n_k, then the d - 1 products of the modes, each one rounding; inside a tile the 16 registers of a lane
one by one, the 6 butterfly steps of a wave and the four waves as two additions; the totals of the `run` tiles a workgroup
owns one by one; the closing sum over the G partials: ceil(G / 256) per thread, then a wave and the four waves), so a
computation in float64 with any order of those sums satisfies, to first order in u = 2^-53,
    |G - G_exact| <= L u G_abs,
and the bound used is twice that for the second-order terms.  The numbers G and run are those of cp_gram_plan.h
(tests/test_cp_gram_host.py holds this restatement against the header compiled by the host compiler).  For <tt, cp> the
depth is L = sum_k r_k n_k + N: mode k sums over r_k n_k, the close over N.  tests/test_cp_gram_host.py holds float64 NumPy
against np.longdouble inside these bounds for every case of the GPU test.
"""
import math
from typing import NamedTuple, Optional, Tuple

import numpy as np

# cp_gram_plan.h
TILE = 64               # CPG_TILE
KC = 16                 # CPG_KC: rows of a mode in LDS at once -- a mode above 16 takes a second step
WG_PER_CU = 3           # CPG_WG_PER_CU
TILE_SUMS = 24          # CPG_TILE_SUMS
CLOSE_SUMS = 8          # CPG_CLOSE_SUMS
MAX_MODES = 32          # CPG_MAX_MODES
CHIP_CUS = 256          # the chip the over-cap cases are sized for; the GPU test checks that they are over the cap there

CHAIN_MAX_RANK = 128    # the widest train rank ttsk_cp_chain_step covers (cp_pass_plan.h: CP_MAX_RANK)


class Case(NamedTuple):
    name: str
    shape: Tuple[int, ...]
    N: int
    M: Optional[int]        # None: the symmetric form, b = a
    pad_a: int = 0          # the factors are column slices of matrices pad columns wider: lda = N + pad_a
    pad_b: int = 0


def _over_cap(sym: bool) -> Tuple[int, int]:
    """(N, M) whose tiles outnumber the grid cap of a chip of CHIP_CUS units, so that some workgroup owns two tiles"""
    cap = WG_PER_CU * CHIP_CUS
    if sym:
        t = 1
        while t * (t + 1) // 2 <= cap:
            t += 1
        return TILE * (t - 1) + 5, TILE * (t - 1) + 5
    t = math.isqrt(cap) + 2
    return TILE * (t - 1) + 1, TILE * (t - 1)          # t x (t - 1) tiles


# the smallest shapes that reach each edge: N, M in {1, 15, 16, 17, 63, 64, 65, 129}, unequal; modes 1, 3, 4, 5, 12 mixed,
# and 16, 17, 33 for the second step of a mode; d = 1, 2, 5, 8; column slices; sym at N = 1, 16, 65, 129 (diagonal tiles
# only, diagonal and off-diagonal); more tiles than the grid cap, both forms
CASES = [
    Case("d1_N1_M15", (5,), 1, 15),
    Case("d1_N16_M17", (12,), 16, 17),
    Case("d1_N1_M1_n1", (1,), 1, 1),
    Case("d2_N15_M1", (3, 4), 15, 1),
    Case("d2_N63_M64", (1, 12), 63, 64),
    Case("d2_N64_M65", (4, 3), 64, 65),
    Case("d2_N65_M17_steps", (17, 33), 65, 17),
    Case("d3_N17_M65_steps", (16, 32, 1), 17, 65),
    Case("d5_N17_M63", (1, 3, 4, 5, 12), 17, 63),
    Case("d5_N65_M129", (12, 5, 4, 3, 1), 65, 129),
    Case("d8_N129_M16", (1, 3, 4, 5, 12, 3, 4, 5), 129, 16),
    Case("d8_N64_M63", (3,) * 8, 64, 63),
    Case("d2_slices", (4, 5), 17, 63, 3, 7),
    Case("d5_slices", (5, 1, 12, 3, 4), 129, 65, 1, 64),
    Case("sym_N1", (4,), 1, None),
    Case("sym_N16", (3, 12), 16, None),
    Case("sym_N65", (1, 3, 4, 5, 12), 65, None),
    Case("sym_N65_slice", (5, 4), 65, None, 5),
    Case("sym_N129", (3, 1, 4, 1, 5, 3, 12, 4), 129, None),
    Case("over_cap", (2, 2), *_over_cap(False)),
    Case("sym_over_cap", (2, 2), _over_cap(True)[0], None),
]


def case_factors(case: Case):
    """(wide_a, wide_b): per mode the (n_k, N + pad) matrices the factors are the first N (M) columns of; entries of both
    signs.  sym: wide_b is wide_a."""
    rng = np.random.default_rng(sum(map(ord, case.name)))
    wa = [rng.standard_normal((n, case.N + case.pad_a)) for n in case.shape]
    wb = wa if case.M is None else [rng.standard_normal((n, case.M + case.pad_b)) for n in case.shape]
    return wa, wb


def operands(case: Case, wa, wb):
    M = case.N if case.M is None else case.M
    return [w[:, :case.N] for w in wa], [w[:, :M] for w in wb]


def gram(A, B, absolute=False, dtype=np.float64):
    """<a, b> (or the sum of the |terms|) in `dtype`"""
    P = None
    for a, b in zip(A, B):
        a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
        if absolute:
            a, b = np.abs(a), np.abs(b)
        g = a.T @ b
        P = g if P is None else P * g
    return P.sum()


# ---- the plan's numbers
def tiles(N, M, sym):
    tn, tm = -(-N // TILE), -(-M // TILE)
    return tn * (tn + 1) // 2 if sym else tn * tm


def grid(N, M, sym, n_cu):
    return min(tiles(N, M, sym), WG_PER_CU * max(n_cu, 1))


def run(N, M, sym, n_cu):
    return -(-tiles(N, M, sym) // grid(N, M, sym, n_cu))


def tile_of(tn, tm, sym, t):
    """(tile row, tile column, weight) of tile t as cp_gram_tile orders them"""
    if not sym:
        return t // tm, t % tm, 1
    ti = 0
    while t >= tn - ti:
        t -= tn - ti
        ti += 1
    return ti, ti + t, (2 if t else 1)


def depth(shape, N, M, sym, n_cu):
    G = grid(N, M, sym, n_cu)
    return sum(shape) + len(shape) - 1 + TILE_SUMS + run(N, M, sym, n_cu) + -(-G // 256) + CLOSE_SUMS


def bound(A, B, sym, n_cu):
    """the tolerance 2 L 2^-53 G_abs"""
    shape = [a.shape[0] for a in A]
    return 2.0 * depth(shape, A[0].shape[1], B[0].shape[1], sym, n_cu) * 2.0 ** -53 * float(gram(A, B, absolute=True))


# ---- <tt, cp>
def tt_cp_dot(cores, V, absolute=False, dtype=np.float64):
    L = np.ones((V[0].shape[1], 1), dtype=dtype)
    for C, v in zip(cores, V):
        C, v = np.asarray(C, dtype=dtype), np.asarray(v, dtype=dtype)
        if absolute:
            C, v = np.abs(C), np.abs(v)
        L = np.einsum("ja,ij,aib->jb", L, v, C)
    return L.sum()


def tt_cp_bound(cores, V):
    """2 L 2^-53 of the sum of the |terms|, L = sum_k r_k n_k + N"""
    L = sum(C.shape[0] * C.shape[1] for C in cores) + V[0].shape[1]
    return 2.0 * L * 2.0 ** -53 * float(tt_cp_dot(cores, V, absolute=True))


def random_tt(rng, shape, ranks):
    rk = (1,) + tuple(ranks) + (1,)
    return [rng.standard_normal((rk[k], n, rk[k + 1])) / np.sqrt(rk[k]) for k, n in enumerate(shape)]


def fast_error(norm_a, norm_b, dot_ab, relative):
    """the reference's fast formula (tensor.py:68-72) on three numbers"""
    tot = norm_a ** 2 + norm_b ** 2
    err = np.sqrt(tot) * np.sqrt(abs(1 - 2 * dot_ab / tot))
    return err / norm_b if relative else err


def load_cases(path=None):
    """The fixtures of tests/golden/make_golden_cp_gram.py (runs of the reference) as a list of dicts."""
    import json
    import os
    if path is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cp_gram_cases.npz")
    z = np.load(path)
    cases = []
    for name, m in json.loads(str(z["meta"])).items():
        shape, d = tuple(m["shape"]), len(m["shape"])
        rk = (1,) + tuple(m["rank"]) + (1,)
        flat, cores, pos = z[f"{name}/cores"], [], 0
        for k in range(d):
            size = rk[k] * shape[k] * rk[k + 1]
            cores.append(flat[pos:pos + size].reshape(rk[k], shape[k], rk[k + 1]))
            pos += size
        factors = {}
        for side in "ab":
            flat, fs, pos, N = z[f"{name}/factors_{side}"], [], 0, m[f"cp_rank_{side}"]
            for n in shape:
                fs.append(flat[pos:pos + n * N].reshape(n, N))
                pos += n * N
            factors[side] = fs
        keys = ("norm_a", "norm_b", "dot_ab", "dot_a_tt", "dot_tt_a", "norm_tt", "error_tt_a", "error_a_tt")
        cases.append(dict(name=name, shape=shape, cores=cores, factors_a=factors["a"], factors_b=factors["b"],
                          **{k: float(v) for k, v in zip(keys, z[f"{name}/scalars"])}))
    return cases
