"""Gram-SVD rounding of a tensor train restated in NumPy, and what the tests of
``ttsk_gram_round_bonds`` / ``TensorTrain.round_gram`` share: random trains, dense parts of a bond, the truths a bond solve is
held against and the cases with the deviations of this restatement from those truths.

Bond matrices in the form the kernel takes (step 6): ``P = V_L L_L^{-1/2} U_rho`` and ``Q = U_rho^T L_L^{1/2} V_L^T``."""
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

EPS_MACHINE = float(np.finfo(np.float64).eps)


def random_tt(shape, ranks, seed) -> List[np.ndarray]:
    rng = np.random.default_rng(seed)
    rk = (1,) + tuple(ranks) + (1,)
    return [rng.standard_normal((rk[k], n, rk[k + 1])) / np.sqrt(n * rk[k]) for k, n in enumerate(shape)]


def dense(cores) -> np.ndarray:
    acc = cores[0]
    for c in cores[1:]:
        acc = np.tensordot(acc, c, axes=(-1, 0))
    return acc.reshape(acc.shape[1:-1])


def add(A, B) -> List[np.ndarray]:
    """the direct sum of two trains"""
    out = [np.concatenate((A[0], B[0]), axis=2)]
    for a, b in zip(A[1:-1], B[1:-1]):
        blk = np.zeros((a.shape[0] + b.shape[0], a.shape[1], a.shape[2] + b.shape[2]))
        blk[:a.shape[0], :, :a.shape[2]] = a
        blk[a.shape[0]:, :, a.shape[2]:] = b
        out.append(blk)
    out.append(np.concatenate((A[-1], B[-1]), axis=0))
    return out


def scale(cores, alpha) -> List[np.ndarray]:
    return [c.copy() for c in cores[:-1]] + [cores[-1] * alpha]


def rel_error(a: np.ndarray, b: np.ndarray) -> float:
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


# ---------------------------------------------------------------- steps 1-7
def grams(cores) -> Tuple[List[np.ndarray], List[np.ndarray]]:
    """steps 1 and 2: (GL, GR), entry b - 1 the Grams of bond b"""
    GL = [np.ones((1, 1))]
    for c in cores[:-1]:
        GL.append(np.einsum("ab,aic,bie->ce", GL[-1], c, c, optimize=True))
    GR = [np.ones((1, 1))]
    for c in cores[:0:-1]:
        GR.append(np.einsum("ce,aic,bie->ab", GR[-1], c, c, optimize=True))
    return GL[1:], GR[1:][::-1]


def eig_kept(G: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """step 3: the eigenpairs with lambda > r eps_machine lambda_max, descending (at least one)"""
    w, V = np.linalg.eigh((G + G.T) / 2)
    w, V = w[::-1], V[:, ::-1]
    keep = max(1, int(np.sum(w > w[0] * G.shape[0] * EPS_MACHINE)))
    return np.maximum(w[:keep], 0.0), V[:, :keep]


def bond_solve(GL: np.ndarray, GR: np.ndarray, eps: float = 0.0, cap: Optional[int] = None):
    """steps 3-6 of one bond: (P (r, rho), Q (rho, r), Sigma, rho)"""
    wl, Vl = eig_kept(GL)
    wr, Vr = eig_kept(GR)
    M = (np.sqrt(wl)[:, None] * (Vl.T @ Vr)) * np.sqrt(wr)[None, :]
    U, S, _ = np.linalg.svd(M, full_matrices=False)
    r = GL.shape[0]
    rho = max(1, min(int(np.sum(S > S[0] * eps)), r if cap is None else cap))
    inv = np.divide(1.0, np.sqrt(wl), out=np.zeros_like(wl), where=wl > 0)
    P = (Vl * inv) @ U[:, :rho]
    Q = (U[:, :rho].T * np.sqrt(wl)) @ Vl.T
    return P, Q, S, rho


def round_gram(cores, eps: float = 0.0, caps: Optional[Sequence[int]] = None):
    """steps 1-7: (new cores, the Sigma of every bond)"""
    d = len(cores)
    GL, GR = grams(cores)
    sol = [bond_solve(GL[b], GR[b], eps, None if caps is None else caps[b]) for b in range(d - 1)]
    one = np.ones((1, 1))
    out = []
    for k, c in enumerate(cores):
        q = sol[k - 1][1] if k > 0 else one
        p = sol[k][0] if k < d - 1 else one
        out.append(np.einsum("ra,aib,bs->ris", q, c, p, optimize=True))
    return out, [s[2] for s in sol]


# ---------------------------------------------------------------- the truths of one bond
def parts(cores, b: int) -> Tuple[np.ndarray, np.ndarray]:
    """the dense left part A (rows x r_b) and right part B (columns x r_b) of bond b: the b-th unfolding is A B^T"""
    acc = cores[0].reshape(cores[0].shape[1], cores[0].shape[2])
    for c in cores[1:b]:
        acc = np.tensordot(acc, c, axes=(1, 0)).reshape(-1, c.shape[2])
    A = acc
    acc = cores[-1].reshape(cores[-1].shape[0], cores[-1].shape[1])
    for c in cores[-2:b - 1:-1]:
        acc = np.tensordot(c, acc, axes=(2, 0)).reshape(c.shape[0], -1)
    return A, acc.T


class BondDeviation(NamedTuple):
    orth: float        # max |P^T GL P - I|
    trunc: float       # ||A P Q B^T - (rank-rho truncation of A B^T)||_F / ||A B^T||_F
    sigma: float       # max |Sigma - svd(A B^T)| / sigma_1


def bond_deviation(A: np.ndarray, B: np.ndarray, P: np.ndarray, Q: np.ndarray, S: np.ndarray, rho: int) -> BondDeviation:
    X = A @ B.T
    U, sv, Vt = np.linalg.svd(X, full_matrices=False)
    k = min(len(S), len(sv))
    orth = float(np.max(np.abs(P.T @ (A.T @ A) @ P - np.eye(rho))))
    trunc = float(np.linalg.norm((A @ P) @ (Q @ B.T) - (U[:, :rho] * sv[:rho]) @ Vt[:rho]) / np.linalg.norm(X))
    return BondDeviation(orth, trunc, float(np.max(np.abs(S[:k] - sv[:k])) / sv[0]))


def expected_rank(A: np.ndarray, B: np.ndarray, eps: float, cap: int) -> int:
    sv = np.linalg.svd(A @ B.T, compute_uv=False)
    return max(1, min(int(np.sum(sv > sv[0] * eps)), cap))


class BondCase(NamedTuple):
    """The bonds of one ttsk_gram_round_bonds call: every bond of the train (shape, ranks), caps as given.  `dev`: the
    deviations of this restatement from the truths on these inputs, the largest over the bonds, measured on the CPU
    (tests/test_gram_round_host.py holds the restatement inside them); the GPU test allows the kernel 16 times as much,
    with a floor of 1e-13."""
    name: str
    shape: Tuple[int, ...]
    ranks: Tuple[int, ...]
    caps: Tuple[int, ...]
    eps: float
    seed: int
    dev: BondDeviation


BOND_CASES = [
    # bond ranks 1, 2, 16, 17 in one call, mixed, caps that bind at two of them
    BondCase("r1_2_16_17", (3, 4, 5, 6, 20), (1, 2, 16, 17), (1, 2, 9, 17), 0.0, 11, BondDeviation(1.05e-14, 2.7e-15, 2.0e-15)),
    # LDS edges: both matrices in LDS (100), one (101, 142), the workspace (143): the shape makes these Grams full rank
    BondCase("r100_101", (150, 4, 150), (100, 101), (60, 101), 0.0, 12, BondDeviation(2.9e-15, 4.2e-15, 2.8e-15)),
    BondCase("r142_143", (150, 4, 150), (142, 143), (142, 70), 0.0, 13, BondDeviation(3.9e-13, 4.4e-15, 2.2e-15)),
    # one bond of 300 in the workspace, count = 1
    BondCase("r300", (310, 320), (300,), (120,), 0.0, 14, BondDeviation(1.8e-15, 5.8e-15, 1.2e-15)),
    # count = 1 with eps deciding the rank
    BondCase("r17_eps", (20, 30), (17,), (17,), 0.3, 15, BondDeviation(2.9e-15, 2.1e-15, 1.1e-15)),
]


def case_cores(case: BondCase) -> List[np.ndarray]:
    return random_tt(case.shape, case.ranks, case.seed)


def floor16(x: float) -> float:
    """the GPU tolerance from a recorded deviation"""
    return max(16.0 * x, 1e-13)


# ---------------------------------------------------------------- the cases of round_gram against round
class RoundCase(NamedTuple):
    name: str
    shape: Tuple[int, ...]
    ranks: Tuple[int, ...]
    max_rank: object          # what round takes: None, an int or a per-bond tuple
    seed: int


ROUND_CASES = [
    RoundCase("d4_cap4", (9, 12, 7, 10), (5, 8, 6), 4, 21),
    RoundCase("d5_cap12", (30, 40, 30, 20, 30), (20, 35, 35, 18), 12, 22),
    RoundCase("infeasible", (3, 4, 3, 5), (9, 20, 11), 5, 23),
    RoundCase("d2", (11, 13), (7,), 3, 24),
    RoundCase("mode1", (6, 1, 7, 5), (4, 4, 3), 2, 25),
    RoundCase("per_bond", (12, 10, 12, 10), (17, 33, 16), (7, 9, 5), 26),
    RoundCase("cap_above", (8, 9, 7), (5, 4), 50, 27),
]
EXACT_CASE = RoundCase("no_truncation", (16, 16, 16), (8, 8), None, 28)
# error of Gram rounding against the input over that of `round`, the cases above that truncate: the largest ratio the
# restatement shows on the CPU is 1.00572 (d5_cap12; tests/test_gram_round_host.py prints them), plus 2 %
ERROR_RATIO_CAP = 1.00572 * 1.02
