"""NumPy restatement of the two CP sketch entries (csrc/cp_pass.hip), with factor matrix V (n, N), DRM core D (rho, n, rho')
and contractions L (N, rho or l), R (N, r), R_om (N, r_om):

    ttsk_cp_chain_step   out[j, m]    = sum_{a, k} L[j, a] V[k, j] D[a, k, m]
    ttsk_cp_psi_omega    psi[i, k, m] = sum_j L[j, i] V[k, j] R[j, m]        omega[i, m] = sum_j L[j, i] R_om[j, m]

in float64, or in any other dtype for a check of the bound; a missing L or R is all ones with rank 1, a missing R_om is R.

The same on |operands| gives the sum of the absolute values of all terms.  Every term of the chain step is two products
under a sum of rho n terms, of Psi two products under a sum of N terms (in chunks, which changes the order of the sum and
not its depth), of Omega one product under that sum; a float64 computation in any order of the sums satisfies, to first
order in u = 2^-53, |x - x_exact| <= (depth) u x_abs with depth rho n + 2, N + 3 and N + 2.  The bounds used are twice that
for the second-order terms.  tests/test_cp_pass_host.py holds float64 NumPy against np.longdouble inside them for every case.
"""
from typing import NamedTuple, Optional

import numpy as np

# the plan constants of csrc/cp_pass_plan.h; tests/test_cp_pass_host.py checks them against the header's
MAX_RANK = 128                 # CP_MAX_RANK
SMALL_N = 64                   # CP_SMALL_N: up to here one 16-row tile per wave, one workgroup
ROWS_PER_WORKGROUP = 128       # 16 CP_ROW_TILES CP_WAVES, from N = SMALL_N + 1 on
ROW_CHUNK = 32                 # CP_KC: rows (a, k) of D per LDS stage
D_PITCH = 144                  # CP_D_PITCH
CHAIN_LDS = 2 * ROW_CHUNK * D_PITCH * 8
PSI_COLS = 128                 # CP_PSI_COLS: columns (k, m) of one workgroup
N_CHUNK = 512                  # CP_N_CHUNK: terms of the sum over N per workgroup
U = 2.0 ** -53


class ChainCase(NamedTuple):
    name: str
    N: int
    rho: int
    n: int
    rho1: int
    no_L: bool = False         # NULL L: rho = 1
    v: str = "plain"           # "plain" (n, N) contiguous, "transposed" view of an (N, n) array, "slice" of columns of a wider one
    pad: int = 0               # columns past the width in the rows of L and out


class PsiCase(NamedTuple):
    name: str
    N: int
    l: int
    n: int
    r: int
    omega: Optional[int] = None    # None: no Omega; 0: Omega with R itself; > 0: with an R_om of its own of that many columns
    no_L: bool = False
    no_R: bool = False
    v: str = "plain"
    pad: int = 0


# The smallest shapes that reach each edge.  Rows: N in {1, 15, 16, 17, 33}, at the switch to two tiles per wave (63, 64, 65)
# and around the rows of a workgroup (127, 128, 129; 257 for a third workgroup).  Contracted length rho n in {1, .., 31, 32,
# 33, 65, 96, 561}: below 4, the chunk edges, three chunks, many.  n in {1, 3, 4, 5, 33}: the lane's (a, k) step wraps every
# k-block, never, with 4 / n in {4, 1, 1, 0, 0}.  rho' in {1, 15, 16, 17, 33, 128}.
CHAIN_CASES = [
    ChainCase("ones", 1, 1, 1, 1),
    ChainCase("N15_first_mode", 15, 1, 3, 15, no_L=True),
    ChainCase("N16_k31", 16, 31, 1, 16),
    ChainCase("N17_k32", 17, 8, 4, 17, pad=3),
    ChainCase("N33_k33", 33, 1, 33, 33),
    ChainCase("N63_k65", 63, 13, 5, 1),
    ChainCase("N64_k96_cols128", 64, 3, 32, 128),
    ChainCase("N65_two_tiles", 65, 16, 3, 15, pad=1),
    ChainCase("N127_vT", 127, 17, 3, 17, v="transposed"),
    ChainCase("N128_vslice", 128, 3, 5, 16, v="slice"),
    ChainCase("N129_k561", 129, 17, 33, 33, pad=5),
    ChainCase("N257_first_mode_vT", 257, 1, 4, 128, no_L=True, v="transposed"),
    ChainCase("N33_n1_rho17", 33, 17, 1, 3),
    ChainCase("N20_k64_two_full_chunks", 20, 16, 4, 33, v="slice", pad=2),
]

# l and r each in {1, 15, 16, 17, 33, 128}; n in {1, 3, 17}; N in {1, 3, 4, 5} (k-blocks), {511, 512, 513, 1025} (chunks: one,
# one full, two, three); columns n r (+ Omega's) in {127, 128, 129} and beyond one column block; the missing operands.
PSI_CASES = [
    PsiCase("ones", 1, 1, 1, 1),
    PsiCase("N3_l15_r17_om", 3, 15, 3, 17, omega=0),
    PsiCase("N4_l16_r16", 4, 16, 1, 16),
    PsiCase("N5_l17_r15_om_own", 5, 17, 3, 15, omega=33, pad=2),
    PsiCase("N511_l33_r1_om", 511, 33, 17, 1, omega=0),
    PsiCase("N512_l1_r33", 512, 1, 3, 33, omega=16),
    PsiCase("N513_l128_r3", 513, 128, 1, 3, omega=0, pad=1),
    PsiCase("N1025_l3_r128_om_own", 1025, 3, 1, 128, omega=1),
    PsiCase("cols127", 33, 5, 1, 127),
    PsiCase("cols128_om_spills", 33, 5, 8, 16, omega=0),
    PsiCase("cols129", 17, 16, 3, 43),
    PsiCase("cols126_om2_fills", 17, 3, 3, 42, omega=2),
    PsiCase("first_mode", 40, 1, 17, 33, no_L=True),
    PsiCase("last_mode_om_own", 40, 17, 3, 1, omega=15, no_R=True, v="transposed"),
    PsiCase("both_missing", 7, 1, 3, 1, omega=0, no_L=True, no_R=True),
    PsiCase("omega_alone", 600, 16, 0, 17, omega=0),
    PsiCase("vslice_N1025", 1025, 17, 3, 15, omega=17, v="slice", pad=4),
]


def _rng(name):
    return np.random.default_rng(sum(map(ord, name)))


def _factor(rng, n, N, layout):
    """V (n, N) in the layout asked for, and the array it is a view of"""
    if layout == "transposed":
        base = rng.standard_normal((N, n))
        return base.T, base
    if layout == "slice":
        base = rng.standard_normal((n, N + 5))
        return base[:, 2:2 + N], base
    base = rng.standard_normal((n, N))
    return base, base


def _padded(rng, rows, cols, pad):
    """(rows, cols) as the leading columns of a (rows, cols + pad) array whose other cells are NaN"""
    base = np.full((rows, cols + pad), np.nan)
    base[:, :cols] = rng.standard_normal((rows, cols))
    return base[:, :cols], base


def chain_arrays(case: ChainCase):
    """dict of L (None when missing), V, D and the arrays L_base, V_base they are views of"""
    rng = _rng(case.name)
    V, V_base = _factor(rng, case.n, case.N, case.v)
    L, L_base = (None, None) if case.no_L else _padded(rng, case.N, case.rho, case.pad)
    D = rng.standard_normal((case.rho, case.n, case.rho1)) / np.sqrt(case.rho * case.n)
    return dict(L=L, L_base=L_base, V=V, V_base=V_base, D=D)


def psi_arrays(case: PsiCase):
    """dict of L, R, R_om (None when missing), V (None for Omega alone) and their base arrays"""
    rng = _rng(case.name)
    V, V_base = _factor(rng, case.n, case.N, case.v) if case.n else (None, None)
    L, L_base = (None, None) if case.no_L else _padded(rng, case.N, case.l, case.pad)
    R, R_base = (None, None) if case.no_R else _padded(rng, case.N, case.r, case.pad)
    Ro, Ro_base = _padded(rng, case.N, case.omega, case.pad) if case.omega else (None, None)
    return dict(L=L, L_base=L_base, R=R, R_base=R_base, R_om=Ro, R_om_base=Ro_base, V=V, V_base=V_base)


def _as(x, rows, dtype, absolute):
    x = np.ones((rows, 1), dtype=dtype) if x is None else np.asarray(x, dtype=dtype)
    return np.abs(x) if absolute else x


def chain_step(L, V, D, absolute=False, dtype=np.float64):
    """out (N, rho'), or the same sum on |operands|"""
    N = V.shape[1]
    L, V, D = _as(L, N, dtype, absolute), _as(V, 0, dtype, absolute), _as(D, 0, dtype, absolute)
    A = L[:, :, None] * V.T[:, None, :]
    return np.einsum("jak,akm->jm", A, D)


def psi(L, R, V, absolute=False, dtype=np.float64):
    """Psi (l, n, r)"""
    N = V.shape[1]
    L, R, V = _as(L, N, dtype, absolute), _as(R, N, dtype, absolute), _as(V, 0, dtype, absolute)
    B = V.T[:, :, None] * R[:, None, :]
    return np.einsum("ji,jkm->ikm", L, B)


def omega(L, R_om, N, absolute=False, dtype=np.float64):
    """Omega (l, r_om)"""
    L, R_om = _as(L, N, dtype, absolute), _as(R_om, N, dtype, absolute)
    return np.einsum("ji,jm->im", L, R_om)


def chain_bound(L, V, D):
    """the entrywise tolerance 2 (rho n + 2) 2^-53 out_abs"""
    return 2.0 * (D.shape[0] * D.shape[1] + 2) * U * chain_step(L, V, D, absolute=True)


def psi_bound(L, R, V):
    """2 (N + 3) 2^-53 psi_abs"""
    return 2.0 * (V.shape[1] + 3) * U * psi(L, R, V, absolute=True)


def omega_bound(L, R_om, N):
    """2 (N + 2) 2^-53 omega_abs"""
    return 2.0 * (N + 2) * U * omega(L, R_om, N, absolute=True)


# today's compositions (tensor_train_drm.py sketch_cp, cp_sketch.py), the contract formulas as np.einsum
def chain_step_composed(L, V, D):
    if L is None:
        return np.einsum("ij,ik->jk", V, D[0])
    W = np.einsum("ij,jkl->ikl", L, D)
    return np.einsum("ki,ikl->il", V, W)


def psi_composed(L, R, V):
    if L is None and R is None:
        return V[None, :, :].sum(axis=2)[:, :, None]
    if L is None:
        return np.einsum("ji,il->jl", V, R)[None]
    if R is None:
        return np.einsum("li,kl->ik", L, V)[:, :, None]
    W = np.einsum("kj,jm->jkm", V, R)
    return np.einsum("ji,jkm->ikm", L, W)


def omega_composed(L, R_om):
    return np.einsum("ji,jk->ik", L, R_om)
