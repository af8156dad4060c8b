"""The long-double references of tests/solve_ref.py against fp64 LAPACK (CPU only): what tests/test_gpu_solve_edges.py
measures the device with has to be right itself, to well below the fp64 error it is there to resolve."""
import numpy as np
import pytest
import scipy.linalg

from tests import solve_ref as sr

LD, EPS = sr.LD, sr.EPS


def test_long_double_is_wider_than_double():
    assert np.finfo(LD).eps < 1e-18      # 80-bit extended: without it these references resolve nothing


@pytest.mark.parametrize("m,n,kappa", [(1, 1, 1), (2, 2, 3), (5, 1, 1), (33, 33, 30), (40, 7, 10), (193, 97, 10), (138, 138, 30)])
def test_hh_qr_is_lapacks_q(m, n, kappa):
    """column by column, signs included (m == n: the last reflector is the identity; n = 1: one reflector or none)"""
    A = sr.prescribed(m, n, kappa, np.random.default_rng(m * 1000 + n))
    Q = sr.hh_qr(A)
    Qs, _ = scipy.linalg.qr(A, mode="economic")
    assert sr.col_err(Qs, Q) <= 64 * EPS
    assert sr.orth_err(Q) <= 1e-17 * n
    # Q spans A: the residual of A against its projection, in long double
    AL = A.astype(LD)
    assert np.max(np.abs(Q @ (Q.T @ AL) - AL)) <= 1e-17 * n * np.max(np.abs(A))


def test_hh_qr_is_invariant_under_column_scaling():
    """the inputs that make CholeskyQR2 give up are a column-scaled matrix: Householder's Q does not see the scaling"""
    rng = np.random.default_rng(5)
    A = sr.prescribed(130, 5, 10, rng)
    As = A * np.logspace(0, -8, 5)
    Qs, _ = scipy.linalg.qr(As, mode="economic")
    assert sr.col_err(Qs, sr.hh_qr(As)) <= 64 * EPS
    assert sr.col_err(sr.hh_qr(As), sr.hh_qr(A)) <= 1e-8       # As is rounded to fp64 after the scaling: not the same matrix


def test_hh_qr_zero_tail_is_the_identity_reflector():
    A = np.array([[-2.0, 1.0], [0.0, 3.0], [0.0, 4.0]])
    Q = sr.hh_qr(A)
    Qs, _ = scipy.linalg.qr(A, mode="economic")
    assert Q[0, 0] == 1.0 and sr.col_err(Qs, Q) <= 8 * EPS


@pytest.mark.parametrize("l,r,kappa", [(1, 1, 1), (1, 4, 1), (4, 1, 1), (20, 20, 30), (40, 90, 10), (90, 40, 10), (64, 200, 3000), (300, 20, 3000), (200, 64, 3000)])
def test_pinv_full_is_the_moore_penrose_inverse(l, r, kappa):
    rng = np.random.default_rng(l * 1000 + r)
    A = sr.prescribed(max(l, r), min(l, r), kappa, rng)
    A = A if l >= r else np.ascontiguousarray(A.T)
    X = sr.pinv_full(A, agree=sr.NS_AGREE if kappa <= 100 else sr.NS_AGREE_ILL)
    AL = A.astype(LD)
    a, x = np.max(np.abs(AL)), np.max(np.abs(X))
    tol = 1e-17 * max(l, r)
    # the four Penrose conditions, in long double
    assert np.max(np.abs(AL @ X @ AL - AL)) <= tol * kappa * a
    assert np.max(np.abs(X @ AL @ X - X)) <= tol * kappa * x
    assert np.max(np.abs(AL @ X - (AL @ X).T)) <= tol * kappa
    assert np.max(np.abs(X @ AL - (X @ AL).T)) <= tol * kappa
    assert sr.col_err(np.linalg.pinv(A), X) <= 64 * EPS * kappa


def test_newton_schulz_stopping_rule():
    rng = np.random.default_rng(11)
    A = sr.prescribed(60, 25, 10, rng)
    X0 = np.linalg.pinv(A)
    _, steps = sr.newton_schulz(A, X0)
    assert steps <= 3                                 # an fp64 start is 1e-15 away: 1e-30 after one step, the second confirms it
    X = sr.pinv_full(A)
    # 1e-3 away: 1e-6, 1e-12, 1e-24 -- the fourth step is the first that changes nothing
    X4, steps = sr.newton_schulz(A, X * LD(1 + 1e-3))
    assert steps == 4 and sr.col_err(X4, X) <= sr.NS_AGREE
    with pytest.raises(RuntimeError):                 # 0.5 away: 0.25, 0.06, 4e-3, 1.5e-5 -- not a start
        sr.newton_schulz(A, X * LD(0.5))
    with pytest.raises(RuntimeError):
        sr.newton_schulz(A, X0, max_steps=1, agree=0.0)


def test_pinv_full_removes_what_the_iteration_cannot():
    """The iteration keeps the part of its start that A annihilates (rows outside the column space of a tall A): refined
    without the projection, LAPACK's pinv converges -- to something that is still LAPACK's 1e-15 away from pinv(A)."""
    rng = np.random.default_rng(11)
    A = sr.prescribed(60, 25, 10, rng)
    AL = A.astype(LD)
    X = sr.pinv_full(A)
    Xn, _ = sr.newton_schulz(A, np.linalg.pinv(A))
    P = AL @ X                                         # projector onto the column space of A
    assert np.max(np.abs(X - X @ P)) <= 1e-18 * np.max(np.abs(X))
    assert np.max(np.abs(Xn - Xn @ P)) >= 1e-16 * np.max(np.abs(X))


@pytest.mark.parametrize("l,r,k", [(40, 90, 7), (90, 40, 7), (8, 12, 3), (30, 50, 3)])
def test_pinv_rank_k_on_integer_factors(l, r, k):
    rng = np.random.default_rng(l + r + k)
    B, C = sr.int_factors(l, r, k, rng)
    A = B @ C                                          # exact in fp64
    assert np.linalg.matrix_rank(A) == k
    X = sr.pinv_rank_k(B, C)
    AL = A.astype(LD)
    assert np.max(np.abs(AL @ X @ AL - AL)) <= 1e-16 * np.max(np.abs(A))
    assert np.max(np.abs(X @ AL @ X - X)) <= 1e-16 * np.max(np.abs(X))
    assert np.max(np.abs(AL @ X - (AL @ X).T)) <= 1e-16
    assert np.max(np.abs(X @ AL - (X @ AL).T)) <= 1e-16
    assert sr.col_err(np.linalg.pinv(A, rcond=1e-10), X) <= 1e-13


def test_prescribed_has_the_stated_condition_number():
    rng = np.random.default_rng(2)
    for m, n, kappa in [(17, 17, 30), (300, 128, 10), (200, 64, 3000), (7, 1, 1)]:
        A = sr.prescribed(m, n, kappa, rng)
        assert sr.cond_is(A, kappa)
    assert not sr.cond_is(sr.prescribed(50, 20, 10, rng), 11)


def test_col_err_sees_one_wrong_element():
    ref = np.ones((300, 40))
    got = ref.copy()
    got[299, 39] += 1e-9                               # 1e-9 in one of 12000 entries: 1e-11 in a Frobenius ratio
    assert abs(sr.col_err(got, ref) - 1e-9) < 1e-15
    assert sr.col_err(ref, ref) == 0.0
    got[0, 0] = np.nan
    assert sr.col_err(got, ref) == float("inf")


def test_svd_residuals_of_numpys_svd():
    rng = np.random.default_rng(4)
    for m, n in [(1, 1), (7, 1), (40, 40), (90, 30)]:
        A = sr.prescribed(m, n, 100, rng)
        U, S, Vt = np.linalg.svd(A, full_matrices=False)
        res = sr.svd_residuals(A, U * S, S, Vt)
        assert max(res) <= 64 * EPS * np.sqrt(m), (m, n, res)
    # a wrong factor shows in the residual it belongs to
    US = U * S
    US[:, 3] *= 1 + 1e-9
    bad = sr.svd_residuals(A, US, S, Vt)
    assert bad[3] > 1e-11 and bad[2] > 1e-10
    # a zero singular value: its column is left out of U^T U
    res = sr.svd_residuals(A[:, :2] @ np.ones((2, 3)), np.c_[A[:, :2] @ np.ones((2, 1)) * np.sqrt(3), np.zeros((m, 2))],
                           np.array([np.linalg.norm(A[:, :2].sum(axis=1)) * np.sqrt(3), 0, 0]),
                           np.array([[1, 1, 1], [1, -1, 0], [1, 1, -2]]) / np.sqrt([[3], [2], [6]]))
    assert max(res) <= 64 * EPS
