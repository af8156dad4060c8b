"""Plain ``np.longdouble`` references for the small dense solves (csrc/cholesky.hip, householder.hip, jacobi.hip, pinv.hip).

No LAPACK result appears in an answer: fp64 LAPACK only supplies the start of an iteration that is then carried to
convergence in long double (64-bit mantissa, eps = 1.1e-19), so every reference stands about three digits beyond the
fp64 results it is compared with.

  hh_qr          Householder thin QR with LAPACK's conventions (dlarfg signs, tau = 0 for a zero tail)
  pinv_full      Moore-Penrose inverse of a full-rank matrix: LAPACK start, projected, Newton-Schulz to convergence
  pinv_rank_k    the same for A = B C with small-integer factors (A exact in fp64, rank exactly k)
  prescribed     a matrix with stated singular values 1 .. 1 / kappa
  col_err        element-wise error, the worst column: max_j max_i |got - ref|_ij / max_i |ref|_ij
  svd_residuals  the four residuals a thin SVD is judged by (no vector comparison: equal singular values are fine)
"""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
NS_AGREE = 2.0 ** -55        # two successive Newton-Schulz iterates agree to this (relative, max-abs) ...
NS_MAX_STEPS = 4             # ... within this many steps, or the start was not what it was taken for
# An iterate of a matrix with condition number kappa carries rounding noise of about 0.2 kappa 2^-63 (measured: 6e-19 at
# kappa = 10, 3e-17 at 3000), so at kappa = 3000 two iterates never agree to 2^-55 = 2.8e-17 reliably.  Callers with kappa
# beyond 100 ask for this instead: one fp64 eps, still 128 times below the tightest bar (128 eps) a reference is used for.
NS_AGREE_ILL = 2.0 ** -52


def hh_qr(A):
    """Q (m, n) of the thin Householder QR of A (m >= n), in long double.  beta = -copysign(norm, x0); a reflector whose
    vector has length 1 or a zero tail is the identity (dlarfg returns tau = 0) -- for a square matrix that is the last
    one, the `square` rule of the sign reconstruction on the device."""
    A = np.array(A, dtype=LD)
    m, n = A.shape
    assert m >= n >= 1
    refl = []
    for j in range(n):
        x = A[j:, j].copy()
        if x.size == 1 or not np.any(x[1:]):
            refl.append(None)
            continue
        beta = -np.copysign(np.sqrt(x @ x), x[0])
        v = x
        v[0] -= beta
        vv = v @ v
        refl.append((v, vv))
        A[j:, j:] -= np.outer(v, (2 / vv) * (v @ A[j:, j:]))
    Q = np.eye(m, n, dtype=LD)
    for j in range(n - 1, -1, -1):
        if refl[j] is not None:
            v, vv = refl[j]
            Q[j:, j:] -= np.outer(v, (2 / vv) * (v @ Q[j:, j:]))
    return Q


def newton_schulz(A, X0, max_steps=NS_MAX_STEPS, agree=NS_AGREE):
    """(X, steps): X <- X (2 I - A X) (A with no more rows than columns) or (2 I - X A) X, in long double, until two
    successive iterates agree to ``agree``; RuntimeError if they do not within ``max_steps``.  Every iterate keeps the
    column space (row space) of X0, so X0 has to lie in the range of A^T (pinv_full sees to that)."""
    A, X = np.asarray(A, dtype=LD), np.asarray(X0, dtype=LD)
    l, r = A.shape
    two = 2 * np.eye(min(l, r), dtype=LD)
    for step in range(1, max_steps + 1):
        Xn = X @ (two - A @ X) if l <= r else (two - X @ A) @ X
        done = np.max(np.abs(Xn - X)) <= agree * np.max(np.abs(Xn))
        X = Xn
        if done:
            return X, step
    raise RuntimeError(f"Newton-Schulz: {l} x {r}, iterates still apart after {max_steps} steps")


def pinv_full(A, agree=NS_AGREE):
    """pinv(A) (r, l) of a FULL-RANK A (l, r) in long double.  np.linalg.pinv is only the start: X0 is first put into the
    range of A^T exactly (A^+ = A^T A^+T A^+, resp. A^+ A^+T A^T, holds for the true inverse, and the right-hand side
    lies in that range for any X0 -- the iteration cannot remove a null-space component), then refined."""
    A = np.asarray(A, dtype=np.float64)
    l, r = A.shape
    X0 = np.linalg.pinv(A).astype(LD)
    AL = A.astype(LD)
    X0 = AL.T @ (X0.T @ X0) if l <= r else (X0 @ X0.T) @ AL.T
    return newton_schulz(AL, X0, agree=agree)[0]


def inv_ld(M):
    """Inverse of a small well-conditioned square matrix in long double (np.linalg.inv, refined)."""
    M = np.asarray(M, dtype=LD)
    return newton_schulz(M, np.linalg.inv(M.astype(np.float64)))[0]


def pinv_rank_k(B, C):
    """pinv(B C) for B (l, k), C (k, r) of full rank k: C^T (C C^T)^-1 (B^T B)^-1 B^T in long double.  With integer
    entries the two Gram matrices are exact."""
    B, C = np.asarray(B, dtype=LD), np.asarray(C, dtype=LD)
    return C.T @ inv_ld(C @ C.T) @ inv_ld(B.T @ B) @ B.T


def int_factors(l, r, k, rng):
    """B (l, k), C (k, r) with entries in -3..3 and full rank k (redrawn until both Gram matrices are comfortably regular
    and B C has no zero row or column: pinv(B C) has no zero column or row then, and col_err a scale for every column)."""
    while True:
        B = rng.integers(-3, 4, (l, k)).astype(np.float64)
        C = rng.integers(-3, 4, (k, r)).astype(np.float64)
        if np.linalg.cond(B) < 50 and np.linalg.cond(C) < 50 and np.all(np.any(B != 0, axis=1)) and np.all(np.any(C != 0, axis=0)):
            return B, C


def prescribed(m, n, kappa, rng):
    """(m, n) fp64, m >= n, with singular values logspace(0, -log10 kappa, n): U diag(s) V^T from two fp64 QR factors."""
    assert m >= n >= 1
    U, _ = np.linalg.qr(rng.standard_normal((m, n)))
    V, _ = np.linalg.qr(rng.standard_normal((n, n)))
    return (U * np.logspace(0, -np.log10(kappa), n)) @ V.T


def cond_is(A, kappa):
    """whether np.linalg.cond of the drawn matrix is within 1 % of the kappa its case states"""
    return abs(np.linalg.cond(A) / kappa - 1) <= 0.01


def col_err(got, ref):
    """max over columns of max |got - ref| / max |ref|, in long double: a wrong element is not averaged away in a norm."""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    assert got.shape == ref.shape and ref.ndim == 2
    scale = np.max(np.abs(ref), axis=0)
    if not np.all(scale > 0):
        raise ValueError("col_err: a reference column is zero")
    d = np.abs(got - ref)
    if not np.all(np.isfinite(d.astype(np.float64))):
        return float("inf")
    return float(np.max(np.max(d, axis=0) / scale))


def orth_err(Q):
    """max |Q^T Q - I| in long double"""
    Q = np.asarray(Q, dtype=LD)
    return float(np.max(np.abs(Q.T @ Q - np.eye(Q.shape[1], dtype=LD))))


def svd_residuals(A, US, S, Vt):
    """(max |US Vt - A| / max |A|,  max |Vt Vt^T - I|,  max |U^T U - I| with U the columns of US over S where S > 0,
    max | ||US_j|| - S_j | / S_0), in long double."""
    A, US, S, Vt = (np.asarray(x, dtype=LD) for x in (A, US, S, Vt))
    n = Vt.shape[0]
    recon = float(np.max(np.abs(US @ Vt - A)) / np.max(np.abs(A)))
    v_orth = float(np.max(np.abs(Vt @ Vt.T - np.eye(n, dtype=LD))))
    keep = S > 0
    U = US[:, keep] / S[keep]
    u_orth = float(np.max(np.abs(U.T @ U - np.eye(U.shape[1], dtype=LD)))) if U.shape[1] else 0.0
    norms = float(np.max(np.abs(np.sqrt(np.sum(US * US, axis=0)) - S)) / S[0])
    return recon, v_orth, u_orth, norms
