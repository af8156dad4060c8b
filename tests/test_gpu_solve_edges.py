"""The small dense solves at every edge of their dispatch, element by element against long-double references.

ttsk_qr_thin, ttsk_pinv / _begin / _end / _batch / _batch_deferred, ttsk_orth_step / _orth_step_pinv, ttsk_svd_small and
ttsk_triu (csrc/cholesky.hip, householder.hip, jacobi.hip, pinv.hip), called through the C entry points.  The references
are tests/solve_ref.py (np.longdouble, no LAPACK in an answer; tests/test_solve_ref_host.py holds them against LAPACK).

THE ONE ACCEPTANCE RULE.  For every case e_lapack = col_err(numpy / scipy fp64 result, reference) on the same input,
floored at 4 eps; the device passes with col_err(device, reference) <= 32 e_lapack where its route is backward stable (the
Householder kernels, Jacobi) and <= 32 kappa e_lapack on a normal-equations / CholeskyQR fast path, documented as costing up
to one further factor kappa.  col_err is the worst column's max |d| / max |ref|: nothing is averaged in a norm.  Edge cases
have kappa <= 30, so every bar is below ~1e-11.  The 32 is a guess at the constant between methods of one order and is
NOT tuned to the device: a case beyond its bar is a finding.  The worst err / e_lapack per route is printed when the
module ends; DESIGN.md section 2 records the last run.

Every boundary shape is computed from the constants of the sources, which are read from the sources (src_const): a constant
that moves takes its shapes with it.  The values in the comments are those of today's constants.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import scipy.linalg

from tests import solve_ref as sr
from tests.edge_kit import same_bits, tsa  # noqa: F401

pytestmark = pytest.mark.gpu

LD, EPS = sr.LD, sr.EPS
MARGIN = 32.0
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tt_sketch_amd", "csrc")


def src_const(fname, name):
    """the value of `name = <arithmetic>;` in a source file"""
    with open(os.path.join(CSRC, fname)) as f:
        m = re.search(r"\b%s\s*=\s*([^;]+);" % name, f.read())
    assert m and re.fullmatch(r"[0-9eE.+\-*/ ()]+", m.group(1)), (fname, name)
    return eval(m.group(1))


SMALL_QR_MAX = src_const("cholesky.hip", "SMALL_QR_MAX")          # 19000 doubles of LDS for small_qr_kernel (m n + n)
CHOL_SIGN_MAX = src_const("cholesky.hip", "CHOL_SIGN_MAX")        # 72: second factorisation + signs in one kernel
CHOL_ONE_N = src_const("linalg_int.h", "CHOL_ONE_N")              # 128: one workgroup's Cholesky
CHOL_MAX_N = src_const("linalg_int.h", "CHOL_MAX_N")              # 256: the 2 x 2 block Cholesky
CHOL_GATE = src_const("linalg_int.h", "CHOL_GATE")                # 1 / 300: diag(R) spread ttsk_pinv's normal equations accept
CHOL_GATE_REFINED = src_const("linalg_int.h", "CHOL_GATE_REFINED")  # 1 / 3e4: the same with the Newton-Schulz step (deferred)
PINV_FAST_RCOND = src_const("linalg_int.h", "PINV_FAST_RCOND")    # 1e-4: a larger rcond skips the normal equations
QR_ROWS = src_const("householder.hip", "QR_ROWS")                 # 128 rows per workgroup of the Householder launches
JAC_CAP = src_const("jacobi.hip", "cap")                          # 160 * 1024 - 256 bytes of LDS for the Jacobi kernel
QR_GATE = 1e-6                # qr_cholesky: diag(R) spread CholeskyQR2 accepts (a literal at its two chol_inv_any / launch calls)
PINV_MAX_N = 1024             # ttsk_pinv_begin / _end: min(l, r) beyond it is TTSK_ERR_ARG (a literal in both)
TRIU_GRID = 1024 * 256        # ttsk_triu: at most 1024 workgroups of 256 threads, a grid-stride loop beyond


def jacobi_lds_mode(mW, nW):
    """jacobi.hip: 2 = W and V in LDS, 1 = W only, 0 = global scratch"""
    small, w, v = (nW + (nW + 1) // 2) * 8, mW * nW * 8, nW * nW * 8
    return 2 if small + w + v <= JAC_CAP else (1 if small + w <= JAC_CAP else 0)


def last_rows(nW, mode):
    """the tallest mW x nW matrix that still gets `mode`"""
    mW = nW
    assert jacobi_lds_mode(mW, nW) >= mode
    while jacobi_lds_mode(mW + 1, nW) >= mode:
        mW += 1
    return mW


def last_square(mode):
    n = 1
    while jacobi_lds_mode(n + 1, n + 1) >= mode:
        n += 1
    return n


def largest(pred, lo=1):
    n = lo
    while pred(n + 1):
        n += 1
    return n


N_SQ = largest(lambda n: n * n + n <= SMALL_QR_MAX)               # 137: the largest square small_qr_kernel takes
N_HALF = largest(lambda n: (2 * n - 1) * n + n <= SMALL_QR_MAX)   # 97: the largest n it takes at m = 2 n - 1
JW = 64                                                           # the narrow side of the rectangular Jacobi cases
J2, J1 = last_rows(JW, 2), last_rows(JW, 1)                       # 254, 318: last mW with W and V / with W in LDS at nW = 64
S2, S1 = last_square(2), last_square(1)                           # 100, 142: the same for square matrices


# ------------------------------------------------------------------ plumbing
WORST = {}        # route -> (worst err / e_lapack, case)


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    print("\nworst err / e_lapack per route (stable bar 32, fast bar 32 kappa):")
    for route in sorted(WORST):
        print(f"  {route:34s} {WORST[route][0]:9.2f}   at {WORST[route][1]}")


_CACHE = {}


def cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def rng_for(*key):
    return np.random.default_rng([int(k) for k in key])


def nat():
    from tt_sketch_amd import _native
    return _native


def dev(a, stream=0):
    from tt_sketch_amd.device import DevArray
    return DevArray.from_host(np.ascontiguousarray(a, dtype=np.float64), stream=stream)


def dev_nan(shape):
    return dev(np.full(shape, np.nan))


def sync():
    nat().call("ttsk_sync", -1)


def accept(route, case, got, ref, lapack, kappa=None, extra=0.0):
    """the one acceptance rule; kappa = None: the stable bar"""
    e_lapack = max(sr.col_err(lapack, ref), 4 * EPS)
    err = sr.col_err(got, ref)
    bar = MARGIN * (kappa if kappa else 1.0) * e_lapack + extra
    ratio = err / e_lapack
    if ratio > WORST.get(route, (-1.0, None))[0]:
        WORST[route] = (ratio, case)
    print(f"{route} {case}: err {err:.2e}  e_lapack {e_lapack:.2e}  ratio {ratio:.2f}  bar {bar:.2e}")
    assert np.all(np.isfinite(got)), (route, case)
    assert err <= bar, (route, case, err, bar)


def full_rank(l, r, kappa, tag=0):
    """(l, r) fp64 with singular values 1 .. 1 / kappa, its condition number checked"""
    def make():
        A = sr.prescribed(max(l, r), min(l, r), kappa, rng_for(l, r, kappa, tag))
        A = A if l >= r else np.ascontiguousarray(A.T)
        assert sr.cond_is(A, kappa), (l, r, kappa, np.linalg.cond(A))
        return A
    return cached(("A", l, r, kappa, tag), make)


def chol_spread(A):
    """min / max of diag(R), R^T R the Gram matrix of the short side: what the Cholesky gates compare (0: not positive definite)"""
    G = A @ A.T if A.shape[0] <= A.shape[1] else A.T @ A
    try:
        d = np.diag(np.linalg.cholesky(G))
    except np.linalg.LinAlgError:
        return 0.0
    return float(d.min() / d.max())


def pinv_ref(l, r, kappa, tag=0):
    """(A, long-double pinv, numpy's pinv) of a full-rank case"""
    def make():
        A = full_rank(l, r, kappa, tag)
        return A, sr.pinv_full(A, agree=sr.NS_AGREE if kappa <= 100 else sr.NS_AGREE_ILL), np.linalg.pinv(A)
    return cached(("pinv", l, r, kappa, tag), make)


ILL_KAPPA = 3000


def ill_tag(l, r, rejected=True):
    """The gates compare min / max of diag(R), which bounds kappa from below only: for singular values spread evenly in the
    logarithm over 1 .. 1 / 3000 the median of that ratio over draws of the factors is 1 / 270 (200 x 64, 40 draws: 1 / 460
    .. 1 / 185), so CHOL_GATE = 1 / 300 takes about half of such matrices.  A case that says `rejected` (or `accepted`) walks
    the seed until its matrix is, 10 % clear of the gate: the first tag with that property."""
    def make():
        for tag in range(100, 400):
            s = chol_spread(full_rank(l, r, ILL_KAPPA, tag))
            if (s < 0.9 * CHOL_GATE) if rejected else (s > 1.1 * CHOL_GATE):
                return tag
        raise AssertionError(f"no ({l}, {r}) matrix with kappa = {ILL_KAPPA} on that side of the gate in 300 draws")
    return cached(("ill", l, r, rejected), make)


# ------------------------------------------------------------------ ttsk_qr_thin
def c_qr_thin(A):
    d = dev(A)
    nat().call("ttsk_qr_thin", d, A.shape[0], A.shape[1], 0)
    return d.get()


# (route, m, n, kappa, columns scaled, bar); bar "fast": CholeskyQR2 decides, "stable": a Householder kernel does
QR_CASES = []


def _qr(route, shapes, kappa, bar, scaled=False):
    QR_CASES.extend((route, m, n, kappa if n > 1 else 1, scaled, bar) for m, n in shapes)      # one column: one singular value


# small_qr_kernel (m < 2 n and m n + n <= SMALL_QR_MAX), square: the last reflector is the identity
_qr("small_qr square", [(1, 1), (2, 2), (17, 17), (N_SQ, N_SQ)], 30, "stable")                     # ... (137, 137)
# one past its LDS limit: n > CHOL_ONE_N, so the two-block CholeskyQR2 and hh_sign_scale_global_kernel with the square rule
_qr("cholqr2 two-block square", [(N_SQ + 1, N_SQ + 1)], 30, "fast")                                   # (138, 138)
# m = 2 n - 1 at the largest n the LDS takes, and the next n (CholeskyQR2 then)
_qr("small_qr m=2n-1", [(2 * N_HALF - 1, N_HALF)], 10, "stable")                                      # (193, 97)
_qr("cholqr2 past small_qr", [(2 * N_HALF + 1, N_HALF + 1)], 10, "fast")                              # (195, 98)
# the fused sign kernel (n <= CHOL_SIGN_MAX) and hh_sign_scale_kernel behind it, at m = 2 n (the first m that is not
# small_qr_kernel's) and taller
_qr("cholqr2 fused signs", [(2 * CHOL_SIGN_MAX, CHOL_SIGN_MAX), (500, CHOL_SIGN_MAX)], 10, "fast")    # (144, 72) (500, 72)
_qr("cholqr2 hh_sign_scale", [(2 * CHOL_SIGN_MAX + 2, CHOL_SIGN_MAX + 1), (500, CHOL_SIGN_MAX + 1), (300, CHOL_ONE_N)], 10, "fast")
# ^ (146, 73) (500, 73) (300, 128);  v (300, 129) (600, 255) (600, 256) (256, 256): n1 = roundup16((n + 1) / 2), n2 = n - n1
_qr("cholqr2 two-block", [(300, CHOL_ONE_N + 1), (600, CHOL_MAX_N - 1), (600, CHOL_MAX_N)], 10, "fast")
_qr("cholqr2 two-block square", [(CHOL_MAX_N, CHOL_MAX_N)], 10, "fast")
# n > CHOL_MAX_N: nothing but the Householder launches
_qr("householder launches", [(300, CHOL_MAX_N + 1), (CHOL_MAX_N + 1, CHOL_MAX_N + 1)], 10, "stable")  # (300, 257) (257, 257)
# CholeskyQR2 rejected (columns scaled by 1 .. 1e-8: diag(R) spread beyond QR_GATE), the Householder launches behind it with
# blocks_at(j) = ceil((m - j) / QR_ROWS) constant (128), dropping 2 -> 1 at j = 1 (129) and j = 2 (130), 4 -> 3 at j = 1
# (385), 3 -> 2 at j = 4 with the two-block Cholesky as the rejected attempt (260, 130)
_qr("householder after rejection", [(QR_ROWS, 5), (QR_ROWS + 1, 5), (QR_ROWS + 2, 5), (3 * QR_ROWS + 1, 12),
                                     (2 * (CHOL_ONE_N + 2), CHOL_ONE_N + 2)], 10, "stable", scaled=True)
# n = 1 (one singular value: kappa = 1)
_qr("cholqr2 n=1", [(5, 1), (QR_ROWS + 1, 1)], 1, "fast")


def qr_ref(m, n, kappa, scaled):
    def make():
        A = full_rank(m, n, kappa, 1)
        if scaled:
            A = A * np.logspace(0, -8, n)
        Q = sr.hh_qr(A)
        Qs, _ = scipy.linalg.qr(A, mode="economic")
        return A, Q, Qs
    return cached(("qr", m, n, kappa, scaled), make)


@pytest.mark.parametrize("route,m,n,kappa,scaled,bar", QR_CASES, ids=[f"{c[1]}x{c[2]}" for c in QR_CASES])
def test_qr_thin(tsa, route, m, n, kappa, scaled, bar):
    A, Qref, Qs = qr_ref(m, n, kappa, scaled)
    if scaled:
        assert chol_spread(A) < QR_GATE / 4, "the case has to be one CholeskyQR2 rejects"
    elif bar == "fast":
        assert chol_spread(A) > 4 * QR_GATE, "the case has to be one CholeskyQR2 accepts"
    Q = c_qr_thin(A)
    orth = sr.orth_err(Q)
    print(f"{route} ({m}, {n}): max |Q^T Q - I| = {orth:.2e}  bar {MARGIN * n * EPS:.2e}")
    accept("qr_thin: " + route, (m, n), Q, Qref, Qs, kappa if bar == "fast" else None)
    assert orth <= MARGIN * n * EPS


# ------------------------------------------------------------------ ttsk_pinv
def c_pinv(A, rcond, with_rank, entry="ttsk_pinv"):
    l, r = A.shape
    d_om, d_p = dev(A), dev_nan((r, l))
    rk = ctypes.c_int(-7)
    nat().call(entry, d_om, l, r, float(rcond), d_p, ctypes.byref(rk) if with_rank else None, 0)
    sync()
    return d_p.get(), (rk.value if with_rank else None)


def pinv_both(A, rcond, true_rank):
    """ttsk_pinv with host_rank and with host_rank == NULL (the predicated Jacobi launch): bit-identical, the rank right"""
    P, rk = c_pinv(A, rcond, True)
    P0, _ = c_pinv(A, rcond, False)
    same_bits(P, P0, "host_rank == NULL must give the same bits as the read-back form: P")
    assert rk == true_rank
    return P


# (route, l, r, kappa, rcond, bar)
PINV_CASES = []
REJECTED, ACCEPTED_ILL = "jacobi after rejection", "normal equations at the gate"


def _pinv(route, shapes, kappa, rcond, bar, both=False):
    for l, r in shapes:
        PINV_CASES.append((route, l, r, kappa, rcond, bar))
        if both and l != r:
            PINV_CASES.append((route, r, l, kappa, rcond, bar))


# normal equations with the one-workgroup Cholesky (min(l, r) <= CHOL_ONE_N): wide, tall, square; one singular value
_pinv("normal equations", [(CHOL_ONE_N, 300), (300, CHOL_ONE_N), (CHOL_ONE_N, CHOL_ONE_N)], 10, -1.0, "fast")     # 128
_pinv("normal equations", [(1, 4), (4, 1), (1, 1)], 1, -1.0, "fast")
# ... with the two-block Cholesky (CHOL_ONE_N < min(l, r) <= CHOL_MAX_N)
_pinv("normal equations two-block", [(CHOL_ONE_N + 1, 140), (140, CHOL_ONE_N + 1), (CHOL_MAX_N - 1, CHOL_MAX_N),
                                     (CHOL_MAX_N, 600)], 10, -1.0, "fast")                                 # 129, 255, 256
# min(l, r) > CHOL_MAX_N: no attempt, Jacobi alone
_pinv("jacobi beyond the fast limit", [(CHOL_MAX_N + 1, 300)], 10, -1.0, "stable")                          # (257, 300)
# kappa = 3000 and diag(R) spread beyond CHOL_GATE: the attempt is rejected and the Jacobi kernel behind it decides
_pinv(REJECTED, [(JW, 200), (200, JW)], ILL_KAPPA, -1.0, "stable")
# the same kappa with diag(R) spread within the gate (ill_tag): accepted, and the normal equations' further factor kappa is
# what the result costs -- not a case of the issue's table; it pins what the gate lets through
_pinv(ACCEPTED_ILL, [(JW, 200), (200, JW)], ILL_KAPPA, -1.0, "fast")
# rcond = 1e-3 > PINV_FAST_RCOND: no attempt (nothing is truncated at kappa = 10); each LDS mode of the Jacobi kernel on
# both sides of its boundary, both orientations
_pinv("jacobi lds modes", [(JW, J2), (JW, J2 + 1), (JW, J1), (JW, J1 + 1)], 10, 1e-3, "stable", both=True)  # 254 255 318 319
_pinv("jacobi lds modes square", [(S2, S2), (S2 + 1, S2 + 1), (S1, S1), (S1 + 1, S1 + 1)], 10, 1e-3, "stable")  # 100 101 142 143


@pytest.mark.parametrize("route,l,r,kappa,rcond,bar", PINV_CASES, ids=[f"{c[1]}x{c[2]}" + ("-accepted" if c[0] == ACCEPTED_ILL else "") for c in PINV_CASES])
def test_pinv_full_rank(tsa, route, l, r, kappa, rcond, bar):
    assert (rcond > PINV_FAST_RCOND) == route.startswith("jacobi lds")
    tag = ill_tag(l, r, route == REJECTED) if route in (REJECTED, ACCEPTED_ILL) else 0
    A, Pref, Pnp = pinv_ref(l, r, kappa, tag)
    if route.startswith("normal") and route != ACCEPTED_ILL:
        assert chol_spread(A) > 2 * CHOL_GATE, "the case has to be one the gate accepts"
    P = pinv_both(A, rcond, min(l, r))
    accept("pinv: " + route, (l, r), P, Pref, Pnp, kappa if bar == "fast" else None)


def rank_k_case(l, r, k):
    def make():
        B, C = sr.int_factors(l, r, k, rng_for(l, r, k))
        return B @ C, B, C, sr.pinv_rank_k(B, C)
    return cached(("rank_k", l, r, k), make)


@pytest.mark.parametrize("l,r,k", [(40, 90, 7), (90, 40, 7), (8, 12, 3)])
def test_pinv_exactly_rank_deficient(tsa, l, r, k):
    """A = B C with integer factors: exact in fp64 and exactly of rank k; rcond = -1 (eps, with the rank floor of pinv_rcond)"""
    A, B, C, Pref = rank_k_case(l, r, k)
    P = pinv_both(A, -1.0, k)
    accept("pinv: jacobi rank deficient", (l, r, k), P, Pref, np.linalg.pinv(A, rcond=1e-10))


def test_pinv_truncation_by_rcond(tsa):
    """(30, 50): an integer rank-3 A3 plus two directions of size 1e-7 and 1e-8 max |A3| that are orthogonal to its row and
    column spaces; rcond = 1e-4 drops them, and the truncated pseudo-inverse is that of A3 -- exactly, up to the rounding
    of the sum.  The bar is the stable one plus the first-order effect of the perturbation, 2e-7 ||A3^+|| max |A3|."""
    l, r, k = 30, 50, 3
    A3, B, C, Pref = rank_k_case(l, r, k)
    rng = rng_for(l, r, k, 1)
    U = np.linalg.qr(np.c_[B, rng.standard_normal((l, 2))])[0][:, k:]          # two directions orthogonal to range(A3)
    V = np.linalg.qr(np.c_[C.T, rng.standard_normal((r, 2))])[0][:, k:]        # ... and to range(A3^T)
    a = np.max(np.abs(A3))
    A = A3 + a * ((U * np.array([1e-7, 1e-8])) @ V.T)
    s = np.linalg.svd(A, compute_uv=False)
    assert s[2] > 1e-3 * s[0] and s[3] < 1e-5 * s[0]                           # rcond = 1e-4 sits well inside the gap
    P = pinv_both(A, 1e-4, k)
    extra = 2e-7 * float(np.linalg.norm(Pref.astype(np.float64), 2)) * a
    accept("pinv: jacobi truncation", (l, r, k), P, Pref, np.linalg.pinv(A, rcond=1e-4), extra=extra)


def test_pinv_limits(tsa):
    """min(l, r) = 1025 and l = 0: TTSK_ERR_ARG, nothing queued (the output keeps its bits)"""
    n = PINV_MAX_N + 1
    d_om, d_p = dev(np.ones((n, n))), dev(np.full((n, n), 7.25))
    for entry in ("ttsk_pinv", "ttsk_pinv_begin"):
        with pytest.raises(ValueError):
            nat().call(entry, d_om, n, n, -1.0, d_p, *(() if entry.endswith("begin") else (None,)), 0)
    with pytest.raises(ValueError):
        nat().call("ttsk_pinv_end", d_om, n, n, -1.0, d_p, None, 0)
    with pytest.raises(ValueError):
        nat().call("ttsk_pinv", d_om, 0, 5, -1.0, d_p, None, 0)
    with pytest.raises(ValueError):
        nat().call("ttsk_pinv", d_om, 5, 0, -1.0, d_p, None, 0)
    sync()
    assert np.all(d_p.get() == 7.25)


def test_pinv_begin_end_on_two_streams(tsa):
    """begin on streams 0 and 1 -- one matrix the gate accepts, one it rejects -- then both ends: each result has the bits
    of the single call, with the rank read back and without"""
    cases = [(CHOL_ONE_N, 300, 10, 0), (JW, 200, ILL_KAPPA, ill_tag(JW, 200))]
    mats = [pinv_ref(*c)[0] for c in cases]
    single = [c_pinv(A, -1.0, True)[0] for A in mats]
    for with_rank in (True, False):
        for order in ((0, 1), (1, 0)):                    # accepted on stream 0 / rejected on stream 1, and the other way round
            d_om = [dev(A) for A in mats]
            d_p = [dev_nan(A.T.shape) for A in mats]
            sync()
            rk = [ctypes.c_int(-7), ctypes.c_int(-7)]
            for i, s in enumerate(order):
                nat().call("ttsk_pinv_begin", d_om[i], *mats[i].shape, -1.0, d_p[i], s)
            for i, s in enumerate(order):
                nat().call("ttsk_pinv_end", d_om[i], *mats[i].shape, -1.0, d_p[i], ctypes.byref(rk[i]) if with_rank else None, s)
            sync()
            for i in range(2):
                same_bits(d_p[i].get(), single[i], str((with_rank, order, i)))
                if with_rank:
                    assert rk[i].value == min(mats[i].shape)


# ------------------------------------------------------------------ ttsk_pinv_batch, ttsk_pinv_batch_deferred
def c_pinv_batch(entry, mats, slots, stream=0):
    """the matrices at the given slots of one input buffer (and of one output buffer): equal slots apart or not"""
    from tt_sketch_amd.device import DevArray
    l, r = mats[0].shape
    host = np.full((max(slots) + 1, l * r), np.nan)
    for A, s in zip(mats, slots):
        host[s] = A.ravel()
    d_in, d_out = dev(host), dev_nan((max(slots) + 1, r * l))
    ins, outs = [d_in[s] for s in slots], [d_out[s] for s in slots]
    assert all(isinstance(v, DevArray) for v in ins)
    nat().call(entry, len(mats), nat().ptr_array(ins), l, r, nat().ptr_array(outs), stream)
    sync()
    out = d_out.get()
    unused = [s for s in range(max(slots) + 1) if s not in slots]
    assert all(np.all(np.isnan(out[s])) for s in unused), "a slot between the matrices was written"
    return [out[s].reshape(r, l) for s in slots]


def deferred_flag(stream=0):
    f = ctypes.c_int(-7)
    nat().call("ttsk_deferred_status", stream, ctypes.byref(f))
    return f.value


BATCH_SHAPES = [(CHOL_ONE_N, 150), (150, CHOL_ONE_N)]       # the widest the batched fast path takes, both orientations


@pytest.mark.parametrize("entry", ["ttsk_pinv_batch", "ttsk_pinv_batch_deferred"])
@pytest.mark.parametrize("l,r", BATCH_SHAPES)
@pytest.mark.parametrize("slots", [(0,), (0, 1, 2), (0, 2, 3)], ids=["count1", "spaced", "unequal"])
def test_pinv_batch(tsa, entry, l, r, slots):
    deferred_flag()
    refs = [pinv_ref(l, r, 10, tag) for tag in range(len(slots))]
    got = c_pinv_batch(entry, [x[0] for x in refs], slots)
    for b, ((A, Pref, Pnp), P) in enumerate(zip(refs, got)):
        accept(f"{entry[5:]}: normal equations", (l, r, len(slots), b), P, Pref, Pnp, 10)
    assert deferred_flag() == 0


# (64, 100) beside the shapes above: small enough for W and V in LDS, where equally spaced matrices share ONE Jacobi launch
@pytest.mark.parametrize("l,r", BATCH_SHAPES + [(JW, 100), (100, JW)])
@pytest.mark.parametrize("slots", [(0, 1, 2), (0, 2, 3)], ids=["spaced", "unequal"])
def test_pinv_batch_with_a_rejected_matrix(tsa, l, r, slots):
    """matrix 1 of three at kappa = 3000, rejected by CHOL_GATE (ill_tag): ttsk_pinv_batch still returns its pseudo-inverse
    (Jacobi behind the attempt, predicated per matrix), at the stable bar"""
    assert (jacobi_lds_mode(max(l, r), min(l, r)) == 2) == (min(l, r) == JW)
    refs = [pinv_ref(l, r, 10, 0), pinv_ref(l, r, ILL_KAPPA, ill_tag(l, r)), pinv_ref(l, r, 10, 2)]
    got = c_pinv_batch("ttsk_pinv_batch", [x[0] for x in refs], slots)
    for b, ((A, Pref, Pnp), P) in enumerate(zip(refs, got)):
        if b == 1:
            accept("pinv_batch: jacobi after rejection", (l, r, 3, b), P, Pref, Pnp)
        else:
            accept("pinv_batch: normal equations", (l, r, 3, b), P, Pref, Pnp, 10)


DEFERRED_GATE_REASON = (
    "the contract stated for this case does not hold: ttsk_pinv_batch_deferred runs the normal equations with a Newton-Schulz "
    "step behind them and gates at diag(R) spread 1 / CHOL_GATE_REFINED = 3e4 (linalg_int.h, pinv.hip), not at the 300 of "
    "ttsk_pinv; the spread never exceeds kappa, so kappa = 3000 is always accepted and refined, and no flag is raised; the "
    "flag itself is covered at kappa = 1e7 beside it")


@pytest.mark.parametrize("l,r", BATCH_SHAPES)
@pytest.mark.parametrize("kappa", [pytest.param(3000, marks=pytest.mark.xfail(strict=True, reason=DEFERRED_GATE_REASON)), 10 ** 7])
def test_pinv_batch_deferred_raises_the_flag(tsa, l, r, kappa):
    """matrix 1 of three ill conditioned: the stream's deferred flag is raised; ttsk_deferred_status reads it once, a
    second read gives 0"""
    deferred_flag()
    mats = [full_rank(l, r, 10, 0), full_rank(l, r, kappa, 0), full_rank(l, r, 10, 2)]
    if kappa > ILL_KAPPA:
        assert chol_spread(mats[1]) < CHOL_GATE_REFINED / 2
    c_pinv_batch("ttsk_pinv_batch_deferred", mats, (0, 1, 2))
    first, second = deferred_flag(), deferred_flag()
    assert (first, second) == (1, 0)


@pytest.mark.parametrize("entry", ["ttsk_pinv_batch", "ttsk_pinv_batch_deferred"])
def test_pinv_batch_refuses_beyond_one_workgroup(tsa, entry):
    l, r = CHOL_ONE_N + 1, 150                                      # (129, 150)
    d_in, d_out = dev(full_rank(l, r, 10)), dev(np.full((r, l), 7.25))
    with pytest.raises(nat().TtskUnsupported):
        nat().call(entry, 1, nat().ptr_array([d_in]), l, r, nat().ptr_array([d_out]), 0)
    sync()
    assert np.all(d_out.get() == 7.25)


# ------------------------------------------------------------------ ttsk_orth_step, ttsk_orth_step_pinv
# k on both sides of the fused sign kernel's limit, of the one-workgroup Cholesky's, and at the two-block Cholesky's
ORTH_L = [CHOL_SIGN_MAX, CHOL_SIGN_MAX + 1, CHOL_ONE_N, CHOL_ONE_N + 1, CHOL_MAX_N]          # 72, 73, 128, 129, 256
ORTH_KAPPA = 10


def orth_case(l):
    """Psi = M Omega in long double, rounded to fp64 (M (3 l, l), Omega (l, l + 10), kappa = 10 both); the reference Q is
    hh_qr(Psi pinv(Omega)) in long double; LAPACK's is scipy's QR of the fp64 product with numpy's pinv"""
    def make():
        m, r2 = 3 * l, l + 10
        M, Om = full_rank(m, l, ORTH_KAPPA, 3), full_rank(l, r2, ORTH_KAPPA, 3)
        Psi = (M.astype(LD) @ Om.astype(LD)).astype(np.float64)
        Qref = sr.hh_qr(Psi.astype(LD) @ sr.pinv_full(Om))
        Qs, _ = scipy.linalg.qr(Psi @ np.linalg.pinv(Om), mode="economic")
        return Psi, Om, Qref, Qs
    return cached(("orth", l), make)


@pytest.mark.parametrize("l", ORTH_L)
def test_orth_step(tsa, l):
    Psi, Om, Qref, Qs = orth_case(l)
    m, r2 = Psi.shape
    deferred_flag()
    d_psi, d_om, d_q = dev(Psi), dev(Om), dev_nan((m, l))
    nat().call("ttsk_orth_step", d_psi, m, r2, d_om, l, d_q, 0)
    assert deferred_flag() == 0
    accept("orth_step", (m, r2, l), d_q.get(), Qref, Qs, ORTH_KAPPA)
    same_bits(d_psi.get(), Psi, "Psi")
    same_bits(d_om.get(), Om, "Omega")


@pytest.mark.parametrize("l", ORTH_L)
def test_orth_step_pinv(tsa, l):
    """the same Q from the device's own ttsk_pinv output"""
    Psi, Om, Qref, Qs = orth_case(l)
    m, r2 = Psi.shape
    deferred_flag()
    d_psi, d_om, d_p, d_q = dev(Psi), dev(Om), dev_nan((r2, l)), dev_nan((m, l))
    nat().call("ttsk_pinv", d_om, l, r2, -1.0, d_p, None, 0)
    nat().call("ttsk_orth_step_pinv", d_psi, m, r2, d_p, l, d_q, 0)
    assert deferred_flag() == 0
    accept("orth_step_pinv", (m, r2, l), d_q.get(), Qref, Qs, ORTH_KAPPA)


@pytest.mark.parametrize("k", ORTH_L)
def test_orth_step_without_omega(tsa, k):
    """Omega == NULL: Q = qr_thin(Psi), k = r2 columns (a Psi of full column rank: M itself); and in place, dev_q == dev_psi"""
    m = 3 * k
    A, Qref, Qs = qr_ref(m, k, ORTH_KAPPA, False)
    deferred_flag()
    d_psi, d_q = dev(A), dev_nan((m, k))
    nat().call("ttsk_orth_step", d_psi, m, k, None, 0, d_q, 0)
    assert deferred_flag() == 0
    Q = d_q.get()
    accept("orth_step, no Omega", (m, k), Q, Qref, Qs, ORTH_KAPPA)
    nat().call("ttsk_orth_step", d_psi, m, k, None, 0, d_psi, 0)
    assert deferred_flag() == 0
    same_bits(d_psi.get(), Q, "Psi")


def test_orth_step_limits(tsa):
    l = CHOL_MAX_N + 1                                              # 257: TTSK_ERR_UNSUPPORTED
    m, r2 = 3 * l, l + 10
    d_psi, d_om, d_p, d_q = dev(np.ones((m, r2))), dev(np.ones((l, r2))), dev(np.ones((r2, l))), dev(np.full((m, l), 7.25))
    with pytest.raises(nat().TtskUnsupported):
        nat().call("ttsk_orth_step", d_psi, m, r2, d_om, l, d_q, 0)
    with pytest.raises(nat().TtskUnsupported):
        nat().call("ttsk_orth_step_pinv", d_psi, m, r2, d_p, l, d_q, 0)
    with pytest.raises(nat().TtskUnsupported):
        nat().call("ttsk_orth_step", d_psi, m, l, None, 0, d_q, 0)
    # m < k: TTSK_ERR_ARG
    with pytest.raises(ValueError):
        nat().call("ttsk_orth_step", d_psi, 19, 30, d_om, 20, d_q, 0)
    with pytest.raises(ValueError):
        nat().call("ttsk_orth_step", d_psi, 19, 20, None, 0, d_q, 0)
    with pytest.raises(ValueError):
        nat().call("ttsk_orth_step_pinv", d_psi, 19, 30, d_p, 20, d_q, 0)
    sync()
    assert np.all(d_q.get() == 7.25)


# ------------------------------------------------------------------ ttsk_svd_small
def c_svd(A):
    m, n = A.shape
    d_a, d_us, d_s, d_vt = dev(A), dev_nan((m, n)), dev_nan((n,)), dev_nan((n, n))
    nat().call("ttsk_svd_small", d_a, m, n, d_us, d_s, d_vt, 0)
    sync()
    return d_us.get(), d_s.get(), d_vt.get()


def check_svd(A, case):
    """the four residuals of solve_ref.svd_residuals, each at most 32 x numpy's on this input (floored at 4 eps as e_lapack
    is: below that an fp64 residual is rounding luck -- numpy's is exactly 0 for one column), S >= 0 descending and equal
    to numpy's to 32 n eps S_0.  No vector is compared."""
    m, n = A.shape
    US, S, Vt = c_svd(A)
    U, Sn, Vtn = np.linalg.svd(A, full_matrices=False)
    assert np.all(np.isfinite(US)) and np.all(np.isfinite(S)) and np.all(np.isfinite(Vt))
    got, ref = sr.svd_residuals(A, US, S, Vt), sr.svd_residuals(A, U * Sn, Sn, Vtn)
    names = ("US Vt - A", "Vt Vt^T - I", "U^T U - I", "|US_j| - S_j")
    for name, g, e in zip(names, got, ref):
        e = max(e, 4 * EPS)
        route = "svd_small: " + name
        if g / e > WORST.get(route, (-1.0, None))[0]:
            WORST[route] = (g / e, case)
        print(f"{route} {case}: {g:.2e}  numpy {e:.2e}  ratio {g / e:.2f}")
        assert g <= MARGIN * e, (name, case, g, e)
    assert np.all(S >= 0) and np.all(S[:-1] >= S[1:])
    assert np.max(np.abs(S - Sn)) <= MARGIN * n * EPS * Sn[0]


# both sides of each LDS mode of the Jacobi kernel (factor mode: l >= r, untransposed), and the smallest
SVD_SHAPES = [(J2, JW), (J2 + 1, JW), (J1, JW), (J1 + 1, JW), (S2, S2), (S2 + 1, S2 + 1), (S1, S1), (S1 + 1, S1 + 1), (1, 1), (7, 1)]


@pytest.mark.parametrize("m,n", SVD_SHAPES)
def test_svd_small(tsa, m, n):
    check_svd(full_rank(m, n, 100 if n > 1 else 1, 4), (m, n))


def test_svd_small_with_two_equal_singular_values(tsa):
    rng = rng_for(40, 12)
    U, _ = np.linalg.qr(rng.standard_normal((40, 12)))
    V, _ = np.linalg.qr(rng.standard_normal((12, 12)))
    s = np.logspace(0, -2, 12)
    s[4] = s[3]
    check_svd((U * s) @ V.T, (40, 12, "s3 == s4"))


# ------------------------------------------------------------------ ttsk_triu
# (600, 500) = 300000 elements is past one pass of the grid-stride loop (TRIU_GRID = 262144 threads)
@pytest.mark.parametrize("m,n", [(1, 1), (5, 3), (3, 5), (300, 300), (600, 500)])
def test_triu_is_bit_exact(tsa, m, n):
    assert (m * n > TRIU_GRID) == ((m, n) == (600, 500))
    A = rng_for(m, n).standard_normal((m, n))
    d = dev(A)
    nat().call("ttsk_triu", d, m, n, 0)
    same_bits(d.get(), np.triu(A), "R")
