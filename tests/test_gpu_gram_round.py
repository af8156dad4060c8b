"""Gram-SVD rounding on the device: ``ttsk_gram_round_bonds`` (csrc/gram_round.hip) called directly with guard bands round
every output, and the Python surface on it (``TensorTrain.round_gram`` / ``svdvals_gram``, ``round_tt_sum(method="gram")``).

Bars.  The bond kernel: the deviations of the NumPy restatement (tests/gram_round_ref.py) from the dense truths on the same
inputs, recorded beside each case and held on the CPU by tests/test_gram_round_host.py, times 16, with a floor of 1e-13
(Jacobi and LAPACK eigenvectors differ by rotations inside clusters).  ``round_gram`` against ``round``: equal ranks, the
error against the input within ``ERROR_RATIO_CAP`` of ``round``'s, the figure measured on the CPU.  Errors of a train
against its input are the QR norm of the difference of the two trains on the host: no dense array beyond 10^5 entries."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import gram_round_ref as gr
from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3
GUARD = 32                     # doubles on either side of every output
SENTINEL = 12345.678


# ---------------------------------------------------------------- 1. the bond kernel alone
class _Banded:
    """a device buffer of `n` doubles between two guard bands, all SENTINEL before the call"""

    def __init__(self, n):
        from tt_sketch_amd.device import DevArray
        self.n = n
        self.buf = DevArray.from_host(np.full(n + 2 * GUARD, SENTINEL))
        self.ptr = self.buf.ptr + 8 * GUARD

    def read(self):
        a = self.buf.get()
        assert (a[:GUARD] == SENTINEL).all() and (a[GUARD + self.n:] == SENTINEL).all(), "a guard band was written"
        return a[GUARD:GUARD + self.n]


def c_bonds(GL, GR, ranks, caps, eps):
    """One direct call of the C entry on host Grams: (status, [P^T], [Q], [Sigma], chosen ranks)."""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    count = len(ranks)
    gl = [DevArray.from_host(np.ascontiguousarray(g)) for g in GL]
    g_r = [DevArray.from_host(np.ascontiguousarray(g)) for g in GR]
    pt, q, sg = [_Banded(r * r) for r in ranks], [_Banded(r * r) for r in ranks], [_Banded(r) for r in ranks]
    rk = _Banded((count + 1) // 2)                              # `count` int32 in whole doubles
    table = lambda xs: (ctypes.c_void_p * count)(*[x.ptr for x in xs])
    rc = nat.lib().ttsk_gram_round_bonds(table(gl), table(g_r), nat.i64_array(ranks), nat.i64_array(caps), count, float(eps),
                                         table(pt), table(q), table(sg), ctypes.c_void_p(rk.ptr), 0)
    nat.call("ttsk_sync", -1)
    rho = rk.read().view(np.int32)[:count]
    return (rc, [b.read().reshape(r, r) for b, r in zip(pt, ranks)], [b.read().reshape(r, r) for b, r in zip(q, ranks)],
            [b.read() for b in sg], rho)


@functools.lru_cache(maxsize=None)
def bond_inputs(name):
    """(cores, GL, GR, [(A, B)]) of a case: computed once"""
    case = next(c for c in gr.BOND_CASES if c.name == name)
    cores = gr.case_cores(case)
    GL, GR = gr.grams(cores)
    return cores, GL, GR, [gr.parts(cores, b + 1) for b in range(len(case.ranks))]


@pytest.mark.parametrize("case", gr.BOND_CASES, ids=lambda c: c.name)
def test_bond_kernel_against_the_dense_truths(tsa, case):
    cores, GL, GR, AB = bond_inputs(case.name)
    rc, Pt, Q, S, rho = c_bonds(GL, GR, case.ranks, case.caps, case.eps)
    assert rc == 0
    worst = [0.0, 0.0, 0.0]
    for b, r in enumerate(case.ranks):
        A, B = AB[b]
        k = int(rho[b])
        assert k == gr.expected_rank(A, B, case.eps, case.caps[b]), (b, k)
        assert not Pt[b][k:].any() and not Q[b][k:].any()                    # rows beyond the rank are zero
        assert (S[b] >= 0).all() and (np.diff(S[b]) <= 0).all()              # descending
        dev = gr.bond_deviation(A, B, Pt[b][:k].T, Q[b][:k], S[b], k)
        worst = [max(w, v) for w, v in zip(worst, dev)]
    print(case.name, "kernel", " ".join(f"{w:.2e}" for w in worst), "restatement", " ".join(f"{w:.2e}" for w in case.dev))
    for w, rec in zip(worst, case.dev):
        assert w <= gr.floor16(rec)


def test_bond_kernel_gives_the_same_bits_twice(tsa):
    case = gr.BOND_CASES[0]
    cores, GL, GR, AB = bond_inputs(case.name)
    one, two = c_bonds(GL, GR, case.ranks, case.caps, case.eps), c_bonds(GL, GR, case.ranks, case.caps, case.eps)
    for x, y in zip(one[1] + one[2] + one[3] + [one[4]], two[1] + two[2] + two[3] + [two[4]]):
        assert np.array_equal(x, y)


def test_bond_kernel_refuses_before_it_launches(tsa):
    from tt_sketch_amd import _native as nat
    G = np.eye(3)
    rc, Pt, Q, S, rho = c_bonds([G], [G], [1025], [3], 0.0)        # the rank argument is beyond the cover; nothing may be written
    assert rc == UNSUPPORTED and "1025" in nat.lib().ttsk_last_error().decode()
    assert (Pt[0] == SENTINEL).all() and (S[0] == SENTINEL).all()
    rc = c_bonds([G], [G], [3], [0], 0.0)[0]
    assert rc == -2


# ---------------------------------------------------------------- 2. round_gram against round
def _host_tt(tsa, tt):
    return tsa.TensorTrain([np.asarray(c.get() if hasattr(c, "get") else c) for c in tt.cores])


@functools.lru_cache(maxsize=None)
def round_truth(name):
    """(host cores, ranks of `round`, its relative error against the input): computed once"""
    import tt_sketch_amd as tsa
    case = next(c for c in gr.ROUND_CASES + [gr.EXACT_CASE] if c.name == name)
    cores = gr.random_tt(case.shape, case.ranks, case.seed)
    x = tsa.TensorTrain(cores)
    a = x.round(max_rank=case.max_rank)
    return cores, a.rank, a.error(x, relative=True)


@pytest.mark.parametrize("case", gr.ROUND_CASES + [gr.EXACT_CASE], ids=lambda c: c.name)
def test_round_gram_against_round(tsa, case):
    cores, want_rank, want_err = round_truth(case.name)
    x = tsa.TensorTrain(cores)
    g = x.to_device().round_gram(max_rank=case.max_rank)
    assert g.resident() and g.rank == want_rank and g.shape == x.shape
    err = _host_tt(tsa, g).error(x, relative=True)
    print(f"{case.name}: round {want_err:.6e} round_gram {err:.6e} ratio {err / max(want_err, 1e-300):.5f}")
    if want_err > 1e-8:
        assert err <= gr.ERROR_RATIO_CAP * want_err
    else:
        assert err <= 1e-12


# ---------------------------------------------------------------- 3. rank deficiency and the eps rule, 4. the floor
@functools.lru_cache(maxsize=None)
def pair():
    return gr.random_tt((10, 12, 11, 9), (6, 7, 5), 31), gr.random_tt((10, 12, 11, 9), (3, 4, 2), 32)


def test_rank_deficient_sums(tsa):
    xs, ys = pair()
    x, y = tsa.TensorTrain(xs).to_device(), tsa.TensorTrain(ys).to_device()
    xh = tsa.TensorTrain(xs)
    g = x.add(x).round_gram(eps=1e-6)
    assert g.rank == x.rank and _host_tt(tsa, g).error(xh * 2.0, relative=True) <= 1e-12
    g = x.add(y * 0.0).round_gram(eps=1e-6)                         # a zero summand: exact zero eigenvalues
    assert g.rank == x.rank and _host_tt(tsa, g).error(xh, relative=True) <= 1e-12
    s = tsa.TensorTrain(gr.add(xs, gr.scale(ys, 1e-5)))
    g = s.to_device().round_gram(eps=1e-3)
    small = 1e-5 * tsa.TensorTrain(ys).norm() / xh.norm()
    assert g.rank == x.rank and s.round(eps=1e-3).rank == x.rank
    assert _host_tt(tsa, g).error(s, relative=True) <= 2 * small    # of the size of the dropped term


def test_the_floor(tsa):
    """x + 1e-10 y at eps = 1e-12: `round` keeps every rank, ranks (9, 11, 7), at an error of 2e-15; a Gram method cannot
    resolve the small term.  The restatement returns the ranks of x, (6, 7, 5), at a relative error of 9.58e-11, the size
    of the term: the kernel's ranks lie between the two and its error stays below 10 times that."""
    xs, ys = pair()
    s_cores = gr.add(xs, gr.scale(ys, 1e-10))
    s = tsa.TensorTrain(s_cores)
    ref_err = tsa.TensorTrain(gr.round_gram(s_cores, 1e-12)[0]).error(s, relative=True)
    g = s.to_device().round_gram(eps=1e-12)
    err = _host_tt(tsa, g).error(s, relative=True)
    print(f"floor: ranks {g.rank} error {err:.3e} restatement {ref_err:.3e}")
    assert all(a <= r <= b for a, r, b in zip((6, 7, 5), g.rank, s.rank))
    assert err <= 10 * ref_err


# ---------------------------------------------------------------- 5. other properties
def test_residency_host_input_one_read_back_and_same_bits(tsa, monkeypatch):
    from tt_sketch_amd import _native as nat
    cores, want_rank, _ = round_truth("per_bond")
    x = tsa.TensorTrain(cores)
    assert not x.resident()
    reads, real = [], nat.call

    def call(name, *args):
        if name == "ttsk_d2h":
            reads.append(int(args[2]))
        return real(name, *args)
    monkeypatch.setattr(nat, "call", call)
    one = x.round_gram(max_rank=(7, 9, 5))                          # host cores: uploaded
    monkeypatch.undo()
    assert reads == [4 * (x.ndim - 1)]                             # one read-back: the d - 1 ranks
    assert one.resident() and one.rank == want_rank
    two = x.to_device().round_gram(max_rank=(7, 9, 5))
    for a, b in zip(one.cores, two.cores):
        assert np.array_equal(a.get(), b.get())
    single = tsa.TensorTrain([np.arange(5.0).reshape(1, 5, 1)]).round_gram()       # d = 1: nothing to round
    assert single.resident() and np.array_equal(single.cores[0].get().ravel(), np.arange(5.0))


def test_svdvals_gram_against_svdvals(tsa):
    """a train whose smallest singular value is above 1e-3 of the largest at every bond; the restatement's own deviation
    from `svdvals` on it is 8.2e-16 of the largest (measured on the CPU), times 16 and floored: 1e-13"""
    cores = gr.random_tt((8, 9, 10, 7), (3, 4, 3), 41)
    x = tsa.TensorTrain(cores)
    want = x.svdvals()[1:]
    got = x.to_device().svdvals_gram()
    assert len(got) == x.ndim - 1
    for b, (w, g) in enumerate(zip(want, got)):
        k = min(len(w), len(g))
        assert k == x.rank[b] and w[k - 1] > 1e-3 * w[0]
        assert np.max(np.abs(w[:k] - g[:k])) <= gr.floor16(8.2e-16) * w[0]


# ---------------------------------------------------------------- 6. round_tt_sum(method="gram") and TT-GMRES
def _gmres_problem(tsa):
    from tt_sketch_amd.tt_gmres import MPO, TTLinearMapSum
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gmres_case.npz"))
    shape = tuple(int(n) for n in z["shape"])
    d = len(shape)
    maps = [[z[f"map{m}_core{k}"] for k in range(d)] for m in range(3)]
    b = tsa.TensorTrain([z[f"b_core{k}"] for k in range(d)])
    return b, TTLinearMapSum([MPO(list(cores)) for cores in maps])


def test_round_tt_sum_gram_equals_exact(tsa):
    """the three operator terms of the GMRES case at a rank that represents their sum: both methods return the sum itself"""
    from tt_sketch_amd.tt_gmres import round_tt_sum
    b, A = _gmres_problem(tsa)
    terms = A(b.to_device())
    exact = round_tt_sum(terms, 30, method="exact")
    gram = round_tt_sum(terms, 30, method="gram")
    assert gram.resident() and gram.rank == exact.rank
    assert gr.rel_error(gram.to_numpy(), exact.to_numpy()) < 1e-12
    assert gr.rel_error(gram.to_numpy(), terms.to_numpy()) < 1e-12
    h = tsa.hadamard_round(b, b, 30, method="gram")
    assert gr.rel_error(h.to_numpy(), b.to_numpy() ** 2) < 1e-12


def test_gmres_with_gram_rounding_reaches_the_residual_of_exact(tsa):
    """at a rank that represents every iterate (the setting of the sketched-rounding tests, and their tolerance on the
    residual history)"""
    from tt_sketch_amd.tt_gmres import tt_sum_gmres
    b, A = _gmres_problem(tsa)
    _, exact = tt_sum_gmres(A, b, max_rank=30, tolerance=1e-9, maxiter=3, rounding_method="exact")
    x, gram = tt_sum_gmres(A, b, max_rank=30, tolerance=1e-9, maxiter=3, rounding_method="gram")
    print("exact", exact["residual_norm"], "gram", gram["residual_norm"])
    assert x.resident() and len(gram["residual_norm"]) == len(exact["residual_norm"])
    assert np.allclose(gram["residual_norm"], exact["residual_norm"], rtol=1e-4)
