"""ttsk_tt_orth_sketch: orthogonal_sketch / hmt_sketch of a TT with TT DRMs as one library call.

What the one-call path does differently from the mode-by-mode path (sketch_dispatch.py:160-193 as the reference
writes it): it never forms Psi_mu (Q_mu = qr(T R_mu Omega_mu^+)), it carries the chain on with the UNSIGNED
CholeskyQR factor and reconstructs LAPACK's Householder column signs beside the critical path, and it applies
the signs to the cores at the end.  So the cores are compared entry by entry (signs included) against the
oracle's numpy QR, against the mode-by-mode device path, and the fallbacks are exercised.
"""
import ctypes

import numpy as np
import pytest

from oracle import ttsk_oracle as orc

from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

import os

ONE_CALL = os.environ.get("TTSK_ORTH_ONE_CALL", "1") != "0"      # (the diagnostic switch sends everything mode by mode)
CORE_TOL = 1e-9            # entrywise, relative to the largest entry of the core (cores went through pinv and QR)


def _case(shape, s_in, l, r, seed):
    rng = np.random.default_rng(seed)
    cores = orc.random_tt(shape, s_in, rng)
    ld = orc.random_tt_drm(shape, l, False, rng) if l is not None else None
    rd = orc.random_tt_drm(shape, r, True, rng)
    return cores, ld, rd


def _dev_drms(tsa, shape, l, r, ld, rd):
    right = tsa.TensorTrainDRM(r, shape, True, seed=2, cores=[np.array(c) for c in rd.cores])
    left = None if ld is None else tsa.TensorTrainDRM(l, shape, False, seed=1, cores=[np.array(c) for c in ld.cores])
    return left, right


def _one_call_ran(tsa, monkeypatch):
    """count the calls that went through the one-call entry point"""
    from tt_sketch_amd import tt_fused
    hits = []
    real = tt_fused.try_orth_sketch

    def spy(*a, **k):
        out = real(*a, **k)
        hits.append(out is not None)
        return out
    monkeypatch.setattr(tt_fused, "try_orth_sketch", spy)
    return hits


def _close(got, want):
    assert [np.asarray(c).shape for c in got] == [np.asarray(c).shape for c in want]
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert np.abs(g - w).max() <= CORE_TOL * np.abs(w).max(), f"core {k}"


@pytest.mark.parametrize("shape,s_in,l,r", [
    ((30, 28, 26, 24, 22), 12, 8, 16),           # d = 5, every mode size different
    ((40, 40, 40, 40), 20, 16, 17),              # r = l + 1 (nearly square Omega)
    ((64, 50, 50, 64), 33, 17, 40),              # odd ranks, r > 2 l
    ((200, 200, 200), 60, 50, 64),               # four column tiles wide
    ((12, 100, 100, 12), 10, 6, 9),              # first unfolding only twice as tall as wide
])
def test_orthogonal_one_call_cores_match_oracle_and_mode_by_mode(tsa, monkeypatch, shape, s_in, l, r):
    from tt_sketch_amd import sketch_dispatch
    d = len(shape)
    cores, ld, rd = _case(shape, s_in, l, r, seed=sum(shape) + l)
    left, right = _dev_drms(tsa, shape, (l,) * (d - 1), (r,) * (d - 1), ld, rd)
    hits = _one_call_ran(tsa, monkeypatch)
    X = tsa.TensorTrain(cores)
    one = [np.asarray(c) for c in tsa.orthogonal_sketch(X, (l,) * (d - 1), (r,) * (d - 1), left_drm=left, right_drm=right).cores]
    assert hits == ([True] if ONE_CALL else [])
    monkeypatch.setattr(sketch_dispatch, "_ONE_CALL_ORTH", False)
    per_mode = [np.asarray(c) for c in tsa.orthogonal_sketch(X, (l,) * (d - 1), (r,) * (d - 1), left_drm=left, right_drm=right).cores]
    want, _ = orc.general_sketch("tt", cores, ld, rd, "orthogonal")
    _close(one, want)
    _close(one, per_mode)
    for c in one[:-1]:
        q = c.reshape(-1, c.shape[2])
        assert np.linalg.norm(q.T @ q - np.eye(q.shape[1])) < 1e-12


@pytest.mark.parametrize("shape,s_in,r", [
    ((30, 28, 26, 24, 22), 12, 10),
    ((100, 100, 100, 100), 40, 32),
    ((200, 200, 200), 70, 64),
])
def test_hmt_one_call_cores_match_oracle(tsa, monkeypatch, shape, s_in, r):
    d = len(shape)
    cores, _, rd = _case(shape, s_in, None, r, seed=sum(shape) + r)
    _, right = _dev_drms(tsa, shape, None, (r,) * (d - 1), None, rd)
    hits = _one_call_ran(tsa, monkeypatch)
    got = [np.asarray(c) for c in tsa.hmt_sketch(tsa.TensorTrain(cores), (r,) * (d - 1), drm=right).cores]
    assert hits == ([True] if ONE_CALL else [])
    want, _ = orc.general_sketch("tt", cores, None, rd, "hmt")
    _close(got, want)


def test_one_call_with_a_different_rank_in_every_mode(tsa, monkeypatch):
    """Omega of different shapes per mode: pseudo-inverses one by one instead of batched, same cores as the oracle."""
    shape, s_in = (24, 24, 24, 24), 10
    l, r = (4, 6, 5), (8, 12, 10)
    rng = np.random.default_rng(5)
    cores = orc.random_tt(shape, s_in, rng)
    ld, rd = orc.random_tt_drm(shape, l, False, rng), orc.random_tt_drm(shape, r, True, rng)
    left = tsa.TensorTrainDRM(l, shape, False, seed=1, cores=[np.array(c) for c in ld.cores])
    right = tsa.TensorTrainDRM(r, shape, True, seed=2, cores=[np.array(c) for c in rd.cores])
    hits = _one_call_ran(tsa, monkeypatch)
    got = [np.asarray(c) for c in tsa.orthogonal_sketch(tsa.TensorTrain(cores), l, r, left_drm=left, right_drm=right).cores]
    assert hits == ([True] if ONE_CALL else [])
    want, _ = orc.general_sketch("tt", cores, ld, rd, "orthogonal")
    _close(got, want)


def test_hmt_one_call_nearly_square_interior_unfolding(tsa, monkeypatch):
    """An interior unfolding less than twice as tall as wide (3 x 3 rows, rank 8): each QR signs its own Q instead of the
    sign reconstruction beside the chain (tt_orth.hip `beside`), same cores as the oracle."""
    shape, r = (3, 3, 3, 3), (3, 8, 3)
    rng = np.random.default_rng(13)
    cores = orc.random_tt(shape, r, rng)                  # TT ranks = sketch ranks: every unfolding of full rank
    rd = orc.random_tt_drm(shape, r, True, rng)
    right = tsa.TensorTrainDRM(r, shape, True, seed=2, cores=[np.array(c) for c in rd.cores])
    hits = _one_call_ran(tsa, monkeypatch)
    got = [np.asarray(c) for c in tsa.hmt_sketch(tsa.TensorTrain(cores), r, drm=right).cores]
    assert hits == ([True] if ONE_CALL else [])
    want, _ = orc.general_sketch("tt", cores, None, rd, "hmt")
    _close(got, want)


@pytest.mark.parametrize("l,r", [(140, 150), (100, 200)])
def test_one_call_ranks_beyond_128(tsa, monkeypatch, l, r):
    """two-block Cholesky factors, sign reconstruction with its working copy in global memory (129 .. 256 columns)"""
    shape, s_in = (160, 160, 160), 150
    cores, ld, rd = _case(shape, s_in, l, r, seed=l + r)
    left, right = _dev_drms(tsa, shape, (l,) * 2, (r,) * 2, ld, rd)
    hits = _one_call_ran(tsa, monkeypatch)
    got = [np.asarray(c) for c in tsa.orthogonal_sketch(tsa.TensorTrain(cores), (l,) * 2, (r,) * 2, left_drm=left, right_drm=right).cores]
    assert hits == ([True] if ONE_CALL else [])
    want, _ = orc.general_sketch("tt", cores, ld, rd, "orthogonal")
    _close(got, want)
    if r <= shape[0]:                         # (the first unfolding of hmt_sketch is n_0 x r)
        got = [np.asarray(c) for c in tsa.hmt_sketch(tsa.TensorTrain(cores), (r,) * 2, drm=right).cores]
        want, _ = orc.general_sketch("tt", cores, None, rd, "hmt")
        _close(got, want)


def test_one_call_declines_what_it_does_not_cover(tsa, monkeypatch):
    """a right DRM that is not a tensor train: the mode-by-mode path, same tensor as the oracle's"""
    shape, s_in, l, r = (16, 16, 16, 16), 3, 4, 9            # TT-rank 3 <= l: the sketch recovers the input
    rng = np.random.default_rng(9)
    cores = orc.random_tt(shape, s_in, rng)
    hits = _one_call_ran(tsa, monkeypatch)
    X = tsa.TensorTrain(cores)
    out = tsa.orthogonal_sketch(X, l, r, seed=2, right_drm_type=tsa.DenseGaussianDRM)
    assert hits == ([False] if ONE_CALL else [])
    assert out.error(X) < 1e-10
def test_one_call_rejection_repeats_on_the_robust_path(tsa, monkeypatch):
    """An input of TT-rank 3 sketched with l = 8: Omega has rank 3, the normal equations are rejected on the device,
    the deferred flag is read once and the sketch is repeated with the Jacobi pseudo-inverse -- the recovered tensor
    is the input (sketch_dispatch.py:160-174 with numpy's pinv / qr in the reference)."""
    shape, l, r = (20, 20, 20, 20), 8, 14
    rng = np.random.default_rng(11)
    cores = orc.random_tt(shape, 3, rng)
    hits = _one_call_ran(tsa, monkeypatch)
    X = tsa.TensorTrain(cores)
    out = tsa.orthogonal_sketch(X, l, r, seed=4)
    assert hits == ([True] if ONE_CALL else [])    # it ran, and its result was thrown away
    assert out.error(X) < 1e-10


def test_pinv_batch_mixes_accepted_and_rejected_matrices(tsa):
    """ttsk_pinv_batch: five 12 x 30 matrices in one set of launches, two of them rank deficient (the Jacobi kernel takes
    over for exactly those, through its predicate) -- numpy.linalg.pinv's result for each (utils.py:98-109)."""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray, as_dev
    rng = np.random.default_rng(3)
    l, r = 12, 30
    mats = [rng.standard_normal((l, r)) for _ in range(5)]
    mats[1] = rng.standard_normal((l, 4)) @ rng.standard_normal((4, r))          # rank 4
    mats[3][5] = mats[3][2] * 0.5 - mats[3][7]                                     # rank 11
    P = ctypes.c_void_p
    for transposed in (False, True):
        hs = [m.T.copy() if transposed else m for m in mats]
        ds = [as_dev(h) for h in hs]
        outs = [DevArray.empty(h.T.shape) for h in hs]
        nat.call("ttsk_pinv_batch", 5, (P * 5)(*[x.ptr for x in ds]), hs[0].shape[0], hs[0].shape[1], (P * 5)(*[o.ptr for o in outs]), 0)
        for k, (h, o) in enumerate(zip(hs, outs)):
            want = np.linalg.pinv(h, rcond=16 * np.finfo(float).eps * np.sqrt(max(h.shape)))
            assert np.abs(o.get() - want).max() <= 1e-11 * np.abs(want).max(), (transposed, k)


@pytest.mark.parametrize("direction", ["right", "left"])
@pytest.mark.parametrize("ranks", [((6, 6, 6), (9, 9, 9)), ((4, 7, 5), (8, 11, 6))])
def test_assemble_one_call_matches_the_pair_by_pair_path(tsa, monkeypatch, direction, ranks):
    """ttsk_tt_assemble (batched pseudo-inverses when the Omega share a shape, pair by pair otherwise) against
    assemble_sketched_tt's own loop and against numpy (sketch.py:400-443)."""
    from tt_sketch_amd.sketch import assemble_sketched_tt
    shape = (14, 15, 16, 17)
    lr, rr = ranks
    if direction == "left":
        lr, rr = rr, lr
    rng = np.random.default_rng(21)
    X = tsa.TensorTrain(orc.random_tt(shape, 3, rng))
    stt = tsa.stream_sketch(X, lr, rr, seed=5)
    one = [np.asarray(c) for c in assemble_sketched_tt(stt.sketch_ if hasattr(stt, "sketch_") else stt.sketch, direction=direction)]
    monkeypatch.setenv("TTSK_ASSEMBLE_ONE_CALL", "0")
    pairs = [np.asarray(c) for c in assemble_sketched_tt(stt.sketch_ if hasattr(stt, "sketch_") else stt.sketch, direction=direction)]
    for a, b in zip(one, pairs):
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-10 * max(1.0, np.abs(b).max())
    rec = tsa.TensorTrain(one)
    assert rec.error(X) < 1e-9


@pytest.mark.parametrize("direction", ["right", "left"])
def test_assemble_one_call_d12_mixed_mode_sizes(tsa, monkeypatch, direction):
    """d = 12 with uniform ranks and two mode sizes: the interior pairs whose mode equals n[1] are grouped into batched
    launches, the others (among them pairs k >= 9, which share a helper stream with a grouped pair k - 8) run on helper
    streams that must be forked behind the batched pseudo-inverses whichever pair reaches them first."""
    from tt_sketch_amd.sketch import assemble_sketched_tt
    shape = (9, 12, 12, 12, 12, 12, 12, 12, 12, 10, 11, 13)
    d = len(shape)
    lr, rr = (5,) * (d - 1), (8,) * (d - 1)
    if direction == "left":
        lr, rr = rr, lr
    rng = np.random.default_rng(33)
    X = tsa.TensorTrain(orc.random_tt(shape, 3, rng))
    for rep in range(3):                                  # a race does not show every time
        stt = tsa.stream_sketch(X, lr, rr, seed=7 + rep)
        monkeypatch.setenv("TTSK_ASSEMBLE_ONE_CALL", "1")
        one = [np.asarray(c) for c in assemble_sketched_tt(stt.sketch_ if hasattr(stt, "sketch_") else stt.sketch, direction=direction)]
        monkeypatch.setenv("TTSK_ASSEMBLE_ONE_CALL", "0")
        pairs = [np.asarray(c) for c in assemble_sketched_tt(stt.sketch_ if hasattr(stt, "sketch_") else stt.sketch, direction=direction)]
        for a, b in zip(one, pairs):
            assert a.shape == b.shape and np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(b).max())
        assert tsa.TensorTrain(one).error(X) < 1e-8


@pytest.mark.parametrize("entry", ["ttsk_pinv_batch", "ttsk_pinv_batch_deferred"])
@pytest.mark.parametrize("l,r", [(10, 600), (600, 10)])
def test_pinv_batch_declines_a_stage_beyond_the_small_kernel_before_queuing(tsa, entry, l, r):
    """(10, 600): the Gram product (10 x 10) fits the batched small kernel, the solve (600 x 10) does not.  The batched
    entries check every stage before the first launch: TtskUnsupported, the outputs untouched."""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import as_dev
    rng = np.random.default_rng(8)
    ds = [as_dev(rng.standard_normal((l, r))) for _ in range(3)]
    outs = [as_dev(np.full((r, l), 7.0)) for _ in ds]
    P = ctypes.c_void_p
    with pytest.raises(nat.TtskUnsupported):
        nat.call(entry, 3, (P * 3)(*[x.ptr for x in ds]), l, r, (P * 3)(*[o.ptr for o in outs]), 0)
    for o in outs:
        assert (o.get() == 7.0).all()


@pytest.mark.parametrize("direction", ["right", "left"])
@pytest.mark.parametrize("l,r", [(10, 600), (600, 10)])
def test_assemble_one_call_with_omega_beyond_the_batched_pseudo_inverse(tsa, monkeypatch, direction, l, r):
    """Omega of one shape whose solve the batched small kernel declines: ttsk_tt_assemble's batched pseudo-inverses decline
    before queuing anything and the pairs take the path of their own -- the cores of the pair-by-pair path (sketch.py:400-443)."""
    from tt_sketch_amd import sketch
    from tt_sketch_amd.sketch import assemble_sketched_tt
    from tt_sketch_amd.sketch_container import SketchContainer
    rng = np.random.default_rng(29)
    n, d = (7, 8, 9), 3
    Om = [rng.standard_normal((l, r)) for _ in range(d - 1)]
    Psi = [rng.standard_normal((1 if mu == 0 else l, n[mu], 1 if mu == d - 1 else r)) for mu in range(d)]
    sk = SketchContainer([np.array(p) for p in Psi], [np.array(o) for o in Om])
    hits = []
    real = sketch._assemble_one_call

    def spy(*a, **k):
        out = real(*a, **k)
        hits.append(out is not None)
        return out
    monkeypatch.setattr(sketch, "_assemble_one_call", spy)
    one = [np.asarray(c) for c in assemble_sketched_tt(sk, direction=direction)]
    assert hits == [True]
    monkeypatch.setenv("TTSK_ASSEMBLE_ONE_CALL", "0")
    pairs = [np.asarray(c) for c in assemble_sketched_tt(sk, direction=direction)]
    for a, b in zip(one, pairs):
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-10 * max(1.0, np.abs(b).max())


@pytest.mark.parametrize("direction", ["right", "left"])
def test_assembly_matches_lstsq_for_ill_conditioned_omega(tsa, monkeypatch, direction):
    """Omega with singular values from 1 down to 1e-4 (what the sketches of TT-GMRES iterates look like): the assembled
    tensor agrees with scipy.linalg.lstsq -- the reference's solve, utils.py:98-109 -- to 1e-11 on BOTH assembly paths.
    A product with an explicitly formed pseudo-inverse alone is off by about 1e-10 here (kappa * eps on every component,
    where lstsq loses it only along the small singular directions) (the refinement step of
    ttsk_tt_assemble / utils.refine_right)."""
    import scipy.linalg
    from test_gpu_c3_solves import tt_rel_diff
    from tt_sketch_amd.sketch import assemble_sketched_tt
    from tt_sketch_amd.sketch_container import SketchContainer
    rng = np.random.default_rng(17)
    n, l, r, d = (40, 50, 60, 30), 12, 20, 4
    if direction == "left":
        l, r = r, l
    k = min(l, r)
    Om, Psi = [], []
    for mu in range(d - 1):
        U, _ = np.linalg.qr(rng.standard_normal((l, k)))
        V, _ = np.linalg.qr(rng.standard_normal((r, k)))
        Om.append((U * np.logspace(0, -4, k)) @ V.T)
    for mu in range(d):
        r1, r2 = (1 if mu == 0 else l), (1 if mu == d - 1 else r)
        P = rng.standard_normal((r1, n[mu], r2))
        # consistent with its Omega (rows / columns in Omega's row / column space), as the Psi of a sketch are
        if direction == "right" and mu < d - 1:
            P = np.einsum("ajl,lr->ajr", rng.standard_normal((r1, n[mu], l)), Om[mu])
        if direction == "left" and mu > 0:
            P = np.einsum("lr,rjb->ljb", Om[mu - 1], rng.standard_normal((r, n[mu], r2)))
        Psi.append(P)
    want = []
    if direction == "right":
        for P, O in zip(Psi[:-1], Om):
            r1, nn, r2 = P.shape
            want.append(scipy.linalg.lstsq(O.T, P.reshape(r1 * nn, r2).T, cond=None)[0].T.reshape(r1, nn, -1))
        want.append(Psi[-1])
    else:
        want.append(Psi[0])
        for P, O in zip(Psi[1:], Om):
            r1, nn, r2 = P.shape
            want.append(scipy.linalg.lstsq(O, P.reshape(r1, nn * r2), cond=None)[0].reshape(-1, nn, r2))
    sk = SketchContainer([np.array(p) for p in Psi], [np.array(o) for o in Om])
    one = [np.asarray(c) for c in assemble_sketched_tt(sk, direction=direction)]
    e_one = tt_rel_diff(one, want)
    monkeypatch.setenv("TTSK_ASSEMBLE_ONE_CALL", "0")
    pairs = [np.asarray(c) for c in assemble_sketched_tt(sk, direction=direction)]
    e_pairs = tt_rel_diff(pairs, want)
    print("assembly vs lstsq:", e_one, e_pairs)
    assert e_one < 1e-11 and e_pairs < 1e-11


# ---------------------------------------------------------------------------------------------------------------------------
# orthogonal_sketch_batch / hmt_sketch_batch (ttsk_tt_orth_sketch_batch): same-signature TTs as concurrent chains
@pytest.mark.parametrize("shape,s_in,l,r,count", [
    ((30, 28, 26, 24, 22), 12, 8, 16, 9),        # more tensors than stream pairs: a second tensor queues behind the first on a pair
    ((64, 50, 50, 64), 33, 17, 40, 4),
    ((200, 200, 200), 60, 50, 64, 3),
    ((12, 20, 20, 12), 10, 8, 10, 5),            # n_0 = 12 < 2 l: outside the fused batch's cover, the tensors as concurrent chains
])
def test_orthogonal_sketch_batch_every_tensor_vs_oracle(tsa, shape, s_in, l, r, count):
    """every tensor of the batch entry by entry against the oracle (sketch_dispatch.py:160-193), and
    against the single calls (the batched launches sum in another order: to rounding, not bit for bit)."""
    d = len(shape)
    rng = np.random.default_rng(sum(shape) + count)
    ld, rd = orc.random_tt_drm(shape, l, False, rng), orc.random_tt_drm(shape, r, True, rng)
    left, right = _dev_drms(tsa, shape, (l,) * (d - 1), (r,) * (d - 1), ld, rd)
    all_cores = [orc.random_tt(shape, s_in, rng) for _ in range(count)]
    tts = [tsa.TensorTrain(c) for c in all_cores]
    from tt_sketch_amd import tt_fused
    assert tt_fused.try_orth_sketch_batch(tts, left, right, tsa.SketchMethod.orthogonal) is not None
    got = tsa.orthogonal_sketch_batch(tts, (l,) * (d - 1), (r,) * (d - 1), left_drm=left, right_drm=right)
    assert len(got) == count
    for cores, tt in zip(all_cores, got):
        want, _ = orc.general_sketch("tt", cores, ld, rd, "orthogonal")
        _close([np.asarray(c) for c in tt.cores], want)
    for k in (0, count - 1):
        one = tsa.orthogonal_sketch(tts[k], (l,) * (d - 1), (r,) * (d - 1), left_drm=left, right_drm=right)
        _close([np.asarray(c) for c in got[k].cores], [np.asarray(c) for c in one.cores])


def test_hmt_sketch_batch_every_tensor_vs_oracle(tsa):
    shape, s_in, r, count = (100, 100, 100, 100), 40, 32, 6
    d = len(shape)
    rng = np.random.default_rng(8)
    rd = orc.random_tt_drm(shape, r, True, rng)
    _, right = _dev_drms(tsa, shape, None, (r,) * (d - 1), None, rd)
    all_cores = [orc.random_tt(shape, s_in, rng) for _ in range(count)]
    got, drm = tsa.hmt_sketch_batch([tsa.TensorTrain(c) for c in all_cores], (r,) * (d - 1), drm=right, return_drm=True)
    assert drm is right and len(got) == count
    for cores, tt in zip(all_cores, got):
        want, _ = orc.general_sketch("tt", cores, None, rd, "hmt")
        _close([np.asarray(c) for c in tt.cores], want)


def test_orthogonal_sketch_batch_verdict_per_tensor_and_fallbacks(tsa, monkeypatch):
    """A rank-deficient tensor inside a batch (TT-rank 5 < l: its Omega have rank 5, the Cholesky attempts are rejected):
    the verdict comes back and the affected tensors are repeated one by one on the robust path (the fused batch has ONE
    flag for all its tensors, the concurrent-chains form one per tensor) -- every result is right either way; a list that
    is not of one signature, and a dense tensor, go through orthogonal_sketch one by one; the argument policy is
    orthogonal_sketch's."""
    from tt_sketch_amd import sketch_dispatch
    shape, l, r = (20, 22, 24, 26), 8, 14
    d = len(shape)
    rng = np.random.default_rng(11)
    ld, rd = orc.random_tt_drm(shape, l, False, rng), orc.random_tt_drm(shape, r, True, rng)
    left, right = _dev_drms(tsa, shape, (l,) * (d - 1), (r,) * (d - 1), ld, rd)
    good = [orc.random_tt(shape, 10, rng) for _ in range(5)]
    low = orc.random_tt(shape, 5, rng)
    low = [np.concatenate([c, np.zeros((c.shape[0], c.shape[1], 10 - c.shape[2]))], axis=2) if k < d - 1 else c for k, c in enumerate(low)]
    low = [np.concatenate([c, np.zeros((10 - c.shape[0], c.shape[1], c.shape[2]))], axis=0) if k > 0 else c for k, c in enumerate(low)]
    cores = good[:2] + [low] + good[2:]                                  # same signature (TT-rank 10), numerical rank 5
    before = dict(sketch_dispatch.robust_reruns)
    got = tsa.orthogonal_sketch_batch([tsa.TensorTrain(c) for c in cores], (l,) * (d - 1), (r,) * (d - 1), left_drm=left, right_drm=right)
    reruns = sketch_dispatch.robust_reruns.get("orthogonal", 0) - before.get("orthogonal", 0)
    assert reruns >= 1                                                   # (the batch's verdict, then orthogonal_sketch's own optimistic pass)
    for k, (c, tt) in enumerate(zip(cores, got)):
        if k == 2:
            assert tt.error(tsa.TensorTrain(c), relative=True) < 1e-9      # exact recovery of the rank-5 tensor
        else:
            want, _ = orc.general_sketch("tt", c, ld, rd, "orthogonal")
            _close([np.asarray(x) for x in tt.cores], want)
    # mixed signatures / a dense tensor: one by one
    other = orc.random_tt(shape, 7, rng)
    mixed = [tsa.TensorTrain(good[0]), tsa.TensorTrain(other), tsa.DenseTensor(tsa.TensorTrain(good[1]).to_numpy())]
    res = tsa.orthogonal_sketch_batch(mixed, (l,) * (d - 1), (r,) * (d - 1), left_drm=left, right_drm=right)
    want, _ = orc.general_sketch("tt", good[0], ld, rd, "orthogonal")
    _close([np.asarray(x) for x in res[0].cores], want)
    assert len(res) == 3 and res[2].shape == shape
    with pytest.raises(ValueError):
        tsa.orthogonal_sketch_batch(mixed[:2], (l,) * (d - 1), (l,) * (d - 1))
    assert tsa.orthogonal_sketch_batch([], l, r) == [] and tsa.hmt_sketch_batch([], r) == []
    # default DRMs: one pair for the whole batch, returned
    res, L, R = tsa.orthogonal_sketch_batch(mixed[:1] * 3, l, r, seed=5, return_drm=True)
    assert type(L).__name__ == "TensorTrainDRM" and len(res) == 3
    _close([np.asarray(a) for a in res[0].cores], [np.asarray(b) for b in res[2].cores])


def test_batch_entries_beyond_one_slice_and_of_one_tensor(tsa):
    """20 tensors = two slices of the batch entry (16 + 4); a list of one tensor goes through the single call; default DRMs of
    hmt_sketch_batch are one DRM for all."""
    shape, s_in, l, r = (24, 20, 22, 18), 9, 6, 11
    d = len(shape)
    rng = np.random.default_rng(21)
    ld, rd = orc.random_tt_drm(shape, l, False, rng), orc.random_tt_drm(shape, r, True, rng)
    left, right = _dev_drms(tsa, shape, (l,) * (d - 1), (r,) * (d - 1), ld, rd)
    all_cores = [orc.random_tt(shape, s_in, rng) for _ in range(20)]
    tts = [tsa.TensorTrain(c) for c in all_cores]
    got = tsa.orthogonal_sketch_batch(tts, (l,) * (d - 1), (r,) * (d - 1), left_drm=left, right_drm=right)
    assert len(got) == 20
    for k in (0, 15, 16, 19):
        want, _ = orc.general_sketch("tt", all_cores[k], ld, rd, "orthogonal")
        _close([np.asarray(c) for c in got[k].cores], want)
    one = tsa.orthogonal_sketch_batch(tts[:1], (l,) * (d - 1), (r,) * (d - 1), left_drm=left, right_drm=right)
    want, _ = orc.general_sketch("tt", all_cores[0], ld, rd, "orthogonal")
    _close([np.asarray(c) for c in one[0].cores], want)
    res, drm = tsa.hmt_sketch_batch(tts[:3], r, seed=4, return_drm=True)
    assert type(drm).__name__ == "TensorTrainDRM" and drm.transpose and len(res) == 3
    for t, g in zip(tts[:3], res):
        assert g.error(t, relative=True) < 1e-9            # sketch rank 11 covers the TT rank 9: exact recovery
