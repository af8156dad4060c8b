"""KhatriRaoDRM on the host: the rank bookkeeping (rank, T, slice, increase_rank), the embedding ``as_train`` and the
reference tests/khatri_rao_ref.py against the oracle.  The matrices are injected from NumPy (``mats=``), so nothing here
touches a device."""
import numpy as np
import pytest

from oracle import ttsk_oracle as orc
from tests import khatri_rao_ref as ref

SHAPE = (6, 5, 4, 7)


def _mats(shape, transpose, R, seed):
    walk = shape[::-1] if transpose else shape
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((R, n)) for n in walk[:-1]]


def _drm(rank, transpose, seed=3, shape=SHAPE, R=None, **kw):
    from tt_sketch_amd import KhatriRaoDRM
    rk = (rank,) * (len(shape) - 1) if isinstance(rank, int) else tuple(rank)
    top = max(kw.get("true_rank", rk))
    return KhatriRaoDRM(rank, shape, transpose, seed=seed, mats=_mats(shape, transpose, R or top, seed), **kw)


def test_exported_and_capable():
    import tt_sketch_amd as tsa
    from tt_sketch_amd.drm import KhatriRaoDRM
    from tt_sketch_amd.drm_base import CanIncreaseRank, CanSlice
    from tt_sketch_amd.sketching_methods import abstract_methods as am
    assert tsa.KhatriRaoDRM is KhatriRaoDRM
    for cap in (CanSlice, CanIncreaseRank, am.CansketchTT, am.CansketchCP, am.CansketchSparse, am.CansketchDense, am.CanSketchTucker):
        assert issubclass(KhatriRaoDRM, cap), cap


@pytest.mark.parametrize("transpose", [False, True])
def test_rank_and_T(transpose):
    rank = (4, 5, 6)
    drm = _drm(rank, transpose)
    stored = rank[::-1] if transpose else rank
    assert drm.rank == stored and drm.true_rank == stored and drm.rank_min == (0, 0, 0) and drm.rank_max == stored
    assert [m.shape for m in drm.mats] == [(6, n) for n in (SHAPE[::-1] if transpose else SHAPE)[:-1]]
    other = drm.T
    assert other.transpose is (not transpose) and other.rank == stored[::-1] and other.mats is drm.mats
    S = ref.of_drm(drm)
    walk = SHAPE[::-1] if transpose else SHAPE
    assert [s.shape for s in S] == [(stored[mu],) + tuple(walk[:mu + 1]) for mu in range(3)]
    # by the definition, entry by entry
    m, idx = 2, (1, 3, 2)
    assert S[2][(m,) + idx] == drm.mats[0][m, 1] * drm.mats[1][m, 3] * drm.mats[2][m, 2]


def test_wrong_matrices_are_refused():
    from tt_sketch_amd import KhatriRaoDRM
    good = _mats(SHAPE, False, 5, 0)
    with pytest.raises(ValueError):
        KhatriRaoDRM(5, SHAPE, False, seed=0, mats=good[:2])
    with pytest.raises(ValueError):
        KhatriRaoDRM(6, SHAPE, False, seed=0, mats=good)                    # too few rows
    with pytest.raises(ValueError):
        KhatriRaoDRM(5, SHAPE, True, seed=0, mats=good)                     # the walk of the other side


@pytest.mark.parametrize("transpose", [False, True])
def test_slice_keeps_the_columns(transpose):
    drm = _drm((6, 7, 8), transpose)
    lo, hi = (1, 2, 3), (4, 7, 5)
    cut = drm.slice(lo, hi)
    assert cut.mats is drm.mats and cut.true_rank == drm.true_rank
    slo, shi = (lo[::-1], hi[::-1]) if transpose else (lo, hi)
    assert cut.rank_min == slo and cut.rank_max == shi and cut.rank == tuple(b - a for a, b in zip(slo, shi))
    for mu, (whole, part) in enumerate(zip(ref.of_drm(drm), ref.of_drm(cut))):
        assert np.array_equal(part, whole[slo[mu]:shi[mu]])
    lead = drm.slice(None, (2, 2, 2))
    for whole, part in zip(ref.of_drm(drm), ref.of_drm(lead)):
        assert np.array_equal(part, whole[:2])


@pytest.mark.parametrize("transpose", [False, True])
def test_increase_rank_keeps_the_leading_columns(transpose):
    big = _mats(SHAPE, transpose, 9, 3)
    from tt_sketch_amd import KhatriRaoDRM
    small = KhatriRaoDRM((4, 5, 6), SHAPE, transpose, seed=3, mats=[m[:6] for m in big])
    with pytest.raises(ValueError):
        small.increase_rank((6, 7, 9))                   # injected matrices cannot be sampled further
    grown = small.increase_rank((6, 7, 9), mats=big)
    assert type(grown) is KhatriRaoDRM and grown.transpose == transpose and grown.seed == small.seed
    assert grown.rank == ((9, 7, 6) if transpose else (6, 7, 9))
    for a, b in zip(ref.of_drm(small), ref.of_drm(grown)):
        assert np.array_equal(a, b[:a.shape[0]])
    back = grown.slice(None, (4, 5, 6))
    for a, b in zip(ref.of_drm(small), ref.of_drm(back)):
        assert np.array_equal(a, b)


def _train_matrices(train):
    """the sketching matrices of a TensorTrainDRM from its cores, cut as it cuts them: (w_mu, n_0, ..., n_mu)"""
    out, P = [], None
    for mu, D in enumerate(train.cores):
        D = np.asarray(D)
        P = D[0] if P is None else np.einsum("...a,akb->...kb", P, D)
        cut = P[..., train.rank_min[mu]:train.rank_max[mu]]
        out.append(np.moveaxis(cut, -1, 0))
    return out


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("sliced", [False, True])
def test_as_train_hands_out_the_same_columns(transpose, sliced):
    from tt_sketch_amd import TensorTrainDRM
    drm = _drm((6, 7, 8), transpose)
    if sliced:
        drm = drm.slice((1, 2, 3), (4, 7, 5))
    train = drm.as_train()
    assert type(train) is TensorTrainDRM and train.transpose == transpose and train.shape == drm.shape
    assert train.rank == drm.rank
    R = max(drm.rank_max) - min(drm.rank_min)
    walk = SHAPE[::-1] if transpose else SHAPE
    assert [tuple(c.shape) for c in train.cores] == [(1 if s == 0 else R, walk[s], R) for s in range(3)]
    for s, c in enumerate(train.cores[1:], start=1):     # diagonal in the two rank indices
        off = c.copy()
        off[np.arange(R), :, np.arange(R)] = 0.0
        assert not off.any()
    for a, b in zip(ref.of_drm(drm), _train_matrices(train)):
        assert a.shape == b.shape and np.allclose(a, b, rtol=1e-15, atol=0)


@pytest.mark.parametrize("kind", ["tt", "cp"])
def test_reference_agrees_with_the_oracle_on_the_embedding(kind):
    """tests/khatri_rao_ref.py (explicit S_mu, sketches by definition) against the oracle's streaming sketch with the
    cores of ``as_train``: the products of four factors and sums of 840 terms of either side agree to a few ulps.  (The
    oracle cuts a train DRM to rank_min:rank_max for these two kinds; its dense and Tucker chains hand out whole cores.)"""
    rng = np.random.default_rng(11)
    if kind == "tt":
        cores = orc.random_tt(SHAPE, 3, rng)
        X = orc.tt_to_numpy(cores)
    else:
        cores = [rng.standard_normal((n, 3)) for n in SHAPE]
        X = np.einsum("at,bt,ct,dt->abcd", *cores)
    left, right = _drm((4, 5, 6), False, seed=5), _drm((5, 6, 7), True, seed=6)
    lt, rt = left.as_train(), right.as_train()
    ld = orc.TTDrm([np.asarray(c) for c in lt.cores], SHAPE, False, rank_min=tuple(lt.rank_min), rank_max=tuple(lt.rank_max))
    rd = orc.TTDrm([np.asarray(c) for c in rt.cores], SHAPE, True, rank_min=tuple(rt.rank_min), rank_max=tuple(rt.rank_max))
    Psis, Omegas = orc.general_sketch(kind, cores, ld, rd, "streaming")
    Psi, Omega = ref.sketch(X, ref.of_drm(left), ref.of_drm(right))
    assert [p.shape for p in Psi] == [(1, 6, 5), (4, 5, 6), (5, 4, 7), (6, 7, 1)]
    for a, b in zip(Psi + Omega, Psis + Omegas):
        assert a.shape == b.shape
        assert np.linalg.norm(a - b) <= 1e-12 * np.linalg.norm(b)
