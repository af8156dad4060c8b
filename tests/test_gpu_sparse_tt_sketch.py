"""Streaming sketches of sparse tensors with TensorTrainDRM through the one-pass sparse path (sparse_fused.py: chain factors
of csrc/sparse_pass.h, tables of the DRM's partial products) at the Python level: against the oracle, against the panel path
(``paths.forced("composed")``), against itself, and what it allocates."""
import numpy as np
import pytest

from oracle import ttsk_oracle as orc

from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = 1e-12            # the project's tolerance for TT-DRM cases (no ndtri is involved)
TOL_HASHED = 1e-11     # of the existing hashed-DRM tests
C4 = (200, 150, 100, 120, 300)


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb else 1.0)


def _sparse(shape, nnz, seed):
    rng = np.random.default_rng(seed)
    idx = np.stack([rng.integers(0, n, nnz) for n in shape]).astype(np.int64)
    return idx, rng.standard_normal(nnz)


def _tt_pair(tsa, shape, l, r, seed):
    rng = np.random.default_rng(seed)
    old, ord_ = orc.random_tt_drm(shape, l, False, rng), orc.random_tt_drm(shape, r, True, rng)
    t = lambda v: v if isinstance(v, tuple) else (v,) * (len(shape) - 1)
    return (tsa.TensorTrainDRM(t(l), shape, transpose=False, cores=old.cores),
            tsa.TensorTrainDRM(t(r), shape, transpose=True, cores=ord_.cores), old, ord_)


def _kernel_sketch(tsa, T, ld, rd):
    from tt_sketch_amd import paths, sparse_fused
    with paths.forced("kernel"):
        assert sparse_fused.try_sparse_gauss_sketch(T, ld, rd, tsa.SketchMethod.streaming) is not None
        sk = tsa.general_sketch(T, ld, rd, tsa.SketchMethod.streaming)
    return sk.Psi_cores + sk.Omega_mats


@pytest.mark.parametrize("case", [
    # (shape, nnz, left ranks, right ranks)
    ((7, 9), 1, 3, 4),
    ((7, 9), 33, 3, 4),
    ((7, 9), 5000, 5, 2),                                  # every level a table
    ((6, 1, 11), 1, 2, 3),                                 # a mode of extent 1; one nonzero: chains from the first core
    ((6, 1, 11), 33, (2, 5), (4, 3)),
    ((300, 7, 250), 5000, (16, 17), (32, 9)),              # ranks on either side of 16, up to the cover; non-uniform
    ((5, 4, 1, 6, 7), 1, 3, 2),
    ((5, 4, 1, 6, 7), 33, (2, 3, 4, 5), (5, 4, 3, 2)),
    ((40, 30, 20, 25, 35), 5000, (4, 9, 6, 7), (8, 5, 11, 3)),
    (C4, 200000, 10, 15),                                  # tables up to level 1 on both sides, chains of up to three steps
], ids=lambda c: "x".join(map(str, c[0])) + f"-nnz{c[1]}")
def test_tt_drm_pass_against_the_oracle(tsa, case):
    """kernel route == the oracle's restatement of tensor_train_drm.py:60-69 + sparse_sketch.py:8-69, == the panel path, and
    the same bits on a second run with fresh objects"""
    from tt_sketch_amd import paths
    shape, nnz, l, r = case
    idx, val = _sparse(shape, nnz, nnz + len(shape))
    ld, rd, old, ord_ = _tt_pair(tsa, shape, l, r, 3)
    got = _kernel_sketch(tsa, tsa.SparseTensor(shape, idx, val), ld, rd)
    oP, oO = orc.general_sketch("sparse", (shape, idx, val), old, ord_, "streaming")
    for a, b in zip(got, oP + oO):
        assert a.shape == b.shape and rel(a, b) < TOL, (a.shape, rel(a, b))
    ld2, rd2, _, _ = _tt_pair(tsa, shape, l, r, 3)
    for a, b in zip(got, _kernel_sketch(tsa, tsa.SparseTensor(shape, idx, val), ld2, rd2)):
        assert np.array_equal(a, b)
    with paths.forced("composed"):
        sk = tsa.general_sketch(tsa.SparseTensor(shape, idx, val), ld, rd, tsa.SketchMethod.streaming)
    for a, b in zip(got, sk.Psi_cores + sk.Omega_mats):
        assert rel(a, b) < TOL, rel(a, b)


@pytest.mark.parametrize("case", [
    # (shape, nnz, which side is the train, the hashed side: (kind, true rank, lo, hi, non-zeros per row))
    ((300, 7, 250, 9), 9000, "left", ("g", 13, 2, 15, None)),
    ((300, 7, 250, 9), 9000, "right", ("s", 16, 3, 11, 9)),
    ((40, 30, 20, 25, 35), 5000, "left", ("s", 24, 0, 24, 5)),
    ((40, 30, 20, 25, 35), 5000, "right", ("g", 20, 0, 20, None)),
], ids=lambda c: f"train-{c[2]}-{c[3][0]}")
def test_tt_drm_beside_a_hashed_drm(tsa, case):
    """TT x SparseGaussian / SparseSign and SparseSign / SparseGaussian x TT against the oracle"""
    shape, nnz, side, (kind, tr, lo, hi, nz) = case
    d = len(shape)
    idx, val = _sparse(shape, nnz, nnz)
    t = lambda v: (v,) * (d - 1)
    transpose = side == "left"                             # the hashed DRM takes the other side
    if kind == "g":
        hd = tsa.SparseGaussianDRM(t(hi), shape, transpose, seed=4, rank_min=t(lo), rank_max=t(hi), true_rank=t(hi))
        ho = orc.HashGaussDrm(4, shape, transpose, t(lo), t(hi))
    else:
        hd = tsa.SparseSignDRM(t(tr), shape, transpose, seed=4, rank_min=t(lo), rank_max=t(hi), true_rank=t(tr),
                               num_non_zero_per_row=None if nz is None else t(nz))
        ho = orc.HashSignDrm(4, shape, transpose, t(tr), t(lo), t(hi), None if nz is None else t(nz))
    rng = np.random.default_rng(8)
    to = orc.random_tt_drm(shape, 7, not transpose, rng)
    td = tsa.TensorTrainDRM(t(7), shape, transpose=not transpose, cores=to.cores)
    ld, rd, old, ord_ = (td, hd, to, ho) if side == "left" else (hd, td, ho, to)
    got = _kernel_sketch(tsa, tsa.SparseTensor(shape, idx, val), ld, rd)
    oP, oO = orc.general_sketch("sparse", (shape, idx, val), old, ord_, "streaming")
    for a, b in zip(got, oP + oO):
        assert a.shape == b.shape and rel(a, b) < TOL_HASHED, (a.shape, rel(a, b))


def test_blocked_sketch_equals_the_blocks_of_the_unblocked_one(tsa):
    """rank slices of seeded TensorTrainDRMs (a slice keeps the whole cores and cuts the last one): the chain factor's
    [lo, lo + w) and, where the level has a table, the cut table"""
    from tt_sketch_amd import paths
    shape, nnz = (30, 7, 25, 9), 4000
    idx, val = _sparse(shape, nnz, 2)
    T = tsa.SparseTensor(shape, idx, val)
    ld = tsa.TensorTrainDRM((9, 9, 9), shape, transpose=False, seed=21)
    rd = tsa.TensorTrainDRM((12, 12, 12), shape, transpose=True, seed=22)
    with paths.forced("kernel"):
        whole = tsa.general_sketch(T, ld, rd, tsa.SketchMethod.streaming)
        blocked = tsa.blocked_stream_sketch(T, ld, rd, [(0,) * 3, (4,) * 3, (9,) * 3], [(0,) * 3, (5,) * 3, (12,) * 3])
    for a, b in zip(blocked.Psi_cores + blocked.Omega_mats, whole.Psi_cores + whole.Omega_mats):
        assert a.shape == b.shape and rel(a, b) < TOL, rel(a, b)


def test_sum_of_three_shards_equals_the_whole(tsa):
    shape, nnz = (40, 30, 20, 25), 6000
    idx, val = _sparse(shape, nnz, 5)
    ld, rd, _, _ = _tt_pair(tsa, shape, 6, 8, 9)
    whole = _kernel_sketch(tsa, tsa.SparseTensor(shape, idx, val), ld, rd)
    cuts = [0, 1500, 1533, nnz]
    shards = tsa.TensorSum([tsa.SparseTensor(shape, idx[:, a:b], val[a:b]) for a, b in zip(cuts, cuts[1:])])
    for a, b in zip(_kernel_sketch(tsa, shards, ld, rd), whole):
        assert rel(a, b) < TOL, rel(a, b)


def test_second_sketch_allocates_no_panel(tsa, monkeypatch):
    """with the tensor's streams and the DRM's tables cached, a sketch allocates its outputs only: nothing of 8 nnz bytes"""
    from tt_sketch_amd import paths, sparse_fused
    from tt_sketch_amd.device import DevArray
    nnz = 200000
    idx, val = _sparse(C4, nnz, 1)
    T = tsa.SparseTensor(C4, idx, val)
    ld, rd, _, _ = _tt_pair(tsa, C4, 10, 15, 3)
    sizes = []

    def counted(name):
        orig = getattr(DevArray, name).__func__

        def wrapper(cls, shape, dtype=np.float64, stream=0):
            out = orig(cls, shape, dtype, stream)
            sizes.append(out.size * out.dtype.itemsize)
            return out
        return classmethod(wrapper)

    with paths.forced("kernel"):
        first = sparse_fused.try_sparse_gauss_sketch(T, ld, rd, tsa.SketchMethod.streaming)
        assert first is not None
        monkeypatch.setattr(DevArray, "empty", counted("empty"))
        monkeypatch.setattr(DevArray, "zeros", counted("zeros"))
        second = sparse_fused.try_sparse_gauss_sketch(T, ld, rd, tsa.SketchMethod.streaming)
    assert second is not None and sizes, "the one-pass path declined or allocated nothing"
    print(f"[sparse tt] largest allocation of the second sketch {max(sizes)} bytes, 8 nnz = {8 * nnz}")
    assert max(sizes) < 8 * nnz, sorted(sizes)[-4:]
    for a, b in zip(first[0] + first[1], second[0] + second[1]):
        assert np.array_equal(a.get(), b.get())
