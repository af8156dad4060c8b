"""``DenseGaussianDRM(stored=False)`` / ``LazyGaussianDRM`` on the host: the recipes and their rank bookkeeping, with nothing
of a device.  ``device._Buffer`` is a NumPy-backed buffer that records every allocation, and ``nat.call`` goes to Python
emulations of the three entry points a materialisation needs: ``ttsk_fill_normal`` (element i of a fill of seed s is the
number ``1000 * (s % 997) + i``, so a row cut shows which rows and which seed it came from), ``ttsk_copy_strided`` and
``ttsk_d2h``."""
import ctypes

import numpy as np
import pytest

import tt_sketch_amd.device as dev
from tt_sketch_amd import _native as nat_mod
from tt_sketch_amd.device import DevArray

SHAPE = (6, 5, 4, 7)


def _seed_mu(seed, mu):
    return (seed << 20) + 0x5A5A0000 + mu


def _fill_value(seed, i):
    return 1000.0 * (seed % 997) + i


class Library:
    def __init__(self):
        self.allocated, self.calls, self.buffers = [], [], []

    def view(self, addr, n):
        for base, mem in self.buffers:
            if base <= addr and addr + 8 * n <= base + mem.size:
                return mem[addr - base:addr - base + 8 * n].view(np.float64)
        raise AssertionError("access of %d doubles at %#x is inside no buffer" % (n, addr))

    def call(self, name, *args):
        self.calls.append((name, args))
        addr = lambda x: x.ptr if isinstance(x, DevArray) else int(x)
        if name == "ttsk_fill_normal":
            out, n, seed, scale = addr(args[0]), int(args[1]), int(args[2]), float(args[3])
            assert scale == 1.0
            self.view(out, n)[:] = _fill_value(seed, np.arange(n))
        elif name == "ttsk_copy_strided":
            nd = int(args[2])
            shape, ds, ss = (list(a)[:nd] for a in args[3:6])
            span = lambda st: 1 + sum((n - 1) * s for n, s in zip(shape, st))
            src = np.lib.stride_tricks.as_strided(self.view(addr(args[1]), span(ss)), shape=shape, strides=[8 * s for s in ss]).copy()
            np.lib.stride_tricks.as_strided(self.view(addr(args[0]), span(ds)), shape=shape, strides=[8 * s for s in ds])[...] = src
        elif name == "ttsk_d2h":
            ctypes.memmove(int(args[0]), addr(args[1]), int(args[2]))
        else:
            raise AssertionError("unexpected call of %s" % name)


@pytest.fixture
def lib(monkeypatch):
    L = Library()

    class Buffer:
        def __init__(self, nbytes, stream=0):
            self.nbytes = int(nbytes)
            self.mem = np.full(max(self.nbytes, 8) + 8, 0xFF, dtype=np.uint8)
            self.ptr = self.mem.ctypes.data
            L.buffers.append((self.ptr, self.mem))
            L.allocated.append(self.nbytes)

    monkeypatch.setattr(dev, "_Buffer", Buffer)
    monkeypatch.setattr(nat_mod, "call", L.call)
    return L


def _walk(transpose):
    return SHAPE[::-1] if transpose else SHAPE


def test_exported_not_in_all_drm_and_defaults_unchanged():
    import inspect

    import tt_sketch_amd as tsa
    from tt_sketch_amd.drm import ALL_DRM, LazyGaussian, LazyGaussianDRM
    from tt_sketch_amd.drm_base import CanIncreaseRank, CanSlice
    from tt_sketch_amd.sketching_methods import abstract_methods as am
    assert tsa.LazyGaussianDRM is LazyGaussianDRM and LazyGaussianDRM not in ALL_DRM and len(ALL_DRM) == 4
    assert issubclass(LazyGaussianDRM, tsa.DenseGaussianDRM)
    for cap in (CanSlice, CanIncreaseRank, am.CansketchTT, am.CansketchSparse, am.CansketchDense):
        assert issubclass(LazyGaussianDRM, cap), cap
    assert inspect.signature(tsa.DenseGaussianDRM.__init__).parameters["stored"].default is True
    assert LazyGaussian(7, 1, 3, 10).shape == (2, 10)
    with pytest.raises(ValueError):
        LazyGaussianDRM(3, SHAPE, False, seed=1, stored=True)
    with pytest.raises(ValueError):
        LazyGaussian(7, 3, 1, 10)


@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("by_class", [False, True])
def test_recipes_and_rank_bookkeeping_allocate_nothing(lib, transpose, by_class):
    from tt_sketch_amd import DenseGaussianDRM, LazyGaussianDRM
    from tt_sketch_amd.drm import LazyGaussian
    rank = (4, 5, 6)
    drm = LazyGaussianDRM(rank, SHAPE, transpose, seed=9) if by_class else DenseGaussianDRM(rank, SHAPE, transpose, seed=9, stored=False)
    stored = rank[::-1] if transpose else rank
    cols = np.cumprod(_walk(transpose)[:-1])
    assert drm.stored is False and drm.rank == stored
    for mu, m in enumerate(drm.sketching_mats):
        assert type(m) is LazyGaussian
        assert (m.seed, m.row_lo, m.row_hi, m.cols, m.rows) == (_seed_mu(9, mu), 0, stored[mu], cols[mu], stored[mu])
        assert m.shape == (stored[mu], cols[mu])
    lo, hi = (1, 2, 3), (3, 5, 4)
    cut = drm.slice(lo, hi)
    slo, shi = (lo[::-1], hi[::-1]) if transpose else (lo, hi)
    assert type(cut) is type(drm) and cut.stored is False and cut.true_rank == drm.true_rank
    assert cut.rank_min == slo and cut.rank_max == shi and cut.rank == tuple(b - a for a, b in zip(slo, shi))
    for mu, m in enumerate(cut.sketching_mats):
        assert (m.seed, m.row_lo, m.row_hi, m.cols, m.rows) == (_seed_mu(9, mu), slo[mu], shi[mu], cols[mu], stored[mu])
    lead = drm.slice(None, (2, 2, 2))
    assert [(m.row_lo, m.row_hi) for m in lead.sketching_mats] == [(0, 2)] * 3
    grown = drm.increase_rank((6, 7, 9))
    big = (9, 7, 6) if transpose else (6, 7, 9)
    assert type(grown) is type(drm) and grown.stored is False and grown.rank == big and grown.seed == drm.seed
    for mu, (a, b) in enumerate(zip(drm.sketching_mats, grown.sketching_mats)):
        assert (b.seed, b.row_lo, b.row_hi, b.cols, b.rows) == (a.seed, 0, big[mu], a.cols, big[mu])
    other = drm.T
    assert other.transpose is (not transpose) and other.sketching_mats is drm.sketching_mats
    assert lib.allocated == [] and lib.calls == []


@pytest.mark.parametrize("transpose", [False, True])
def test_materialisation_is_the_full_fill_cut_to_the_rows(lib, transpose):
    from tt_sketch_amd import LazyGaussianDRM
    from tt_sketch_amd.device import as_dev
    drm = LazyGaussianDRM((4, 5, 6), SHAPE, transpose, seed=9)
    cut = drm.slice((1, 2, 3), (3, 5, 4))
    for mu, m in enumerate(cut.sketching_mats):
        del lib.calls[:], lib.allocated[:]
        got = np.asarray(m)
        fills = [a for name, a in lib.calls if name == "ttsk_fill_normal"]
        assert len(fills) == 1 and int(fills[0][1]) == m.rows * m.cols and int(fills[0][2]) == _seed_mu(9, mu) == m.seed
        assert lib.allocated[0] == 8 * m.rows * m.cols
        want = _fill_value(m.seed, np.arange(m.rows * m.cols)).reshape(m.rows, m.cols)[m.row_lo:m.row_hi]
        assert np.array_equal(got, want)
        for other in (m.get(), as_dev(m).get(), m.materialise().get(), cut._mat(mu).get()):
            assert np.array_equal(other, want)
    # the leading rows of a grown DRM are the old ones -- for as many columns as the fill is keyed by: (row, column) -> row * cols + column
    grown = drm.increase_rank((6, 7, 9))
    for a, b in zip(drm.sketching_mats, grown.sketching_mats):
        assert np.array_equal(np.asarray(a), np.asarray(b)[:a.shape[0]])
    # a stored DRM's _mat caches in place; a recipe stays in sketching_mats, its matrix is kept beside it
    first = cut._mat(0)
    assert cut._mat(0) is first and type(cut.sketching_mats[0]).__name__ == "LazyGaussian"


def test_dispatch_passes_recipes_through_and_prepare_left_declines(lib):
    from tt_sketch_amd import LazyGaussianDRM
    from tt_sketch_amd.sketching_methods import dense_sketch as ds
    drm = LazyGaussianDRM(4, (4, 4, 4, 4, 64), False, seed=3)
    mats = list(drm.sketching_mats)
    for m in mats:
        assert ds._norm(m) is m and ds._mat(m) is m
        assert ds._ident(m) == ("lazy", m.seed, m.row_lo, m.row_hi, m.cols)
    assert ds._ident(mats[0]) == ds._ident(drm.slice(None, None).sketching_mats[0]) != ds._ident(mats[1])

    class NoTensor:
        def dev_data(self):
            raise AssertionError("prepare_left looked at the tensor")
    assert ds.prepare_left(NoTensor(), mats) is False
    assert lib.allocated == [] and lib.calls == []
