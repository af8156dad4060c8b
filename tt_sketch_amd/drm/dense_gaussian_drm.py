"""Dense Gaussian DRM: one explicit (rank, prod n_{<=mu}) Gaussian matrix per unfolding.

API of the reference's ``tt_sketch/drm/dense_gaussian_drm.py:17-80``.  Matrices are filled on
the device, row-major, keyed by (seed, mu, element) so that the leading rows are unchanged
when the rank grows (CanIncreaseRank) and a ``rank_min:rank_max`` slice is a row view.
For parity tests ``sketching_mats`` may be overwritten after construction.

``stored=False`` (``LazyGaussianDRM``) keeps no matrix: ``sketching_mats[mu]`` is the recipe ``LazyGaussian`` of the same
matrix -- (seed, row range, row length) -- and a dense tensor is sketched by ``ttsk_gauss_lazy_left`` / ``_right``
(``csrc/gauss_lazy.hip``), which sample the entries where the product consumes them.  ``slice`` and ``increase_rank`` then
touch no device memory; every other tensor kind, and a shape outside the kernels' cover, fills the matrix on demand.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple, Union

import numpy as np

from .. import _native as nat
from ..device import DevArray, as_dev, contract
from ..drm_base import CanIncreaseRank, handle_transpose
from ..sketching_methods.abstract_methods import CansketchDense, CansketchSparse, CansketchTT
from ..utils import random_normal_dev


class LazyGaussian:
    """Rows ``[row_lo, row_hi)`` of ``random_normal_dev((rows, cols), seed)`` as a recipe: nothing is sampled until a
    product consumes the entries (``dense_sketch``) or somebody asks for the matrix (``materialise`` / ``get`` /
    ``np.asarray`` / ``as_dev``), which runs that very fill and cuts the rows."""
    __slots__ = ("seed", "row_lo", "row_hi", "cols", "rows")

    def __init__(self, seed: int, row_lo: int, row_hi: int, cols: int, rows: Optional[int] = None):
        self.seed, self.row_lo, self.row_hi, self.cols = int(seed), int(row_lo), int(row_hi), int(cols)
        self.rows = self.row_hi if rows is None else int(rows)
        if not 0 <= self.row_lo <= self.row_hi <= self.rows or self.cols < 1:
            raise ValueError(f"LazyGaussian: rows [{row_lo}, {row_hi}) of ({self.rows}, {cols})")

    @property
    def shape(self) -> Tuple[int, int]:
        return (self.row_hi - self.row_lo, self.cols)

    def materialise(self) -> DevArray:
        return random_normal_dev((self.rows, self.cols), seed=self.seed)[self.row_lo:self.row_hi]

    __dev_array__ = materialise                      # what ``device.as_dev`` asks for

    def get(self) -> np.ndarray:
        return self.materialise().get()

    def __array__(self, dtype=None, copy=None):
        a = self.get()
        return a if dtype is None else a.astype(dtype)

    def __repr__(self) -> str:
        return f"<LazyGaussian rows [{self.row_lo}, {self.row_hi}) of ({self.rows}, {self.cols}), seed {self.seed:#x}>"


def _rebuilt(drm, **kw):
    """a recipe DRM of the same class, shape, side and seed: no device is touched"""
    return type(drm)(shape=drm.shape, transpose=drm.transpose, seed=drm.seed, stored=False, **kw)


class DenseGaussianDRM(CansketchTT, CansketchSparse, CansketchDense, CanIncreaseRank):
    sketching_mats: list

    def __init__(self, rank: Union[Tuple[int, ...], int], shape: Tuple[int, ...], transpose: bool,
                 seed: Optional[int] = None, stored: bool = True, **kwargs) -> None:
        super().__init__(rank, shape, transpose, seed=seed, **kwargs)
        walk = self.shape[::-1] if transpose else self.shape
        self.stored = bool(stored)
        self.sketching_mats = []
        cols = 1
        for mu, (r, n) in enumerate(zip(self.true_rank, walk[:-1])):
            cols *= n
            seed_mu = (self.seed << 20) + 0x5A5A0000 + mu
            if self.stored:
                full = random_normal_dev((r, cols), seed=seed_mu)
                self.sketching_mats.append(full[self.rank_min[mu]:self.rank_max[mu]])
            else:
                self.sketching_mats.append(LazyGaussian(seed_mu, self.rank_min[mu], self.rank_max[mu], cols, r))

    def slice(self, start_rank, end_rank) -> "DenseGaussianDRM":
        if self.stored:
            return super().slice(start_rank, end_rank)
        full = self.true_rank[::-1] if self.transpose else self.true_rank
        return _rebuilt(self, rank=self.rank, rank_min=start_rank, rank_max=end_rank, true_rank=full)

    def increase_rank(self, new_rank) -> "DenseGaussianDRM":
        return super().increase_rank(new_rank) if self.stored else _rebuilt(self, rank=new_rank)

    def _mat(self, mu) -> DevArray:
        """the matrix of level mu in device memory: the stored one, or a recipe's, filled at its first use here"""
        m = self.sketching_mats[mu]
        if isinstance(m, LazyGaussian):
            made = self.__dict__.setdefault("_filled", {})
            if made.get(mu, (None, None))[0] is not m:
                made[mu] = (m, m.materialise())
            return made[mu][1]
        if not isinstance(m, DevArray):
            m = self.sketching_mats[mu] = as_dev(m)
        return m

    @handle_transpose
    def sketch_dense(self, tensor):
        """reference :77-80."""
        for mu in range(len(self.sketching_mats)):
            m = self.sketching_mats[mu]
            yield m if isinstance(m, LazyGaussian) else self._mat(mu)

    @handle_transpose
    def sketch_tt(self, tensor):
        """(mat_mu @ X_{<=mu}).T with X_{<=mu} the dense partial product (reference :68-75)."""
        Xs = tensor.dev_cores()
        P = Xs[0].reshape(-1, Xs[0].shape[-1])
        for mu in range(len(self.sketching_mats)):
            if mu > 0:
                P = contract("ij,jkl->ikl", P, Xs[mu])
                P = P.reshape(-1, P.shape[-1])
            yield contract("ri,is->sr", self._mat(mu), P)

    @handle_transpose
    def sketch_sparse(self, tensor):
        """Columns of mat_mu at the C-order ravelled leading indices (reference :59-66)."""
        idx = tensor.dev_indices()
        order = tensor.dev_row_order
        N = tensor.nnz
        for mu in range(len(tensor.shape) - 1):
            mat = self._mat(mu).contiguous()
            rank, cols = mat.shape
            out = DevArray.empty((N, rank))
            m = mu + 1
            nat.call("ttsk_sparse_densedrm_gather", mat, rank, cols, idx, N, (ctypes.c_int * m)(*order[:m]),
                     nat.i64_array(tensor.shape[:m]), m, N, out, 0)
            yield out.T


class LazyGaussianDRM(DenseGaussianDRM):
    """``DenseGaussianDRM(..., stored=False)`` under a name of its own, for ``left_drm_type=`` / ``right_drm_type=``: the
    same matrices as the stored class gives for the seed, none of them in memory."""

    def __init__(self, rank: Union[Tuple[int, ...], int], shape: Tuple[int, ...], transpose: bool,
                 seed: Optional[int] = None, stored: bool = False, **kwargs) -> None:
        if stored:
            raise ValueError("LazyGaussianDRM stores no matrices: DenseGaussianDRM is the stored class")
        super().__init__(rank, shape, transpose, seed=seed, stored=False, **kwargs)
