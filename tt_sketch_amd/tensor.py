"""Tensor types of the sketch API: the data model, its host arithmetic and HBM residency.

Mirrors the public surface of the reference's ``tt_sketch/tensor.py`` (classes,
constructor signatures, ``.T``, ``shape``/``rank``/``cores``...), because these are
the input and output types of ``stream_sketch`` / ``orthogonal_sketch`` /
``hmt_sketch``.  What is new here is residency: every tensor lazily uploads its
payload to HBM once (``dev_*`` accessors) and ``.T`` re-uses that upload through
strided views, so a right sketch (drm_base.py:122-145 in the reference transposes
the tensor on every call) costs no copy and no PCIe traffic.

The arithmetic of the classes (``error``, ``norm``, ``dot``, ``round``, ...) is plain NumPy on the host.  Where a method
has a device form it decides here whether to take it, and the pass itself lives beside the name of its kernel, reached
by an import inside the method: ``tensor_gather`` (evaluation of a train, a CP or a Tucker tensor at index lists:
``gather_dev``, ``support_error``, ``SparseTensor.dot``), ``tensor_tucker`` (a ``TuckerTensor`` against a Tucker tensor, a
train or a CP tensor: resident ``dot`` / ``norm`` / ``error(fast=True)``), ``tensor_dense`` (the pass over a dense
tensor: ``dense_stats``, ``to_dense_dev`` and with them
``error`` / ``dot`` against a ``DenseTensor``) and ``tensor_gram`` (``tt_gram``, ``cp_gram`` and the chain of a train against a
``CPTensor``: resident ``dot`` / ``norm`` / ``error(fast=True)``), ``tensor_round`` (Gram-SVD rounding: ``round_gram``,
``svdvals_gram``) and ``tensor_sparse`` (the sorted-key join: ``SparseTensor.dot`` against a sparse or a dense tensor,
``SparseTensor.gather`` / ``gather_dev``).  Those modules import the classes from this one and
never ``_host``, so a device pass has no way to a host copy.  The TT sweeps ``orthogonalize_dev`` / ``round_dev`` are
methods without a helper layer and stay with ``TensorTrain``.

Residency contract: payload arrays are treated as immutable once a tensor has been
sketched; replace a core (``tt[i] = new``) rather than writing into it, or call
``invalidate_device()``.
"""
from __future__ import annotations

import abc
from functools import cached_property
from typing import Dict, Iterable, List, Optional, Tuple, Union

import numpy as np
import numpy.typing as npt

from .device import DevArray, as_dev, axpby, contract, copy_into
from .utils import ArrayList, TTRank, process_tt_rank, random_normal


def _host(a) -> np.ndarray:
    return a.get() if isinstance(a, DevArray) else np.asarray(a)


def _same_objects(key, items) -> bool:
    """The cached device copies belong to exactly these payload objects (identity, not id(): the id of
    a collected array can be handed to a new one)."""
    return key is not None and len(key) == len(items) and all(a is b for a, b in zip(key, items))


def _prod(xs) -> int:
    out = 1
    for x in xs:
        out *= int(x)
    return out


def _dense_current(dense: "DenseTensor") -> bool:
    """The dense tensor lives on the device, or has an upload that is still current."""
    return isinstance(dense.data, DevArray) or (dense._dev is not None and dense._dev_src is dense.data)


def _on_device(t) -> bool:
    """The condition of ``SparseTensor.dot`` for a device path: the payload lives in HBM only, or is uploaded already."""
    return t.resident() or t._dev is not None


def _fast_error(aa, ab, bb):
    """``||a - b||`` from ``<a, a>``, ``<a, b>`` and ``<b, b>`` by the reference's fast formula (tensor.py:68-72), whose
    floor is a relative error of about 1e-8.  No guard for ``aa + bb == 0``: a caller that has one keeps it."""
    tot = aa + bb
    return np.sqrt(tot) * np.sqrt(abs(1 - 2 * ab / tot))


def _error_tail(err, ref_norm, shape, relative: bool, rmse: bool):
    """The tail of every ``error``: ``relative`` divides by ``ref_norm`` (read only then; ``inf`` against a zero
    reference), ``rmse`` by ``sqrt(prod(shape))``."""
    if relative:
        if ref_norm == 0:
            return np.inf
        err /= ref_norm
    if rmse:
        err /= np.sqrt(np.prod(shape))
    return err


class _CoreList:
    """What ``TensorTrain`` and ``CPTensor`` share: a list ``cores`` of payload arrays, its cached upload ``_dev`` with
    the objects it was made from (``_dev_key``), and the gather kernels' ``gather_dev`` / ``support_error``."""

    def _set_cores(self, cores: ArrayList, _dev) -> None:
        self.cores = cores
        self._dev = _dev
        self._dev_key = None if _dev is None else tuple(cores)      # the objects, compared with `is`

    def _dev_current(self) -> Optional[List[DevArray]]:
        """The cached device copies if they still belong to the current core objects, None otherwise."""
        return self._dev if self._dev is not None and _same_objects(self._dev_key, self.cores) else None

    def dev_cores(self) -> List[DevArray]:
        if self._dev_current() is None:
            self._dev = [as_dev(c) for c in self.cores]
            self._dev_key = tuple(self.cores)
        return self._dev

    prepare_device = dev_cores

    def resident(self) -> bool:
        """True if the cores (factor matrices) live in HBM only (as ``to_tt`` / ``round_dev`` / an MPO product leave
        them); arithmetic on such a tensor stays on the device."""
        return all(isinstance(c, DevArray) for c in self.cores)

    def __getitem__(self, k: int):
        return self.cores[k]

    def __setitem__(self, k: int, data) -> None:
        self.cores[k] = data
        self.invalidate_device()

    def gather_dev(self, idx) -> DevArray:
        """Entries at the given multi-indices as a device array (N,): ``idx`` is a ``SparseTensor`` of this shape (its
        resident index matrix is used in place), a ``(d, N)`` array or a tuple of ``d`` arrays."""
        from .tensor_gather import _gather_device
        return _gather_device(self, idx, True, False)[0]

    def support_error(self, sparse: "SparseTensor", relative: bool = False) -> float:
        """``|| self[indices] - entries ||`` over ALL nonzeros of ``sparse`` in one device pass (the figure the
        reference's scripts/frostt.py:112-116 forms on a sample of 10^4); exact where ``error(fast=True)`` has lost
        everything below 1e-8.  ``relative``: divided by ``||entries||``."""
        from .tensor_gather import _gather_device
        err = float(np.sqrt(_gather_device(self, sparse, False, True)[1][2]))
        return _error_tail(err, sparse.norm() if relative else None, None, relative, False)


class Tensor(abc.ABC):
    """Base class: shape, transpose, conversion and the lazy-sum arithmetic."""

    shape: Tuple[int, ...]

    @property
    @abc.abstractmethod
    def T(self):
        """Tensor with the order of the modes reversed."""

    @property
    @abc.abstractmethod
    def size(self) -> int:
        """Number of stored floating point values."""

    @abc.abstractmethod
    def to_numpy(self) -> npt.NDArray[np.float64]:
        """Dense ndarray of the same shape."""

    def prepare_device(self) -> None:
        """Upload the payload to HBM (once); views such as ``.T`` then share it."""

    def invalidate_device(self) -> None:
        for name in ("_dev", "_dev_key"):
            if hasattr(self, name):
                setattr(self, name, None)

    @property
    def ndim(self) -> int:
        return len(self.shape)

    def dense(self) -> "DenseTensor":
        return DenseTensor(self.to_numpy())

    # -- error / norms (host NumPy; reference tensor.py:53-88)
    def error(self, other, relative: bool = False, rmse: bool = False, fast: bool = False) -> float:
        if isinstance(other, np.ndarray):
            other = DenseTensor(other)
        ref_norm = other.norm()
        if fast:
            err = _fast_error(self.norm()**2, self.dot(other), ref_norm**2)
        else:
            err = np.linalg.norm(self.to_numpy() - other.to_numpy())
        return _error_tail(err, ref_norm, self.shape, relative, rmse)

    def dot(self, other, reverse: bool = False) -> float:
        if isinstance(other, TensorSum):
            return other.dot(self)
        if not reverse:
            return other.dot(self, reverse=True)
        return float(np.dot(self.to_numpy().ravel(), other.to_numpy().ravel()))

    def norm(self) -> float:
        return float(np.sqrt(abs(self.dot(self))))

    def __matmul__(self, other) -> float:
        return self.dot(other)

    # -- lazy sums (reference tensor.py:100-123)
    def __add__(self, other) -> "TensorSum":
        mine = self.tensors if isinstance(self, TensorSum) else [self]
        theirs = other.tensors if isinstance(other, TensorSum) else [other]
        return TensorSum(list(mine) + list(theirs))

    @abc.abstractmethod
    def __mul__(self, other: float):
        """Scalar multiple."""

    def __rmul__(self, other: float):
        return self.__mul__(other)

    def __truediv__(self, other: float):
        return self.__mul__(1 / other)

    def __neg__(self):
        return self * -1

    def __sub__(self, other):
        return self + (-other)


# --------------------------------------------------------------------------- dense
class DenseTensor(Tensor):
    """Full ndarray (reference tensor.py:140-182)."""

    def __init__(self, data, _dev: Optional[DevArray] = None) -> None:
        self.data = data                  # ndarray, or a DevArray for a tensor built on the device
        self.shape = tuple(data.shape)
        self._dev = _dev
        self._dev_src = data if _dev is not None else None

    def dev_data(self) -> DevArray:
        if self._dev is None or self._dev_src is not self.data:    # `.data` was replaced: upload again
            self._dev = as_dev(self.data)
            self._dev_src = self.data
        return self._dev

    prepare_device = dev_data

    @property
    def T(self) -> "DenseTensor":
        axes = tuple(reversed(range(len(self.shape))))
        if isinstance(self.data, DevArray):
            return DenseTensor(self.data.transpose(axes))
        cur = self._dev is not None and self._dev_src is self.data
        return DenseTensor(np.transpose(self.data, axes), self._dev.transpose(axes) if cur else None)

    @property
    def size(self) -> int:
        return int(np.prod(self.shape))

    def to_numpy(self):
        return _host(self.data)

    def norm(self) -> float:
        """``||X||``: on the device (``ttsk_sumsq``, fixed summation order) for a device tensor or one with a current
        upload, host NumPy otherwise."""
        if not _dense_current(self):
            return super().norm()
        from . import _native as nat
        arr = self.dev_data()
        if not (arr.is_contiguous() or arr.T.is_contiguous()):      # a sum over all entries: their order is free
            arr = arr.contiguous()
        out = DevArray.empty((1,))
        nat.call("ttsk_sumsq", arr, arr.size, out, 0)
        return float(np.sqrt(out.get()[0]))

    def dot(self, other, reverse=False) -> float:
        if isinstance(other, TensorTrain) and (other.resident() or _dense_current(self)):
            return float(other.dense_stats(self)[0])                  # one pass over the tensor, nothing downloaded
        return super().dot(other, reverse=reverse)

    def to_sparse(self) -> "SparseTensor":
        X = self.to_numpy()
        idx = np.indices(X.shape).reshape(X.ndim, -1)
        return SparseTensor(X.shape, idx, X.reshape(-1))

    def __mul__(self, other: float) -> "DenseTensor":
        return DenseTensor(self.to_numpy() * other)

    @classmethod
    def random(cls, shape: Tuple[int, ...]) -> "DenseTensor":
        return cls(random_normal(shape))

    def __repr__(self) -> str:
        return f"<Dense tensor of shape {self.shape} at {hex(id(self))}>"


# --------------------------------------------------------------------------- sparse
class SparseTensor(Tensor):
    """COO tensor: ``indices`` (d, nnz) int64, ``entries`` (nnz,) (reference tensor.py:185-291).

    On the device the index matrix is uploaded once; ``.T`` only reverses the order in
    which its rows are addressed (``dev_row_order``)."""

    def __init__(self, shape, indices, entries, _dev=None, _order=None) -> None:
        self.shape = tuple(int(n) for n in shape)
        if isinstance(indices, tuple):
            indices = np.stack(indices)
        self.indices = indices
        self.entries = entries
        self._dev = _dev
        self._order = tuple(range(len(self.shape))) if _order is None else tuple(_order)

    def _upload(self):
        if self._dev is None:
            idx = np.ascontiguousarray(np.asarray(self.indices), dtype=np.int64)
            # the device kernels address cores, Psi slices and sample tables by these values: out of range
            # is a memory fault there, so it is an error here (the reference would raise IndexError in its slicing)
            if idx.size and (idx.min() < 0 or (idx.max(axis=1) >= np.asarray(self.shape, dtype=np.int64)).any()):
                raise IndexError(f"SparseTensor: an index lies outside the shape {self.shape}")
            # rows are stored in the order of the *first* upload; later views permute
            inv = np.argsort(self._order)
            self._dev = (DevArray.from_host(idx[inv], dtype=np.int64),
                         DevArray.from_host(np.asarray(self.entries, dtype=np.float64)), {})
        return self._dev

    def prepare_device(self) -> None:
        self._upload()

    def dev_indices(self) -> DevArray:
        """(d, nnz) int64 buffer; logical row i lives at physical row dev_row_order[i]."""
        return self._upload()[0]

    def dev_entries(self) -> DevArray:
        return self._upload()[1]

    def dev_mode_perm(self, mu: int) -> DevArray:
        """Permutation that visits the nonzeros in order of their (logical) mode-``mu`` index; sorted
        once per tensor and mode on the device and shared with ``.T`` views."""
        from . import _native as nat
        idx = self._upload()[0]
        phys = self._order[mu]
        cache = self._dev[2]
        if phys not in cache:
            perm = DevArray.empty((self.nnz,), dtype=np.int64)
            nat.call("ttsk_sparse_sort_mode", idx[phys], self.nnz, int(self.shape[mu]), perm, 0)
            cache[phys] = perm
        return cache[phys]

    @property
    def dev_row_order(self) -> Tuple[int, ...]:
        return self._order

    @property
    def T(self) -> "SparseTensor":
        return SparseTensor(self.shape[::-1], self.indices[::-1], self.entries, self._dev,
                            self._order[::-1])

    @property
    def size(self) -> int:
        return self.nnz * (self.ndim + 1)

    @property
    def nnz(self) -> int:
        return len(self.entries)

    def split(self, n_summands: int) -> "TensorSum":
        """Contiguous nnz shards as a TensorSum (reference tensor.py:215-234)."""
        step = self.nnz // n_summands
        parts: List[Tensor] = []
        for i in range(n_summands):
            hi = (i + 1) * step if i < n_summands - 1 else self.nnz
            sl = slice(i * step, hi)
            parts.append(SparseTensor(self.shape, tuple(row[sl] for row in self.indices),
                                      self.entries[sl]))
        return TensorSum(parts)

    def to_numpy(self):
        X = np.zeros(self.shape)
        X[tuple(self.indices)] = self.entries
        return X

    def norm(self) -> float:
        return float(np.linalg.norm(self.entries))

    def dot(self, other, reverse=False, route: Optional[str] = None) -> float:
        """``<self, other>``.  ``route`` is the switch of ``paths.py`` for the lookup in another explicit tensor: the
        sorted-key join on the device, or the host path (``"composed"``: the dict of the reference)."""
        if isinstance(other, (_CoreList, TuckerTensor)) and (other.resident() or self._dev is not None):
            from .tensor_gather import _gather_device
            tucker_route = (route,) if isinstance(other, TuckerTensor) else ()
            return float(_gather_device(other, self, False, True, *tucker_route)[1][0])      # one pass, no (N,) vector
        if (isinstance(other, SparseTensor) and (self._dev is not None or other._dev is not None)) or \
                (isinstance(other, DenseTensor) and (self._dev is not None or _dense_current(other))):
            from .tensor_sparse import _join_dot
            got = _join_dot(self, other, route)        # self as the queries: one join pass, nothing downloaded
            if got is not None:
                return got
        if hasattr(other, "gather"):
            return float(np.dot(other.gather(self.indices), self.entries))
        return super().dot(other, reverse=reverse)

    @classmethod
    def random(cls, shape, nnz: int, seed: Optional[int] = None) -> "SparseTensor":
        rng = np.random.default_rng(seed)
        flat = rng.choice(int(np.prod(shape)), size=nnz, replace=False)
        return cls(shape, np.stack(np.unravel_index(flat, shape)), rng.standard_normal(nnz))

    def __mul__(self, other: float) -> "SparseTensor":
        return SparseTensor(self.shape, self.indices, self.entries * other)

    def gather_dev(self, idx) -> DevArray:
        """Entries at the given multi-indices as a device array (N,), 0.0 where the tensor has none (of a repeated
        index its last entry): ``idx`` is a ``SparseTensor`` of this shape, a ``(d, N)`` array or a tuple of ``d``
        arrays.  One pass of the sorted-key join (``ttsk_sparse_join``)."""
        from .tensor_sparse import _sparse_join
        return _sparse_join(self, idx, True, False)[0]

    def gather(self, indices, route: Optional[str] = None) -> npt.NDArray[np.float64]:
        """Entries at the given multi-indices (reference tensor.py:275-286).  For an uploaded tensor one device pass and
        one download of the result where the rule of ``tensor_sparse`` (or ``route``, as in ``dot``) takes it; host
        otherwise, and for shapes the device entry refuses."""
        if self._dev is not None:
            from ._native import TtskUnsupported
            from .paths import resolve
            from .tensor_sparse import _join_routed
            if _join_routed(self, len(indices[0]), route):
                try:
                    return self.gather_dev(indices).get()
                except TtskUnsupported:
                    if resolve(route) == "kernel":
                        raise
        keys = np.ravel_multi_index(tuple(indices), self.shape)
        table = self.dict
        return np.array([table.get(int(k), 0.0) for k in keys])

    @cached_property
    def dict(self) -> Dict[int, float]:
        keys = np.ravel_multi_index(tuple(self.indices), self.shape)
        return {int(k): float(v) for k, v in zip(keys, self.entries)}

    def __repr__(self) -> str:
        return (f"<Sparse tensor of shape {self.shape} with {self.nnz} non-zero"
                f" entries at {hex(id(self))}>")


# --------------------------------------------------------------------------- TT
class TensorTrain(_CoreList, Tensor):
    """Tensor train with cores ``(r_{k-1}, n_k, r_k)`` (reference tensor.py:294-609)."""

    def __init__(self, cores: ArrayList, _dev=None) -> None:
        self._set_cores(cores, _dev)
        self.shape = tuple(int(C.shape[1]) for C in cores)
        self.rank = tuple(int(C.shape[0]) for C in cores[1:])

    @property
    def T(self) -> "TensorTrain":
        flip = (2, 1, 0)
        cores = [c.transpose(flip) if isinstance(c, DevArray) else np.transpose(c, flip)
                 for c in self.cores[::-1]]
        dev = self._dev_current()
        return TensorTrain(cores, None if dev is None else [c.transpose(flip) for c in dev[::-1]])

    def to_numpy(self):
        acc = _host(self.cores[0])
        acc = acc.reshape(acc.shape[1:])
        for C in self.cores[1:]:
            acc = np.tensordot(acc, _host(C), axes=(acc.ndim - 1, 0))
        return acc.reshape(acc.shape[:-1])

    @classmethod
    def random(cls, shape, rank: TTRank, seed: Optional[int] = None, orthog: bool = False,
               trim: Optional[bool] = None, norm_goal: str = "norm-1") -> "TensorTrain":
        """Gaussian cores; ``norm-1`` scales by 1/sqrt(r1*n), ``norm-preserve`` by 1/sqrt(r1)
        (reference tensor.py:323-378).  Uses a single NumPy Generator stream per core."""
        if trim is None:
            trim = bool(orthog)
        if orthog and not trim:
            raise ValueError("Trimming must be enabled if orthogonalization is enabled.")
        rk = (1,) + tuple(process_tt_rank(rank, shape, trim=trim)) + (1,)
        seeds = np.random.SeedSequence(seed).generate_state(len(shape))
        cores = []
        for k, n in enumerate(shape):
            r1, r2 = rk[k], rk[k + 1]
            M = np.random.default_rng(seeds[k]).standard_normal((r1 * n, r2))
            if orthog and k < len(shape) - 1:
                M, _ = np.linalg.qr(M, mode="reduced")
            elif norm_goal == "norm-1":
                M /= np.sqrt(r1 * n)
            elif norm_goal == "norm-preserve":
                M /= np.sqrt(r1)
            else:
                raise ValueError(f"Unknown norm goal: {norm_goal}")
            cores.append(M.reshape(r1, n, r2))
        return cls(cores)

    @classmethod
    def zero(cls, shape, rank: TTRank) -> "TensorTrain":
        rk = (1,) + process_tt_rank(rank, shape, trim=False) + (1,)
        return cls([np.zeros((rk[k], n, rk[k + 1])) for k, n in enumerate(shape)])

    def partial_dense(self, dir: str = "lr") -> ArrayList:
        """Dense partial products X_0...X_mu as matrices (reference tensor.py:390-406)."""
        cs = [_host(c) for c in self.cores]
        if dir == "lr":
            out = [cs[0].reshape(-1, cs[0].shape[-1])]
            for c in cs[1:-1]:
                nxt = np.tensordot(out[-1], c, axes=(1, 0))
                out.append(nxt.reshape(-1, nxt.shape[-1]))
        elif dir == "rl":
            out = [cs[-1].reshape(cs[-1].shape[0], -1)]
            for c in cs[-2:0:-1]:
                nxt = np.tensordot(c, out[-1], axes=(2, 0))
                out.append(nxt.reshape(nxt.shape[0], -1))
        else:
            raise ValueError(dir)
        return out

    def gather(self, idx) -> npt.NDArray:
        """Entries at the given multi-indices (rows of ``idx`` are modes).  On the device (``gather_dev``) for a
        resident train or a ``SparseTensor`` of indices; host NumPy otherwise."""
        if self.resident() or isinstance(idx, SparseTensor):
            return self.gather_dev(idx).get()
        idx = np.stack(idx) if not isinstance(idx, np.ndarray) else idx
        cs = [_host(c) for c in self.cores]
        acc = cs[0][0][idx[0]]                       # (N, r1)
        for k in range(1, self.ndim):
            sl = cs[k][:, idx[k], :]                 # (r, N, r')
            acc = np.einsum("nr,rns->ns", acc, sl)
        return acc.reshape(-1)

    def dense_stats(self, X) -> npt.NDArray[np.float64]:
        """``[sum x t, sum t^2, sum (t - x)^2, sum x^2]`` over all entries of the dense tensor ``X`` (a ``DenseTensor`` or
        an ndarray of this shape) in one device pass that reconstructs the train tile by tile and stores nothing
        (``ttsk_tt_dense_stats``).  The same bits on every call."""
        from .tensor_dense import _dense_operand, _tt_dense_pass
        arr, transposed = _dense_operand(X, self.shape)
        return _tt_dense_pass(self.T if transposed else self, arr, False, True)[1]

    def to_dense_dev(self) -> "DenseTensor":
        """The full tensor as a ``DenseTensor`` whose data stay on the device (the same kernel, storing its tiles)."""
        from .tensor_dense import _tt_dense_pass
        return DenseTensor(_tt_dense_pass(self, None, True, False)[0])

    def dense(self) -> "DenseTensor":
        return self.to_dense_dev() if self.resident() else super().dense()

    def orthogonalize(self) -> "TensorTrain":
        """Left-orthogonalising QR sweep (reference tensor.py:559-572)."""
        out, carry = [], None
        for k, C in enumerate(self.cores):
            C = _host(C)
            if carry is not None:
                C = np.tensordot(carry, C, axes=(1, 0))
            if k < self.ndim - 1:
                Q, carry = np.linalg.qr(C.reshape(-1, C.shape[2]))
                out.append(Q.reshape(C.shape[0], C.shape[1], -1))
            else:
                out.append(C)
        return TensorTrain(out)

    def norm(self) -> float:
        if self.resident():
            return float(np.linalg.norm(self.orthogonalize_dev().cores[-1].get()))
        return float(np.linalg.norm(self.orthogonalize().cores[-1]))

    def gram_norm(self) -> float:
        """sqrt(<x, x>) by the Gram chain (``tt_gram``: one device pass, no QR sweep).  Accurate to a few ulp
        for a train that is not itself a difference of nearly equal terms -- a direct sum ``a + (-b)`` with
        a ~ b cancels inside the chain and is only good to sqrt(eps) ||a||; ``norm`` (QR sweep, reference
        tensor.py:442-444) has no such limit.  That is why ``error(fast=False)`` keeps the QR sweep of the direct
        sum, and only ``fast=True`` -- whose formula has that floor by definition -- takes the Gram pass."""
        return float(np.sqrt(max(self.dot(self), 0.0)))

    def to_device(self) -> "TensorTrain":
        """The same train with device-resident cores (uploads host cores once)."""
        return self if self.resident() else TensorTrain(list(self.dev_cores()))

    # ---- device versions (the step after to_tt) -------------------------
    def orthogonalize_dev(self) -> "TensorTrain":
        """Left-orthogonalising QR sweep on the device: thin QR by ``ttsk_qr_thin`` (CholeskyQR2
        with LAPACK's signs, Householder fallback), R recovered as Q^T M by the long-K kernel.
        Same result as ``orthogonalize`` (reference tensor.py:559-572) up to rounding."""
        from . import _native as nat
        from .device import contract
        cores = self.dev_cores()
        out, carry = [], None
        for k, C in enumerate(cores):
            if carry is not None:
                C = contract("ij,jkl->ikl", carry, C)
            if k < self.ndim - 1:
                r1, n, r2 = C.shape
                M = C.contiguous().reshape(r1 * n, r2)
                m = r1 * n
                # wide unfolding (m < r2): Q (m x m) from the leading square block, R = Q^T M is m x r2
                Q = M.copy() if m >= r2 else M[:, :m].contiguous()
                q = min(m, r2)
                nat.call("ttsk_qr_thin", Q, m, q, 0)
                carry = contract("ai,aj->ij", Q, M)
                nat.call("ttsk_triu", carry, q, r2, 0)
                out.append(Q.reshape(r1, n, q))
            else:
                out.append(C.contiguous())
        return TensorTrain(out)

    def round_dev(self, eps: Optional[float] = None, max_rank: Optional[TTRank] = None,
                  orthogonalized: bool = False) -> "TensorTrain":
        """TT-SVD rounding on the device, the algorithm of ``round`` (reference tensor.py:446-484):
        the SVD of each wide unfolding M (r x n r') goes through the thin QR of M^T and a Jacobi SVD
        of the r x r factor (``ttsk_svd_small``).  Cores stay on the device; they equal ``round``'s
        up to the sign gauge of the singular vectors (the represented tensor is the same)."""
        from . import _native as nat
        tt = self if orthogonalized else self.orthogonalize_dev()
        eps = 0 if eps is None else eps
        cap = process_tt_rank(tt.rank if max_rank is None else max_rank, tt.shape, trim=True)
        cores = tt.dev_cores()
        out, carry = [], None
        for k in range(tt.ndim - 1, -1, -1):
            C = cores[k]
            if carry is not None:
                C = contract("ijk,kl->ijl", C, carry)
            if k == 0:
                out.append(C)
                continue
            r1, n, r2 = C.shape
            C = C.contiguous()
            k2 = n * r2
            if k2 < r1:
                # tall unfolding M (r1 x k2): one-sided Jacobi over the ROWS of M (columns of M^T padded
                # to r1 x r1), so rows that are exactly zero -- a zero summand -- give exactly zero
                # singular values as they do in LAPACK.  M^T = US Vt  =>  M = Vt^T diag(S) (US/S)^T.
                A = DevArray.zeros((r1, r1))
                copy_into(A[:k2], C.reshape(r1, k2).T)
                Qc = None
            else:
                Mt = C.reshape(r1, k2).T.contiguous()                # (n r2, r1), tall
                Qc = Mt.copy()
                nat.call("ttsk_qr_thin", Qc, k2, r1, 0)
                Rc = contract("ai,aj->ij", Qc, Mt)                   # (r1, r1) upper triangular
                nat.call("ttsk_triu", Rc, r1, r1, 0)
                A = Rc.T.contiguous()                                # M = Rc^T Qc^T
            if r1 > 1024:
                raise ValueError(f"round_dev: TT rank {r1} > 1024 is beyond the one-workgroup SVD; use round()")
            US, S, Vt = DevArray.empty((r1, r1)), DevArray.empty((r1,)), DevArray.empty((r1, r1))
            nat.call("ttsk_svd_small", A, r1, r1, US, S, Vt, 0)
            sv = S.get()
            r = max(1, min(int(np.sum(sv > sv[0] * eps)), cap[k - 1], k2))
            if Qc is None:
                eye = DevArray.from_host(np.eye(r))
                inv = np.divide(1.0, sv[:r], out=np.zeros(r), where=sv[:r] > 0)
                carry = contract("ka,kb->ab", Vt[:r], eye, k_scale=S[:r].contiguous())
                V = contract("ka,ck->ac", eye, US[:k2, :r], k_scale=DevArray.from_host(inv))
            else:
                carry = US[:, :r]
                V = contract("ab,cb->ac", Vt[:r], Qc)
            out.append(V.reshape(r, n, r2))
        return TensorTrain(out[::-1])

    def round_gram(self, eps: Optional[float] = None, max_rank: Optional[TTRank] = None) -> "TensorTrain":
        """Gram-SVD rounding on the device: the rank rule and the arguments of ``round``, all bonds
        truncated at once from the Gram matrices of the left and right parts (``ttsk_gram_round_bonds``) instead of by
        two sweeps.  Takes a resident train or host cores (uploaded once); the result is resident; one read-back, the
        ``d - 1`` chosen ranks.  The same bits on every call.

        The price is the floor of every Gram method (``gram_norm``, ``error(fast=True)``): singular values below about
        ``sqrt(eps_machine)`` of the largest are not resolved, so a term of relative size 1e-10 is lost where ``round`` keeps
        it: ``x.add(y * 1e-10)`` rounded at ``eps=1e-12`` comes back at the ranks of ``x`` with a relative error of 9.6e-11
        against the input, the dropped term (``tests/test_gpu_gram_round.py``), where ``round`` keeps every rank at 2e-15.
        Above the floor the ranks are those of ``round``; the error is within 0.6 % of its error on the test cases and, as
        every bond is cut from the untruncated train, a few percent above it where a flat spectrum is cut hard (DESIGN
        section 18).  Bond ranks up to 1024, as ``round_dev``, which stays the exact method."""
        from .tensor_round import round_gram
        return round_gram(self, eps, max_rank)

    def svdvals_gram(self) -> List[npt.NDArray]:
        """The singular values of the unfoldings at the ``d - 1`` bonds (entry ``b - 1``: bond ``b``, what ``svdvals()[b]``
        holds) from the bond solve of ``round_gram`` with no truncation, on the device.  Values below about
        ``sqrt(eps_machine)`` of the largest of a bond are not resolved: they come back as noise of that size or as zeros."""
        from .tensor_round import svdvals_gram
        return svdvals_gram(self)

    def round(self, eps: Optional[float] = None, max_rank: Optional[TTRank] = None,
              orthogonalized: bool = False) -> "TensorTrain":
        """TT-SVD rounding (reference tensor.py:446-484); host LAPACK (``round_dev`` is the device
        version)."""
        tt = self if orthogonalized else self.orthogonalize()
        eps = 0 if eps is None else eps
        cap = process_tt_rank(tt.rank if max_rank is None else max_rank, tt.shape, trim=True)
        out, carry = [], None
        for k in range(tt.ndim - 1, -1, -1):
            C = _host(tt.cores[k])
            if carry is not None:
                C = np.tensordot(C, carry, axes=(2, 0))
            if k > 0:
                U, S, Vt = np.linalg.svd(C.reshape(C.shape[0], -1))
                r = max(1, min(int(np.sum(S > S[0] * eps)), cap[k - 1]))
                carry = U[:, :r] * S[:r]
                out.append(Vt[:r].reshape(r, C.shape[1], C.shape[2]))
            else:
                out.append(C)
        return TensorTrain(out[::-1])

    def svdvals(self) -> List[npt.NDArray]:
        tt = self.orthogonalize()
        vals, carry = [], None
        for k in range(tt.ndim - 1, -1, -1):
            C = tt.cores[k]
            if carry is not None:
                C = np.tensordot(C, carry, axes=(2, 0))
            M = C.reshape(C.shape[0], -1) if k > 0 else C.reshape(-1, C.shape[2])
            U, S, _ = np.linalg.svd(M)
            carry = U * S[:U.shape[1]] if k > 0 else None
            vals.append(S)
        return vals[::-1]

    def __mul__(self, other: float) -> "TensorTrain":
        if self.resident():
            last = self.cores[-1].copy()
            axpby(last, last, float(other), 0.0)
            return TensorTrain(list(self.cores[:-1]) + [last])
        cores = [np.array(_host(c)) for c in self.cores]
        cores[-1] = cores[-1] * other
        return TensorTrain(cores)

    __rmul__ = __mul__

    def hadamard(self, other: "TensorTrain"):
        """The entrywise product ``self o other`` as a tensor that keeps its two factors (``HadamardProduct``, ``self``
        the outer one): the sketches take it without forming its Kronecker cores."""
        from .hadamard_product import HadamardProduct
        return HadamardProduct(self, other)

    @property
    def size(self) -> int:
        return int(sum(c.size for c in self.cores))

    def add(self, other: "TensorTrain") -> "TensorTrain":
        """Direct-sum addition of two TTs (reference tensor.py:503-525)."""
        if self.resident() and other.resident():
            out, d = [], self.ndim
            for k, (a, b) in enumerate(zip(self.cores, other.cores)):
                ra1, n, ra2 = a.shape
                rb1, _, rb2 = b.shape
                r1 = 1 if k == 0 else ra1 + rb1
                r2 = 1 if k == d - 1 else ra2 + rb2
                blk = DevArray.zeros((r1, n, r2))
                copy_into(blk[:ra1, :, :ra2], a)
                copy_into(blk[r1 - rb1:, :, r2 - rb2:], b)
                out.append(blk)
            return TensorTrain(out)
        A = [_host(c) for c in self.cores]
        B = [_host(c) for c in other.cores]
        out = [np.concatenate((A[0], B[0]), axis=2)]
        for a, b in zip(A[1:-1], B[1:-1]):
            blk = np.zeros((a.shape[0] + b.shape[0], a.shape[1], a.shape[2] + b.shape[2]))
            blk[:a.shape[0], :, :a.shape[2]] = a
            blk[a.shape[0]:, :, a.shape[2]:] = b
            out.append(blk)
        out.append(np.concatenate((A[-1], B[-1]), axis=0))
        return TensorTrain(out)

    def dot(self, other, reverse=False, route: Optional[str] = None) -> float:
        """``<self, other>``.  ``route`` is the switch of ``paths.py`` for the one path here that has a kernel and a
        composition per step, the chain against a ``CPTensor`` (``_tt_cp_dot``)."""
        if isinstance(other, TensorTrain) and self.resident() and other.resident():
            from .tensor_gram import tt_gram
            return float(tt_gram([self], [other])[0, 0])        # one device call, or the chain where tt_gram routes it
        if isinstance(other, CPTensor) and (_on_device(self) or _on_device(other)):
            from .tensor_gram import _tt_cp_dot
            return _tt_cp_dot(self, other, route)
        if isinstance(other, TensorTrain):
            acc = np.ones((1, 1))
            for a, b in zip(self.cores, other.cores):
                acc = np.einsum("ij,ika,jkb->ab", acc, _host(a), _host(b), optimize=True)
            return float(acc.sum())
        if isinstance(other, DenseTensor) and (self.resident() or _dense_current(other)):
            return float(self.dense_stats(other)[0])
        if isinstance(other, TuckerTensor) and (_on_device(self) or _on_device(other)):
            from .tensor_tucker import tucker_tt_dot
            return tucker_tt_dot(other, self)
        return super().dot(other, reverse=reverse)

    def error(self, other, relative: bool = False, rmse: bool = False, fast: bool = False) -> float:
        """``||self - other||`` (reference tensor.py:53-88).  Against a dense tensor with either side on the device all
        of it comes from the four sums of one pass (``dense_stats``): the residual is ``sqrt(sum (t - x)^2)``, the
        reference norm ``sqrt(sum x^2)``, and ``fast`` puts ``sum x t``, ``sum t^2`` and ``sum x^2`` into the reference's
        formula.  A host train with a host array keeps the NumPy path.

        Against a ``CPTensor`` (or a ``TensorSum`` that holds one) ``fast=True`` is the reference's formula on
        ``self.norm()``, ``other.norm()`` and ``self.dot(other)``, which stay on the device when either side is there
        (``cp_gram``, ``_tt_cp_dot``) and form no dense array; that formula has the reference's floor of about 1e-8
        relative.  ``fast=False`` against CP keeps the reference's dense formula.

        Against a ``HadamardProduct`` ``fast=True`` is the same formula on three chains over the factors' cores
        (``hadamard_gram``): the product's Kronecker cores are not formed.  The same against an ``OperatorProduct``
        (``operator_gram``); ``fast=False`` forms ``mpo(tt)`` as before."""
        from .hadamard_product import HadamardProduct
        from .operator_product import OperatorProduct
        if fast and isinstance(other, (HadamardProduct, OperatorProduct)):
            aa, ab, bb = self.dot(self), other.dot(self), other.dot(other)
            err = float(_fast_error(aa, ab, bb)) if aa + bb > 0 else 0.0
            return float(_error_tail(err, float(np.sqrt(abs(bb))), self.shape, relative, rmse))    # sqrt|bb| is other.norm()
        if hasattr(other, "to_tt"):
            other = other.to_tt()
        dense = DenseTensor(other) if isinstance(other, np.ndarray) else other
        if isinstance(dense, DenseTensor) and (self.resident() or _dense_current(dense)):
            s = self.dense_stats(dense)
            ref_norm = float(np.sqrt(s[3]))
            err = _fast_error(s[1], s[0], s[3]) if fast else np.sqrt(s[2])
            return float(_error_tail(err, ref_norm, self.shape, relative, rmse))
        if isinstance(other, TensorTrain) and fast and self.resident() and other.resident():
            # <a, a>, <a, b>, <b, b> from one 2 x 2 Gram in the reference's formula
            from .tensor_gram import tt_gram
            G = tt_gram([self, other])
            err = float(_fast_error(G[0, 0], G[0, 1], G[1, 1])) if G[0, 0] + G[1, 1] > 0 else 0.0
            ref_norm = float(np.sqrt(abs(G[1, 1])))
            return float(_error_tail(err, ref_norm, self.shape, relative, rmse))
        if isinstance(other, TensorTrain):
            err = self.add(-other).norm()
            return _error_tail(err, other.norm() if relative else None, self.shape, relative, rmse)   # the sweep only if asked
        return super().error(other, relative=relative, rmse=rmse, fast=fast)

    def __repr__(self) -> str:
        return f"<Tensor train of shape {self.shape} with rank {self.rank} at {hex(id(self))}>"


# --------------------------------------------------------------------------- sums
class TensorSum(Tensor):
    """Lazy sum of tensors of one shape (reference tensor.py:612-671)."""

    def __init__(self, tensors: List[Tensor], shape=None) -> None:
        self.tensors = tensors
        self.shape = tuple(tensors[0].shape) if shape is None else tuple(shape)

    @property
    def size(self) -> int:
        return sum(t.size for t in self.tensors)

    @property
    def T(self) -> "TensorSum":
        return TensorSum([t.T for t in self.tensors])

    def to_numpy(self):
        acc = np.zeros(self.shape)
        for t in self.tensors:
            acc += t.to_numpy()
        return acc

    def __add__(self, other) -> "TensorSum":
        extra = other.tensors if isinstance(other, TensorSum) else [other]
        return TensorSum(self.tensors + list(extra))

    def __iadd__(self, other) -> "TensorSum":
        if isinstance(other, TensorSum):
            self.tensors.extend(other.tensors)
        else:
            self.tensors.append(other)
        return self

    def prepare_device(self) -> None:
        for t in self.tensors:
            t.prepare_device()

    @property
    def num_summands(self) -> int:
        return len(self.tensors)

    def __mul__(self, other: Union[float, Iterable[float]]) -> "TensorSum":
        try:
            coeffs = list(other)  # type: ignore[arg-type]
        except TypeError:
            return TensorSum([t * other for t in self.tensors])
        if len(coeffs) != len(self.tensors):
            raise ValueError("one coefficient per summand expected")
        return TensorSum([t * c for t, c in zip(self.tensors, coeffs)])

    def dot(self, other, reverse=False) -> float:
        return sum(t.dot(other, reverse) for t in self.tensors)

    def __repr__(self) -> str:
        return f"<Sum of {self.num_summands} tensors of shape {self.shape} at {hex(id(self))}>"


# --------------------------------------------------------------------------- CP
class CPTensor(_CoreList, Tensor):
    """CP format, factor matrices ``(n_k, R)`` (reference tensor.py:674-743).

    ``dot`` / ``norm`` against another ``CPTensor`` or a ``TensorTrain`` run on the device when either operand is there
    (``resident()`` or uploaded already) and form no dense array; with them ``error(fast=True)`` -- the reference's
    formula, whose floor is a relative error of about 1e-8 -- does not either.  Two host objects keep the NumPy path,
    and ``fast=False`` keeps the reference's dense formula."""

    def __init__(self, cores: ArrayList, _dev=None) -> None:
        self._set_cores(cores, _dev)
        self.rank = int(cores[0].shape[1])
        self.shape = tuple(int(C.shape[0]) for C in cores)

    @property
    def size(self) -> int:
        return int(sum(C.size for C in self.cores))

    @property
    def T(self) -> "CPTensor":
        dev = self._dev_current()
        return CPTensor(self.cores[::-1], None if dev is None else dev[::-1])

    def to_numpy(self):
        acc = _host(self.cores[0])
        for C in self.cores[1:]:
            acc = acc[..., None, :] * _host(C)
        return acc.sum(axis=-1)

    @classmethod
    def random(cls, shape, rank: int, seed: Optional[int] = None) -> "CPTensor":
        seeds = np.random.SeedSequence(seed).generate_state(len(shape))
        return cls([np.random.default_rng(s).standard_normal((n, rank)) / np.sqrt(n)
                    for s, n in zip(seeds, shape)])

    def gather(self, idx) -> npt.NDArray:
        """Entries at the given multi-indices; on the device (``gather_dev``) for device factors or a ``SparseTensor``
        of indices, host NumPy otherwise."""
        if self.resident() or isinstance(idx, SparseTensor):
            return self.gather_dev(idx).get()
        acc = 1.0
        for C, rows in zip(self.cores, idx):
            acc = acc * _host(C)[rows]
        return np.sum(acc, axis=1)

    def norm(self) -> float:
        if _on_device(self):
            from .tensor_gram import cp_gram
            return float(np.sqrt(abs(cp_gram(self))))
        return super().norm()

    def dot(self, other, reverse=False, route: Optional[str] = None) -> float:
        """``route``: the switch of ``paths.py`` for the chain against a ``TensorTrain`` (``_tt_cp_dot``)."""
        if isinstance(other, CPTensor) and (_on_device(self) or _on_device(other)):
            from .tensor_gram import cp_gram
            return cp_gram(self, other)
        if isinstance(other, TensorTrain) and (_on_device(self) or _on_device(other)):
            from .tensor_gram import _tt_cp_dot
            return _tt_cp_dot(other, self, route)
        if isinstance(other, TuckerTensor) and (_on_device(self) or _on_device(other)):
            from .tensor_tucker import tucker_cp_dot
            return tucker_cp_dot(other, self)
        return super().dot(other, reverse=reverse)

    def __mul__(self, other: float) -> "CPTensor":
        cores = list(self.cores)
        cores[0] = _host(cores[0]) * other
        return CPTensor(cores)

    def __repr__(self) -> str:
        return f"<CP tensor of shape {self.shape} and rank {self.rank} at {hex(id(self))}>"


# --------------------------------------------------------------------------- Tucker
class TuckerTensor(Tensor):
    """Tucker format: core ``(s_1..s_d)`` and factors ``(s_k, n_k)`` (reference tensor.py:746-816).

    ``gather`` / ``gather_dev`` / ``support_error`` and ``SparseTensor.dot`` evaluate the tensor at index lists in one
    device pass (``ttsk_tucker_gather``: the core against the Khatri-Rao rows of the factor columns on the fp64 matrix
    instructions; ``tensor_gather``), with a composition from column gathers and batched ``contract`` calls beyond the
    kernel's cover (``route=`` is the switch of ``paths.py``).  ``dot`` / ``norm`` against a ``TuckerTensor``, a
    ``TensorTrain`` or a ``CPTensor`` run on the device when either operand is there (``resident()`` or uploaded already;
    ``tensor_tucker``) and form no dense array, so ``error(fast=True)`` -- the reference's formula, whose floor is a
    relative error of about 1e-8 -- does not either.  Two host objects keep the NumPy path, ``fast=False`` the reference's
    dense formula, and a ``DenseTensor`` partner its current path."""

    def __init__(self, factors: ArrayList, core, _dev=None) -> None:
        self.core = core
        self.factors = factors
        self.shape = tuple(int(U.shape[1]) for U in factors)
        self.rank = tuple(int(U.shape[0]) for U in factors)
        self._dev = _dev
        self._core_c = None               # (device core it was made from, its contiguous copy): a .T view's core is strided

    def dev_parts(self) -> Tuple[List[DevArray], DevArray]:
        if self._dev is None:
            self._dev = ([as_dev(U) for U in self.factors], as_dev(self.core))
        return self._dev

    prepare_device = dev_parts

    def dev_core_contiguous(self) -> DevArray:
        """The device core in C order, as ``ttsk_tucker_gather`` reads it: the core itself, or for a strided view (``.T``)
        a copy made on the device once and kept."""
        core = self.dev_parts()[1]
        if core.is_contiguous():
            return core
        if self._core_c is None or self._core_c[0] is not core:
            self._core_c = (core, core.contiguous())
        return self._core_c[1]

    def resident(self) -> bool:
        """True if the core and all factors live in HBM only; arithmetic on such a tensor stays on the device."""
        return isinstance(self.core, DevArray) and all(isinstance(U, DevArray) for U in self.factors)

    def to_device(self) -> "TuckerTensor":
        """A resident copy: core and factors as device arrays (uploaded once, shared with this tensor's cache)."""
        factors, core = self.dev_parts()
        return TuckerTensor(list(factors), core, (factors, core))

    def gather_dev(self, idx, route: Optional[str] = None) -> DevArray:
        """Entries at the given multi-indices as a device array (N,): ``idx`` is a ``SparseTensor`` of this shape (its
        resident index matrix is used in place), a ``(d, N)`` array or a tuple of ``d`` arrays.  ``route``: the switch of
        ``paths.py`` between ``ttsk_tucker_gather`` and its composition."""
        from .tensor_gather import _gather_device
        return _gather_device(self, idx, True, False, route)[0]

    def gather(self, idx, route: Optional[str] = None) -> npt.NDArray:
        """Entries at the given multi-indices; on the device (``gather_dev``) for a resident tensor or a ``SparseTensor``
        of indices, otherwise on the host mode by mode over chunks of the list: no dense array is formed."""
        if self.resident() or isinstance(idx, SparseTensor):
            return self.gather_dev(idx, route).get()
        arr = np.stack(idx) if isinstance(idx, (tuple, list)) else np.asarray(idx)
        if arr.ndim != 2 or arr.shape[0] != self.ndim:
            raise ValueError(f"gather: {self.ndim} index rows expected, got an array of shape {arr.shape}")
        core, N = _host(self.core), arr.shape[1]
        out = np.empty(N)
        chunk = max(1, (1 << 22) // max(1, core.size // max(1, core.shape[0])))
        for lo in range(0, N, chunk):
            sl = arr[:, lo:lo + chunk]
            v = _host(self.factors[0])[:, sl[0]].T @ core.reshape(core.shape[0], -1)
            for k in range(1, self.ndim):
                v = np.einsum("esr,se->er", v.reshape(v.shape[0], core.shape[k], -1), _host(self.factors[k])[:, sl[k]])
            out[lo:lo + chunk] = v[:, 0]
        return out

    def support_error(self, sparse: "SparseTensor", relative: bool = False, route: Optional[str] = None) -> float:
        """``|| self[indices] - entries ||`` over all nonzeros of ``sparse`` in one device pass, as the method of
        ``TensorTrain`` / ``CPTensor``.  ``relative``: divided by ``||entries||``."""
        from .tensor_gather import _gather_device
        err = float(np.sqrt(_gather_device(self, sparse, False, True, route)[1][2]))
        return _error_tail(err, sparse.norm() if relative else None, None, relative, False)

    def norm(self) -> float:
        if _on_device(self):
            from .tensor_tucker import tucker_dot
            return float(np.sqrt(abs(tucker_dot(self, self))))
        return super().norm()

    def dot(self, other, reverse=False, route: Optional[str] = None) -> float:
        """``<self, other>``.  Against a ``SparseTensor`` the one pass of ``SparseTensor.dot`` (``route``: its switch);
        against a ``TuckerTensor``, a ``TensorTrain`` or a ``CPTensor`` with either operand on the device the products of
        ``tensor_tucker``."""
        if isinstance(other, SparseTensor) and (self.resident() or other._dev is not None):
            return other.dot(self, route=route)
        if isinstance(other, (TuckerTensor, TensorTrain, CPTensor)) and (_on_device(self) or _on_device(other)):
            from . import tensor_tucker as tk
            if isinstance(other, TuckerTensor):
                return tk.tucker_dot(self, other)
            return tk.tucker_tt_dot(self, other) if isinstance(other, TensorTrain) else tk.tucker_cp_dot(self, other)
        return super().dot(other, reverse=reverse)

    @property
    def T(self) -> "TuckerTensor":
        axes = tuple(reversed(range(len(self.shape))))
        dev = None if self._dev is None else (self._dev[0][::-1], self._dev[1].transpose(axes))
        core = self.core.transpose(axes) if isinstance(self.core, DevArray) else np.transpose(self.core, axes)
        return TuckerTensor(self.factors[::-1], core, dev)

    @property
    def size(self) -> int:
        return int(self.core.size + sum(U.size for U in self.factors))

    def to_numpy(self):
        acc = _host(self.core)
        for k, U in enumerate(self.factors):
            acc = np.moveaxis(np.tensordot(acc, _host(U), axes=(k, 0)), -1, k)
        return acc

    def __mul__(self, other: float) -> "TuckerTensor":
        if isinstance(self.core, DevArray):
            core = self.core.copy()
            axpby(core, core, float(other), 0.0)
            return TuckerTensor(self.factors, core)
        return TuckerTensor(self.factors, _host(self.core) * other)

    @classmethod
    def random(cls, shape, rank, seed: Optional[int] = None) -> "TuckerTensor":
        try:
            rk = tuple(rank)
        except TypeError:
            rk = (rank,) * len(shape)
        rk = tuple(min(r, n) for r, n in zip(rk, shape))
        seq = np.random.SeedSequence(seed)
        core = np.random.default_rng(seq.generate_state(1)[0]).standard_normal(rk)
        factors = []
        for r, n, s in zip(rk, shape, seq.generate_state(len(shape))):
            U = np.random.default_rng(s).standard_normal((r, n))
            factors.append(np.linalg.qr(U.T)[0].T)
        return cls(factors, core)

    def __repr__(self) -> str:
        return f"<Tucker tensor of shape {self.shape} and rank {self.rank} at {hex(id(self))}>"
