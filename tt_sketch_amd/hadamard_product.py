"""Entrywise products of two tensor trains that are never formed: ``HadamardProduct(x, y)`` is the tensor ``x o y`` kept as
its two factors.  Its core would be ``P[(beta a), i, (beta' a')] = X[beta, i, beta'] Y[a, i, a']``,
``(R r) x n x (R' r')``: the ranks multiply.  The sketch drivers reach the product through the plug-in tables of
``sketch_dispatch``: ``W_k = L_{k-1} o (X_k, Y_k)`` comes from ``hadamard_apply`` -- one ``ttsk_hadamard_apply`` call
(csrc/hadamard_apply.hip) or its composition from ``contract`` calls -- and the chain step, Psi and Omega are one
``contract`` each on ``W_k``.

The rank index of the product is ``(beta a)``, the rank of ``x`` major: the layout ``OperatorProduct`` has for the
diagonal operator of ``x`` applied to ``y``.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from . import _native as nat
from .device import DevArray, contract, copy_into
from .paths import resolve, taken
from .tensor import DenseTensor, Tensor, TensorSum, TensorTrain, _error_tail, _fast_error, _host

# The routing rule of DESIGN section 15, its constants measured on one MI355X (profiles/hadamard_sketch_bench.json, the
# four shapes of hadamard_apply alone): a ttsk_hadamard_apply call costs its floor or its flops at the kernel's rate,
# whichever is more; W composed from `contract` calls costs its four launches and its flops at the rate the composition
# reaches above them (T1 and W pass through HBM three times: that rate is a bandwidth, not the GEMM's peak).
_KERNEL_FLOOR_MS = 0.014     # one call at R = r = n = l = 20
_KERNEL_TFLOPS = 10.6        # at R = r = 32, n = 200, l = 50, where every tile but those of l is full (7.9 at R = 8, r = 64; 9.0 at R = r = 50)
_LAUNCH_MS = 0.0215          # a quarter of the composed W at R = r = n = l = 20
_COMPOSED_LAUNCHES = 4       # see `_composed`
_GEMM_TFLOPS = 15.2          # the composed W at R = r = 50, n = 200, l = 50 above its four launches


def route_ms(R: int, R1: int, r: int, r1: int, n: int, l: int) -> Tuple[float, float]:
    """(kernel, composed) milliseconds the rule expects for one ``hadamard_apply``"""
    flops = 2.0 * l * n * (R * r * r1 + R * R1 * r1)
    return (max(_KERNEL_FLOOR_MS, flops / (_KERNEL_TFLOPS * 1e9)),
            _COMPOSED_LAUNCHES * _LAUNCH_MS + flops / (_GEMM_TFLOPS * 1e9))


def _composed(L: DevArray, X: DevArray, Y: DevArray, stream: int) -> DevArray:
    """W from `contract` calls, T1 through HBM.  The mode index i is a batch index of both products and sits between l and
    (beta', a') in W, which the one batch dimension of the strided GEMM cannot write: the second product leaves
    (i, beta', l, a') and a strided copy puts l first.  For the first product to carry i as its batch, (beta, l) must be one
    index of L: a transposed copy of L, the smallest operand."""
    La = L.transpose(1, 0, 2).contiguous(stream)                        # (r, R, l)
    T1 = contract("abl,aic->iblc", La, Y, stream=stream)                # (n, R, l, r')
    Wt = contract("bik,iblc->iklc", X, T1, stream=stream)               # (n, R', l, r')
    n, R1, l, r1 = Wt.shape
    W = DevArray.empty((l, n, R1, r1), stream=stream)
    copy_into(W, Wt.transpose(2, 0, 1, 3), stream)
    return W.reshape(l, n, R1 * r1)


def hadamard_apply(L: DevArray, X: DevArray, Y: DevArray, stream: int = 0, route: Optional[str] = None) -> DevArray:
    """``W[l, i, beta' r' + a'] = sum_beta X[beta, i, beta'] sum_a L[beta, a, l] Y[a, i, a']``, ``(l, n, R' r')``: the chain
    ``L (R, r, l)`` carried through the product core of ``X (R, n, R')`` and ``Y (r, n, r')`` without that core.  The cores
    may be strided views.  ``route="kernel"`` is one ``ttsk_hadamard_apply`` call, ``"composed"`` the same from `contract`
    calls, None (or ``paths.forced``) what ``route_ms`` expects to be faster."""
    route = resolve(route)
    R, n, R1 = X.shape
    r, ny, r1 = Y.shape
    if ny != n:
        raise ValueError(f"cores {X.shape} and {Y.shape} differ in their mode size")
    if L.shape[:2] != (R, r):
        raise ValueError(f"chain of shape {L.shape}, expected {(R, r)} and the sketch rank")
    l = int(L.shape[2])
    if route is None:
        route = taken(route, *route_ms(R, R1, r, r1, n, l))
    L = L.contiguous(stream)
    if route == "composed":
        return _composed(L, X, Y, stream)
    W = DevArray.empty((l, n, R1 * r1), stream=stream)
    nat.call("ttsk_hadamard_apply", L, X, Y, nat.i64_array((R, R1, r, r1, n, l)), nat.i64_array(tuple(X.strides) + tuple(Y.strides)),
             W, R1 * r1, 0, stream)
    return W


class HadamardProduct(Tensor):
    """``x o y``, the entrywise product of two tensor trains of one shape, held as the two trains.

    ``x`` is the outer factor: the rank index is ``(beta a)`` with the rank ``beta`` of ``x`` major.  The cost of a sketch
    is not symmetric in the two: one step with chain length ``l`` costs ``2 l n (R r r' + R R' r')`` flops for ranks
    ``R, R'`` of ``x`` and ``r, r'`` of ``y``, so of two factors with different ranks the caller chooses which one is
    outer."""

    def __init__(self, x: TensorTrain, y: TensorTrain) -> None:
        if tuple(x.shape) != tuple(y.shape):
            raise ValueError(f"entrywise product of tensors of shapes {tuple(x.shape)} and {tuple(y.shape)}")
        self.x = x
        self.y = y
        self.shape = tuple(x.shape)
        self.rank = tuple(R * r for R, r in zip(x.rank, y.rank))

    def dev_parts(self) -> Tuple[List[DevArray], List[DevArray]]:
        """(cores of x, cores of y) in HBM, strided views as they are: nothing is copied for a transposed view"""
        return self.x.dev_cores(), self.y.dev_cores()

    def prepare_device(self) -> None:
        self.dev_parts()

    @property
    def size(self) -> int:
        return int(self.x.size + self.y.size)

    @property
    def T(self) -> "HadamardProduct":
        """The product with the order of its modes reversed: the product of the reversed factors, views of their cores."""
        return HadamardProduct(self.x.T, self.y.T)

    def to_tt(self) -> TensorTrain:
        """The explicit product with its Kronecker cores ``"bik,aic->baikc"``; on host cores in NumPy, on resident ones by
        `contract`: an outer product batched over the mode, formed mode-major (the one batch dimension of the strided GEMM)
        and copied into place."""
        cores = []
        if self.x.resident() or self.y.resident():
            for X, Y in zip(*self.dev_parts()):
                Q = contract("ibk,iac->ibkac", X.transpose(1, 0, 2).contiguous(), Y.transpose(1, 0, 2).contiguous())
                n, R, R1, r, r1 = Q.shape
                P = DevArray.empty((R, r, n, R1, r1))
                copy_into(P, Q.transpose(1, 3, 0, 2, 4))
                cores.append(P.reshape(R * r, n, R1 * r1))
            return TensorTrain(cores)
        for X, Y in zip(self.x.cores, self.y.cores):
            P = np.einsum("bik,aic->baikc", _host(X), _host(Y))
            cores.append(P.reshape(P.shape[0] * P.shape[1], P.shape[2], P.shape[3] * P.shape[4]))
        return TensorTrain(cores)

    def to_numpy(self):
        return self.to_tt().to_numpy()

    # -- inner products, norm and fast error on the factors alone (hadamard_gram.py)
    def dot(self, other, reverse=False, route: Optional[str] = None) -> float:
        """``<self, other>`` against a ``TensorTrain`` or another ``HadamardProduct`` by a chain over the factors' cores: no
        Kronecker core and no dense array is formed, on the device when a factor is there and in NumPy otherwise.  ``route`` is
        the switch of ``paths.py`` for the closing step against a product (``hadamard_gram.hadamard_close``).  Every other
        partner goes through the base class."""
        if isinstance(other, HadamardProduct):
            from .hadamard_gram import hadamard_dot
            return hadamard_dot(self, other, route)
        if isinstance(other, TensorTrain):
            from .hadamard_gram import hadamard_tt_dot
            return hadamard_tt_dot(self, other)
        return super().dot(other, reverse=reverse)

    def error(self, other, relative: bool = False, rmse: bool = False, fast: bool = False) -> float:
        """``||self - other||``.  ``fast=True`` is the reference's formula on ``<self, self>``, ``<self, other>`` and
        ``<other, other>``, which form nothing dense against trains and Hadamard products (or sums of them); it has that
        formula's floor of about 1e-8 relative.  ``fast=False`` keeps the dense difference of the base class."""
        if not fast:
            return super().error(other, relative=relative, rmse=rmse, fast=False)
        if isinstance(other, np.ndarray):
            other = DenseTensor(other)
        aa, ab, bb = self.dot(self), self.dot(other), other.dot(other)
        err = float(_fast_error(aa, ab, bb)) if aa + bb > 0 else 0.0
        return float(_error_tail(err, float(np.sqrt(abs(bb))), self.shape, relative, rmse))

    def gather(self, idx) -> np.ndarray:
        """Entries at the given multi-indices: those of the two factors, multiplied on the host."""
        return self.x.gather(idx) * self.y.gather(idx)

    def __mul__(self, other: float) -> "HadamardProduct":
        return HadamardProduct(self.x, self.y * other)

    def __repr__(self) -> str:
        return f"<Hadamard product of shape {self.shape} of tensor trains of ranks {tuple(self.x.rank)} and {tuple(self.y.rank)} at {hex(id(self))}>"


def hadamard_round(x: TensorTrain, y: TensorTrain, max_rank, eps: Optional[float] = None, method="sketch",
                   oversample_factor: float = 2) -> TensorTrain:
    """``x o y`` rounded to ``max_rank``: ``tt_gmres.round_tt_sum`` of the one-term sum.  The two sketched methods never
    form the product; ``"exact"``, ``"pairwise"``, ``"gram"`` and None form it first."""
    from .tt_gmres import round_tt_sum
    return round_tt_sum(TensorSum([HadamardProduct(x, y)]), max_rank, eps=eps, method=method, oversample_factor=oversample_factor)
