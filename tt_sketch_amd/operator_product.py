"""Operator-times-train products that are never formed: ``OperatorProduct(mpo, tt)`` is the tensor ``mpo(tt)`` kept as
its two factors.  The sketch drivers reach it through the plug-in tables of ``sketch_dispatch``:
``W_k = L_{k-1} o (M_k, C_k)`` comes from one ``ttsk_op_apply`` call (csrc/op_apply.hip), and the chain step, Psi and
Omega are one ``contract`` each on ``W_k`` -- ``l / (R r)`` of the product core ``MPO.__call__`` (reference
tt_gmres.py:90-101) would have built.

The rank index of the product is ``(beta a)``, operator rank major, as ``MPO.__call__`` lays it out.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _native as nat
from .device import DevArray, contract, copy_into
from .paths import resolve, taken
from .tensor import DenseTensor, Tensor, TensorTrain, _error_tail, _fast_error, _host

MAX_TERMS = 24          # OP_MAX_TERMS of csrc/op_apply_plan.h: the terms of one ttsk_op_apply call

# The routing rule of DESIGN section 13, its constants measured on one MI355X (profiles/operator_sketch_bench.json): a
# ttsk_op_apply call costs its floor or its flops at the kernel's rate, whichever is more, whatever the number of terms;
# W composed from `contract` calls (T1 through HBM) costs every term its launches and its flops at the GEMM's rate.
_KERNEL_FLOOR_MS = 0.090     # one call at K1
_KERNEL_TFLOPS = 3.2         # at K2
_LAUNCH_MS = 0.036           # one `contract` launch: half the composed W at K1
_GEMM_TFLOPS = 35.0          # the composed W at K2 above its two launches

_one: Optional[DevArray] = None


def route_ms(dims) -> Tuple[float, float]:
    """(kernel, composed) milliseconds the rule expects for terms ``(R, R', r, r', n_in, n_out, l, plain)``"""
    flops = [2.0 * l * (R * r * n_in * r1 + R * n_in * n_out * R1 * r1) for R, R1, r, r1, n_in, n_out, l, _ in dims]
    kernel = max(_KERNEL_FLOOR_MS, sum(flops) / (_KERNEL_TFLOPS * 1e9))
    launches = [(1 if plain else 2) + (len(dims) > 1) for *_, plain in dims]
    return kernel, sum(k * _LAUNCH_MS + f / (_GEMM_TFLOPS * 1e9) for k, f in zip(launches, flops))


def _composed(L: DevArray, M: Optional[DevArray], C: DevArray, stream: int) -> DevArray:
    """W of one term from `contract` calls, T1 through HBM"""
    if M is None:
        return contract("al,aic->lic", L[0], C, stream=stream)
    T1 = contract("bal,ajc->bljc", L, C, stream=stream)
    W = contract("bjik,bljc->likc", M, T1, stream=stream)
    return W.reshape(W.shape[0], W.shape[1], W.shape[2] * W.shape[3])


def chain_start() -> DevArray:
    """L_{-1} = 1 as the (R, r, l) = (1, 1, 1) array the first step starts from"""
    global _one
    if _one is None:
        _one = DevArray.from_host(np.ones((1, 1, 1)))
    return _one


def op_apply(Ls: Sequence[DevArray], Ms: Sequence[Optional[DevArray]], Cs: Sequence[DevArray], stream: int = 0,
             route: Optional[str] = None) -> Tuple[DevArray, List[int]]:
    """``W (l, n_out, sum_p R'_p r'_p)`` of the terms p and the column offset of each: term p holds
    ``W[l, i, off_p + beta' r' + a'] = sum_{beta, j} M_p[beta, j, i, beta'] sum_a L_p[beta, a, l] C_p[a, j, a']``.
    ``Ls[p]`` is ``(R, r, l)``, ``Ms[p]`` ``(R, n_in, n_out, R')`` or None for a plain train (``W = L o C``), ``Cs[p]``
    ``(r, n_in, r')``; operator and train cores may be strided views.  Lists longer than one call holds are cut.  Where
    the routing rule expects it to be faster, W is composed from `contract` calls term by term instead; ``route="kernel"``
    or ``"composed"`` (or ``paths.forced``) takes that route whatever the rule says."""
    route = resolve(route)
    dims, strides, offs, keep, off = [], [], [], [], 0
    l = int(Ls[0].shape[2])
    for L, M, C in zip(Ls, Ms, Cs):
        r, n_in, r1 = C.shape
        if M is None:
            R, R1, n_out, sm = 1, 1, n_in, (0, 0, 0, 0)
        else:
            R, mi, n_out, R1 = M.shape
            sm = M.strides
            if mi != n_in:
                raise ValueError(f"operator core {M.shape} does not act on a train core {C.shape}")
        if L.shape != (R, r, l):
            raise ValueError(f"chain of shape {L.shape}, expected {(R, r, l)}")
        keep.append(L.contiguous(stream))
        dims.append((R, R1, r, r1, n_in, n_out, off))
        strides.append(tuple(sm) + tuple(C.strides))
        offs.append(off)
        off += R1 * r1
    n_out = dims[0][5]
    if route is None:
        route = taken(route, *route_ms([d[:6] + (l, M is None) for d, M in zip(dims, Ms)]))
    if route == "composed":
        if len(dims) == 1:
            return _composed(keep[0], Ms[0], Cs[0], stream), offs
        W = DevArray.empty((l, n_out, off), stream=stream)
        for L, M, C, o, d in zip(keep, Ms, Cs, offs, dims):
            copy_into(W[:, :, o:o + d[1] * d[3]], _composed(L, M, C, stream), stream)
        return W, offs
    W = DevArray.empty((l, n_out, off), stream=stream)
    for a in range(0, len(dims), MAX_TERMS):
        b = min(a + MAX_TERMS, len(dims))
        nat.call("ttsk_op_apply", b - a, nat.ptr_array(keep[a:b]),
                 (nat.c_void_p * (b - a))(*[None if M is None else M.ptr for M in Ms[a:b]]), nat.ptr_array(Cs[a:b]),
                 nat.i64_array([x for row in dims[a:b] for x in row]), nat.i64_array([x for row in strides[a:b] for x in row]),
                 l, W, off, stream)
    return W, offs


class OperatorProduct(Tensor):
    """``mpo(tt)`` held as the operator and the train."""

    def __init__(self, mpo, tt: TensorTrain) -> None:
        if tuple(mpo.in_shape) != tuple(tt.shape):
            raise ValueError(f"MPO maps shape {mpo.in_shape}, got a tensor of shape {tt.shape}")
        self.mpo = mpo
        self.tt = tt
        self.shape = tuple(mpo.out_shape)
        self.rank = tuple(R * r for R, r in zip(mpo.rank, tt.rank))

    def dev_parts(self) -> Tuple[List[DevArray], List[DevArray]]:
        """(operator cores, train cores) in HBM, strided views as they are: nothing is copied for a transposed view.  The
        operator's cores are the MPO's own resident ones, uploaded once however many products are made of it."""
        return self.mpo.dev_views(), self.tt.dev_cores()

    def prepare_device(self) -> None:
        self.dev_parts()

    @property
    def size(self) -> int:
        return int(self.mpo.size + self.tt.size)

    @property
    def T(self) -> "OperatorProduct":
        """The product with the order of its modes reversed (not ``mpo.T``, the transpose of the linear map): operator
        cores ``M_{d-1-k}.transpose(3, 1, 2, 0)`` on the reversed train, views of the resident cores where there are any."""
        flip = (3, 1, 2, 0)
        src = self.mpo.dev_views() if self.mpo.resident() else self.mpo.cores
        cores = [c.transpose(flip) if isinstance(c, DevArray) else np.transpose(c, flip) for c in src[::-1]]
        return OperatorProduct(type(self.mpo)(cores), self.tt.T)

    def to_tt(self) -> TensorTrain:
        """The explicit product, ``mpo(tt)``; on host cores in NumPy."""
        if self.tt.resident() or any(isinstance(c, DevArray) for c in self.mpo.cores):
            return self.mpo(self.tt)
        cores = []
        for M, C in zip(self.mpo.cores, self.tt.cores):
            P = np.einsum("ijkl,ajb->iaklb", _host(M), _host(C))
            cores.append(P.reshape(P.shape[0] * P.shape[1], P.shape[2], P.shape[3] * P.shape[4]))
        return TensorTrain(cores)

    def to_numpy(self):
        return self.to_tt().to_numpy()

    # -- inner products, norm and fast error on the factors alone (operator_gram.py)
    def dot(self, other, reverse=False, route: Optional[str] = None) -> float:
        """``<self, other>`` against a ``TensorTrain`` or another ``OperatorProduct`` by a chain over the factors' cores: no
        product core and no dense array is formed, on the device when a factor is there and in NumPy otherwise.  ``route`` is
        the switch of ``paths.py`` for the closing step against a product (``operator_gram.op_close``).  Every other partner
        goes through the base class."""
        if isinstance(other, OperatorProduct):
            from .operator_gram import op_dot
            return op_dot(self, other, route)
        if isinstance(other, TensorTrain):
            from .operator_gram import op_tt_dot
            return op_tt_dot(self, other)
        return super().dot(other, reverse=reverse)

    def norm(self) -> float:
        """``||M x||`` from ``<M x, M x>`` (``operator_gram.op_dot``)"""
        return float(np.sqrt(abs(self.dot(self))))

    def error(self, other, relative: bool = False, rmse: bool = False, fast: bool = False) -> float:
        """``||self - other||``.  ``fast=True`` is the reference's formula on ``<self, self>``, ``<self, other>`` and
        ``<other, other>``, which form nothing dense against trains and operator products (or sums of them); it has that
        formula's floor of about 1e-8 relative.  ``fast=False`` keeps the dense difference of the base class."""
        if not fast:
            return super().error(other, relative=relative, rmse=rmse, fast=False)
        if isinstance(other, np.ndarray):
            other = DenseTensor(other)
        aa, ab, bb = self.dot(self), self.dot(other), other.dot(other)
        err = float(_fast_error(aa, ab, bb)) if aa + bb > 0 else 0.0
        return float(_error_tail(err, float(np.sqrt(abs(bb))), self.shape, relative, rmse))

    def __mul__(self, other: float) -> "OperatorProduct":
        return OperatorProduct(self.mpo, self.tt * other)

    def __repr__(self) -> str:
        return f"<Operator-times-train product of shape {self.shape} with operator rank {tuple(self.mpo.rank)} and train rank {tuple(self.tt.rank)} at {hex(id(self))}>"
