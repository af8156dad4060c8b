"""Inner products of a ``TuckerTensor`` on the device, built from existing device primitives (``contract``, ``ttsk_sum``,
``ttsk_tt_dense_stats``): against another Tucker tensor (``tucker_dot``), a tensor train (``tucker_tt_dot``) and a CP
tensor (``tucker_cp_dot``).  Every product works on the cores and the ``(s_k, n_k)`` factors alone: nothing of the size of
the tensor is formed.  The resident ``dot`` / ``norm`` / ``error(fast=True)`` of ``TuckerTensor``,
``TensorTrain`` and ``CPTensor`` call these.
"""
from __future__ import annotations

from .device import DevArray, contract
from .tensor import CPTensor, DenseTensor, TensorTrain, TuckerTensor


def _same_shape(what: str, a, b) -> None:
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"{what}: tensors of shapes {tuple(a.shape)} and {tuple(b.shape)}")


def _total(v: DevArray) -> float:
    """the sum of all entries in the library's fixed order (``ttsk_sum``)"""
    from . import _native as nat
    v = v.contiguous()
    out = DevArray.empty((1,))
    nat.call("ttsk_sum", v, v.size, out, 0)
    return float(out.get()[0])


def tucker_dot(a: "TuckerTensor", b: "TuckerTensor") -> float:
    """``<a, b>`` of two Tucker tensors of one shape: ``M_k = U_k U'_k^T`` (``s_k x s'_k``), the core of ``a`` times
    ``M_k`` mode after mode, the result against the core of ``b`` row by row, the rows added by ``ttsk_sum``."""
    for t in (a, b):
        if not isinstance(t, TuckerTensor):
            raise TypeError(f"tucker_dot: {type(t).__name__} is not a TuckerTensor")
    _same_shape("tucker_dot", a, b)
    fa, fb = a.dev_parts()[0], b.dev_parts()[0]
    T, cb = a.dev_core_contiguous(), b.dev_core_contiguous()
    left = 1
    for k, (U, V) in enumerate(zip(fa, fb)):
        M = contract("si,ti->st", U, V)
        T = contract("lsr,st->ltr", T.reshape(left, U.shape[0], -1), M)
        left *= V.shape[0]
    rows = cb.shape[0]
    return _total(contract("ar,ar->a", T.reshape(rows, -1), cb.reshape(rows, -1)))


def tucker_tt_dot(tucker: "TuckerTensor", tt: "TensorTrain") -> float:
    """``<tucker, tt>``: the train's cores projected on the factors, ``G'_k[a, s, b] = sum_i G_k[a, i, b] U_k[s, i]``, give a
    train of mode sizes ``s_k``, which runs against the core as a dense tensor (``ttsk_tt_dense_stats``)."""
    if not isinstance(tucker, TuckerTensor) or not isinstance(tt, TensorTrain):
        raise TypeError(f"tucker_tt_dot: a TuckerTensor and a TensorTrain expected, got {type(tucker).__name__} and {type(tt).__name__}")
    _same_shape("tucker_tt_dot", tucker, tt)
    factors, core = tucker.dev_parts()
    small = TensorTrain([contract("aib,si->asb", G, U) for G, U in zip(tt.dev_cores(), factors)])
    return float(small.dense_stats(DenseTensor(core))[0])


def tucker_cp_dot(tucker: "TuckerTensor", cp: "CPTensor") -> float:
    """``<tucker, cp>``: the CP factors projected, ``A'_k = U_k A_k`` (``s_k x R``), the core contracted with them mode by
    mode with the CP rank as the batch index, the ``R`` terms added by ``ttsk_sum``."""
    if not isinstance(tucker, TuckerTensor) or not isinstance(cp, CPTensor):
        raise TypeError(f"tucker_cp_dot: a TuckerTensor and a CPTensor expected, got {type(tucker).__name__} and {type(cp).__name__}")
    _same_shape("tucker_cp_dot", tucker, cp)
    factors, core = tucker.dev_parts()[0], tucker.dev_core_contiguous()
    proj = [contract("si,ir->sr", U, A) for U, A in zip(factors, cp.dev_cores())]
    s0 = proj[0].shape[0]
    v = contract("sx,sr->rx", core.reshape(s0, -1), proj[0])
    for W in proj[1:]:
        v = contract("rsx,sr->rx", v.reshape(cp.rank, W.shape[0], -1), W)
    return _total(v)
