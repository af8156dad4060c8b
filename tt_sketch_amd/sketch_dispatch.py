"""Generic sketch driver: left/right partial contractions, Omega_mu, Psi_mu.

Device counterpart of the reference's ``tt_sketch/sketch_dispatch.py``: the same dispatch
tables keyed by tensor type (:51-82), TensorSum fan-out (:85-147), ``orth_step`` (:160-174),
``OrthogTTDRM`` (:177-193) and ``general_sketch`` (:202-275).  Partial contractions and the
sketch stay in HBM (DevArray) from the first DRM step to the last Psi; they are copied to
the host once, when the ``SketchContainer`` is built.
"""
from __future__ import annotations

import ctypes
import os
import sys
from functools import partial
from typing import Callable, List, Optional, Tuple

import numpy as np

from . import _native as nat
from . import cp_fused, hadamard_fused, operator_fused, sparse_fused, tt_fused
from .device import DevArray, as_dev, axpby, contract
from .drm import TensorTrainDRM
from .drm_base import DRM
from .sketch_container import SketchContainer
from .hadamard_product import HadamardProduct
from .operator_product import OperatorProduct
from .paths import SketchMethod
from .sketching_methods.abstract_methods import (CansketchCP, CansketchDense, CansketchHadamardProduct,
                                                 CansketchOperatorProduct, CansketchSparse, CansketchTT, CanSketchTucker)
from .sketching_methods.cp_sketch import sketch_omega_cp, sketch_psi_cp
from .sketching_methods.dense_sketch import sketch_omega_dense, sketch_psi_dense
from .sketching_methods.hadamard_product_sketch import sketch_omega_hadamard_product, sketch_psi_hadamard_product
from .sketching_methods.operator_product_sketch import sketch_omega_operator_product, sketch_psi_operator_product
from .sketching_methods.sparse_sketch import sketch_omega_sparse, sketch_psi_sparse
from .sketching_methods.tensor_train_sketch import sketch_omega_tt, sketch_psi_tt
from .sketching_methods.tucker_sketch import sketch_omega_tucker, sketch_psi_tucker
from .tensor import (CPTensor, DenseTensor, SparseTensor, Tensor, TensorSum, TensorTrain,
                     TuckerTensor)
from .utils import pinv_dev

ABSTRACT_TENSOR_SKETCH_DISPATCH = {
    SparseTensor: CansketchSparse, TensorTrain: CansketchTT, DenseTensor: CansketchDense,
    CPTensor: CansketchCP, TuckerTensor: CanSketchTucker, OperatorProduct: CansketchOperatorProduct,
    HadamardProduct: CansketchHadamardProduct,
}
DRM_SKETCH_METHOD_DISPATCH = {
    SparseTensor: "sketch_sparse", TensorTrain: "sketch_tt", DenseTensor: "sketch_dense",
    CPTensor: "sketch_cp", TuckerTensor: "sketch_tucker", OperatorProduct: "sketch_operator_product",
    HadamardProduct: "sketch_hadamard_product",
}
OMEGA_METHODS = {
    SparseTensor: sketch_omega_sparse, TensorTrain: sketch_omega_tt, DenseTensor: sketch_omega_dense,
    CPTensor: sketch_omega_cp, TuckerTensor: sketch_omega_tucker, OperatorProduct: sketch_omega_operator_product,
    HadamardProduct: sketch_omega_hadamard_product,
}
PSI_METHODS = {
    SparseTensor: sketch_psi_sparse, TensorTrain: sketch_psi_tt, DenseTensor: sketch_psi_dense,
    CPTensor: sketch_psi_cp, TuckerTensor: sketch_psi_tucker, OperatorProduct: sketch_psi_operator_product,
    HadamardProduct: sketch_psi_hadamard_product,
}


def _accumulate(acc: Optional[DevArray], term, shape) -> DevArray:
    term = as_dev(term)
    if tuple(term.shape) != tuple(shape):
        raise ValueError(f"summand sketch has shape {term.shape}, expected {tuple(shape)}")
    if acc is None:
        return term.copy() if not term.is_contiguous() or term.offset else term
    return axpby(acc, term, 1.0, 1.0)


def sketch_omega_sum(left_sketch_array, right_sketch_array, *, tensor: TensorSum, omega_shape,
                     **kwargs) -> DevArray:
    """Omega of a sum = sum of the summands' Omegas (reference :85-105)."""
    acc = None
    for summand, l, r in zip(tensor.tensors, left_sketch_array, right_sketch_array):
        acc = _accumulate(acc, OMEGA_METHODS[type(summand)](
            l, r, tensor=summand, omega_shape=omega_shape, **kwargs), omega_shape)
    return DevArray.zeros(omega_shape) if acc is None else acc


def sketch_psi_sum(left_sketch_array, right_sketch_array, *, tensor: TensorSum, psi_shape,
                   **kwargs) -> DevArray:
    """Psi of a sum (reference :111-136); either side may be None at the ends."""
    k = tensor.num_summands
    lefts = (None,) * k if left_sketch_array is None else left_sketch_array
    rights = (None,) * k if right_sketch_array is None else right_sketch_array
    acc = None
    for summand, l, r in zip(tensor.tensors, lefts, rights):
        acc = _accumulate(acc, PSI_METHODS[type(summand)](
            l, r, tensor=summand, psi_shape=psi_shape, **kwargs), psi_shape)
    return DevArray.zeros(psi_shape) if acc is None else acc


OMEGA_METHODS[TensorSum] = sketch_omega_sum
PSI_METHODS[TensorSum] = sketch_psi_sum


def sum_sketch(tensor: TensorSum, *, drm: DRM):
    """Per mode, the tuple of the summands' partial contractions (reference :142-147)."""
    gens = [get_sketch_method(t, drm)(t) for t in tensor.tensors]
    for _ in range(len(tensor.shape) - 1):
        yield tuple(next(g) for g in gens)


def get_sketch_method(tensor: Tensor, drm: DRM) -> Callable:
    """``drm.sketch_<kind>`` for the tensor's type (reference :150-157)."""
    name = DRM_SKETCH_METHOD_DISPATCH.get(type(tensor))
    if name is not None:
        if not hasattr(drm, name):
            raise ValueError(f"DRM of type {type(drm)} can't sketch {type(tensor)}")
        return getattr(drm, name)
    if isinstance(tensor, TensorSum):
        return partial(sum_sketch, drm=drm)
    raise ValueError(f"DRM of type {type(drm)} can't sketch {type(tensor)}")


def _pinvs_up_front(Omega_mats) -> dict:
    """{mu: pinv(Omega_mu)} for the Omega of shapes that occur at least twice, every stage ONE batched launch
    (``ttsk_pinv_batch_deferred``): all Omega are known before the sequential Psi loop starts.  Verdicts deferred."""
    groups = {}
    for mu, Om in enumerate(Omega_mats):
        O = as_dev(Om).contiguous()
        groups.setdefault(tuple(O.shape), []).append((mu, O))
    out = {}
    for (l, r), items in groups.items():
        if len(items) < 2 or min(l, r) > 128 or len(items) > 32:
            continue
        Ps = [DevArray.empty((r, l)) for _ in items]
        try:
            nat.call("ttsk_pinv_batch_deferred", len(items), nat.ptr_array([O for _, O in items]), l, r, nat.ptr_array(Ps), 0)
        except nat.TtskUnsupported:
            continue
        for (mu, O), p in zip(items, Ps):
            out[mu] = (p, O)
    return out


def orth_step(Psi, Omega=None, deferred: bool = False, pinv=None) -> DevArray:
    """Psi <- Q of thin QR(Psi_mat pinv(Omega)) (reference :160-174), all on the device.

    ``deferred``: one library call (``ttsk_orth_step``) that does not wait for the acceptance tests of its
    factorisations; the caller checks ``ttsk_deferred_status`` once and repeats on the robust path if needed."""
    P = as_dev(Psi).contiguous()
    r1, n, r2 = P.shape
    M = P.reshape(r1 * n, r2)
    k = r2 if Omega is None else int(as_dev(Omega).shape[0])
    if r1 * n < k:
        raise ValueError(f"cannot orthogonalise a {r1 * n} x {k} unfolding: trim the sketch ranks")
    if deferred and pinv is not None:
        Q = DevArray.empty((r1 * n, k))
        nat.call("ttsk_orth_step_pinv", M, r1 * n, r2, pinv[0], k, Q, 0)
        return Q.reshape(r1, n, k)
    if deferred:
        Om = None if Omega is None else as_dev(Omega).contiguous()
        Q = DevArray.empty((r1 * n, k))
        nat.call("ttsk_orth_step", M, r1 * n, r2, Om, k, Q, 0)
        return Q.reshape(r1, n, k)
    if Omega is not None:
        M = contract("ij,jk->ik", M, pinv_dev(Omega))
    elif M is P or M.buf is P.buf:
        M = M.copy()                       # QR works in place; keep the caller's Psi intact
    m, k = M.shape
    nat.call("ttsk_qr_thin", M, m, k, 0)
    return M.reshape(r1, n, k)


class OrthogTTDRM:
    """Left 'DRM' whose cores are the already orthogonalised Psi cores (reference :177-193)."""

    def __init__(self, rank, tensor):
        self.rank = rank
        self.drm = TensorTrainDRM(rank, tensor.shape, transpose=False, cores=[])
        self.generator = None
        self.tensor = tensor
        self.sketch_method = get_sketch_method(tensor, self.drm)

    def add_core(self, core):
        self.drm.cores.append(core)
        if self.generator is None:
            self.generator = self.sketch_method(self.tensor)

    def __next__(self):
        return next(self.generator)


def general_sketch_device(tensor: Tensor, left_drm: Optional[DRM], right_drm: DRM,
                          method: SketchMethod) -> Tuple[List[DevArray], List[DevArray]]:
    """The sketch as device arrays ``(Psi_cores, Omega_mats)`` (reference :202-275)."""
    from .sketching_methods import dense_sketch
    dense_sketch.clear_shared()
    try:
        return _general_sketch_device(tensor, left_drm, right_drm, method)
    finally:
        dense_sketch.clear_shared()


_ONE_CALL_ORTH = os.environ.get("TTSK_ORTH_ONE_CALL", "1") != "0"
# how often an orthogonal / hmt sketch had to be repeated on the robust factorisations (per method): systematically
# ill-conditioned inputs pay for the sketch twice, and this is where that shows
robust_reruns: dict = {}


def _general_sketch_device(tensor: Tensor, left_drm: Optional[DRM], right_drm: DRM,
                           method: SketchMethod) -> Tuple[List[DevArray], List[DevArray]]:
    if method in (SketchMethod.hmt, SketchMethod.orthogonal):
        # Optimistic pass: every orthogonalisation as one call on the fast factorisations, no verdict awaited (the
        # d - 1 steps are sequential in mu: each blocking read-back drains the queue).  ONE read-back at the end; a
        # rejected factorisation (rank-deficient Omega, ill-conditioned unfolding) repeats the sketch on the robust path.
        out, flag = None, ctypes.c_int(0)
        try:
            out = tt_fused.try_orth_sketch(tensor, left_drm, right_drm, method) if _ONE_CALL_ORTH else None
            if out is None:
                try:
                    out = _sketch_pass(tensor, left_drm, right_drm, method, deferred=True)
                except nat.TtskUnsupported:
                    out = None
        finally:
            # read AND clear the sticky flag whatever the pass raised (a ValueError of the argument checks, a HIP error):
            # left set, it would send the next, unrelated sketch to the robust path
            try:
                nat.call("ttsk_deferred_status", 0, ctypes.byref(flag))
            except nat.TtskError:
                if out is not None:          # (otherwise the pass's own exception is the one to report)
                    raise
        if out is not None and not flag.value:
            return out
        robust_reruns[method.value] = robust_reruns.get(method.value, 0) + 1
        if os.environ.get("TTSK_TRACE_RERUN", "0") != "0":
            print(f"tt_sketch_amd: {method.value} sketch repeated on the robust factorisations "
                  f"(optimistic pass {'rejected' if out is not None else 'unsupported'})", file=sys.stderr)
    return _sketch_pass(tensor, left_drm, right_drm, method, deferred=False)


def _sketch_pass(tensor: Tensor, left_drm: Optional[DRM], right_drm: DRM, method: SketchMethod,
                 deferred: bool) -> Tuple[List[DevArray], List[DevArray]]:
    d = len(tensor.shape)
    tensor.prepare_device()
    if method != SketchMethod.hmt:
        if left_drm is None:
            raise ValueError(f"left_drm must be provided for method '{method}'")
        left_contractions = list(get_sketch_method(tensor, left_drm)(tensor))
    right_contractions = list(get_sketch_method(tensor, right_drm)(tensor))
    if left_drm is None:
        left_drm = right_drm.T          # shape information only (HMT)
    left_rank = tuple(left_drm.rank)
    right_rank = tuple(right_drm.rank[::-1])

    Omega_mats: List[DevArray] = []
    if method != SketchMethod.hmt and type(tensor) is DenseTensor:
        from .sketching_methods import dense_sketch
        dense_sketch.prepare_left(tensor, left_contractions)     # DRM matrices: the left products from one read of the tensor
    if method != SketchMethod.hmt:
        omega_method = OMEGA_METHODS[type(tensor)]
        for mu in range(d - 1):
            Omega_mats.append(omega_method(left_contractions[mu], right_contractions[mu], tensor=tensor,
                                           mu=mu, omega_shape=(left_rank[mu], right_rank[mu])))

    orthogonalise = method in (SketchMethod.hmt, SketchMethod.orthogonal)
    if orthogonalise:
        left_psi_drm = OrthogTTDRM(left_rank, tensor)
    pinvs = _pinvs_up_front(Omega_mats) if (deferred and method == SketchMethod.orthogonal) else {}

    Psi_cores: List[DevArray] = []
    psi_method = PSI_METHODS[type(tensor)]
    for mu in range(d):
        if mu == 0:
            left_sketch, r1 = None, 1
        else:
            if orthogonalise:
                left_psi_drm.add_core(Psi_cores[-1])
                left_sketch = next(left_psi_drm)
            else:
                left_sketch = left_contractions[mu - 1]
            r1 = left_rank[mu - 1]
        if mu < d - 1:
            right_sketch, r2 = right_contractions[mu], right_rank[mu]
        else:
            right_sketch, r2 = None, 1
        Psi = psi_method(left_sketch, right_sketch, tensor=tensor, mu=mu,
                         psi_shape=(r1, tensor.shape[mu], r2))
        if mu < d - 1:
            if method == SketchMethod.orthogonal:
                Psi = orth_step(Psi, Omega_mats[mu], deferred, pinvs.get(mu))
            elif method == SketchMethod.hmt:
                Psi = orth_step(Psi, None, deferred)
        Psi_cores.append(as_dev(Psi))
    return Psi_cores, Omega_mats


# The fused paths, in the order they are asked: each takes (tensor, left_drm, right_drm, method) and returns the device
# arrays (Psi, Omega), or None where it does not apply (what each accepts of a DRM pair: ``paths.drm_pair``).
FUSED_PATHS = (tt_fused.try_stream_sketch, sparse_fused.try_sparse_gauss_sketch, operator_fused.try_operator_sketch,
               cp_fused.try_cp_sketch)
# asked after those, in the same way: the paths added since tests/test_cp_pass_host.py fixed the four above and their order
PRODUCT_PATHS = (hadamard_fused.try_hadamard_sketch,)


def general_sketch(tensor: Tensor, left_drm: Optional[DRM], right_drm: DRM,
                   method: SketchMethod) -> SketchContainer:
    """Sketch on the device, result copied to a host ``SketchContainer``."""
    for path in FUSED_PATHS + PRODUCT_PATHS:
        fused = path(tensor, left_drm, right_drm, method)
        if fused is not None:
            return SketchContainer(*fused)
    return SketchContainer(*general_sketch_device(tensor, left_drm, right_drm, method))
