"""Fast path: streaming sketch of a sum of operator-times-train products (plain trains mixed in) with tensor-train DRMs.

The sum is one block-structured train: with the terms' ``W_k`` side by side along the product-rank axis, the chain step,
Psi and Omega of the whole sum are one product each.  Per mode that is one ``op_apply`` over all terms and one ``contract``
per side for the chains, one ``contract`` for Psi (on the left chain's ``W_k``) and one for Omega.  Where ``op_apply`` takes
the kernel -- several small terms, by its routing rule -- that is six launches whatever the number of terms; where it
composes W from ``contract`` calls instead, two or three more per term and side.  No product core anywhere (DESIGN
section 13).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

from .device import DevArray, contract
from .operator_product import OperatorProduct, chain_start, op_apply
from .paths import SketchMethod, drm_pair
from .tensor import TensorSum, TensorTrain


def _parts(term):
    """(operator cores or Nones, train cores) of a term, on the device"""
    if type(term) is OperatorProduct:
        return term.dev_parts()
    cores = term.dev_cores()
    return [None] * len(cores), cores


def _chain(terms, drm_cores, route=None) -> Tuple[List[DevArray], List[DevArray]]:
    """The d - 1 steps of one side: (W_k, L_k) with W_k (l_{k-1}, n_k, cols_k) over all terms and L_k (cols_k, l_k)"""
    parts = [_parts(t) for t in terms]
    Ls = [chain_start()] * len(terms)
    Ws, Lcat = [], []
    for k, D in enumerate(drm_cores):
        Ms, Cs = [p[0][k] for p in parts], [p[1][k] for p in parts]
        W, offs = op_apply(Ls, Ms, Cs, route=route)
        Lk = contract("lic,lim->cm", W, D)
        Ws.append(W)
        Lcat.append(Lk)
        Ls = []
        for M, C, off in zip(Ms, Cs, offs):
            R1, r1 = (1 if M is None else M.shape[3]), C.shape[2]
            Ls.append(Lk[off:off + R1 * r1].reshape(R1, r1, Lk.shape[1]))
    return Ws, Lcat


def try_operator_sketch(tensor, left_drm, right_drm, method, route: Optional[str] = None) -> Optional[Tuple[list, list]]:
    """(Psi, Omega) device arrays, or None if the path does not apply: streaming sketches, unsliced ``TensorTrainDRM``s,
    an ``OperatorProduct`` or a ``TensorSum`` of ``OperatorProduct``s and ``TensorTrain``s with at least one product.
    ``route`` goes to ``op_apply`` (the switch of ``paths.py``): None is its routing rule, ``"kernel"`` / ``"composed"`` that
    route at every step."""
    if method != SketchMethod.streaming:
        return None
    terms = tensor.tensors if type(tensor) is TensorSum else [tensor]
    if not terms or not all(type(t) in (OperatorProduct, TensorTrain) for t in terms):
        return None
    if not any(type(t) is OperatorProduct for t in terms):
        return None
    # (a rank slice of a blocked sketch: the general path)
    if not drm_pair(tensor.shape, left_drm, right_drm, sliced_ok=False):
        return None
    d = len(tensor.shape)
    if any(tuple(t.shape) != tuple(tensor.shape) for t in terms):
        return None
    for t in terms:
        t.prepare_device()
    WL, Lc = _chain(terms, left_drm.dev_cores(), route)
    WR, Rc = _chain([t.T for t in terms], right_drm.dev_cores(), route)
    # the right contraction at bond mu is step d - 2 - mu of the reversed walk; both sides index the bond by (term, beta, a)
    Psi = [contract("lic,cm->lim", WL[mu], Rc[d - 2 - mu]) for mu in range(d - 1)]
    # the last product cores are W_0 of the reversed walk: Psi_{d-1}[l, i] = sum_c L_{d-2}[c, l] WR_0[0, i, c]
    Psi.append(contract("cl,ic->li", Lc[d - 2], WR[0][0]).reshape(Lc[d - 2].shape[1], tensor.shape[d - 1], 1))
    Omega = [contract("cl,cr->lr", Lc[mu], Rc[d - 2 - mu]) for mu in range(d - 1)]
    return Psi, Omega
