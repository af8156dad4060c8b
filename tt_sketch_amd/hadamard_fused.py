"""Fast path: streaming sketch of one entrywise product of two tensor trains (``HadamardProduct``) with tensor-train DRMs.

The left chain's ``W_k = L_{k-1} o (X_k, Y_k)`` serves both the chain step and ``Psi_k``, so a mode costs two
``hadamard_apply`` calls, one per side, where the generic driver makes three; the chains, Psi and Omega are one ``contract``
each on them.  No Kronecker core anywhere.  Sums, orthogonal / hmt sketches and rank slices go
through the generic driver.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

from .device import DevArray, contract
from .hadamard_product import HadamardProduct, hadamard_apply
from .operator_product import chain_start
from .paths import SketchMethod, drm_pair


def _chain(product: HadamardProduct, drm_cores, route=None) -> Tuple[List[DevArray], List[DevArray]]:
    """The d - 1 steps of one side: (W_k, L_k) with W_k (l_{k-1}, n_k, R_k r_k) and L_k (R_k r_k, l_k)"""
    Xs, Ys = product.dev_parts()
    L = chain_start()
    Ws, Lks = [], []
    for k, D in enumerate(drm_cores):
        W = hadamard_apply(L, Xs[k], Ys[k], route=route)
        Lk = contract("lic,lim->cm", W, D)
        Ws.append(W)
        Lks.append(Lk)
        L = Lk.reshape(Xs[k].shape[2], Ys[k].shape[2], Lk.shape[1])
    return Ws, Lks


def try_hadamard_sketch(tensor, left_drm, right_drm, method, route: Optional[str] = None) -> Optional[Tuple[list, list]]:
    """(Psi, Omega) device arrays, or None if the path does not apply: streaming sketches of a single ``HadamardProduct``
    with unsliced ``TensorTrainDRM``s.  ``route`` goes to ``hadamard_apply`` (the switch of ``paths.py``): None is its routing
    rule, ``"kernel"`` / ``"composed"`` that route at every step."""
    if method != SketchMethod.streaming or type(tensor) is not HadamardProduct:
        return None
    # (a rank slice of a blocked sketch: the general path)
    if not drm_pair(tensor.shape, left_drm, right_drm, sliced_ok=False):
        return None
    d = len(tensor.shape)
    tensor.prepare_device()
    WL, Lc = _chain(tensor, left_drm.dev_cores(), route)
    WR, Rc = _chain(tensor.T, right_drm.dev_cores(), route)
    # the right contraction at bond mu is step d - 2 - mu of the reversed walk; both sides index the bond by (beta, a)
    Psi = [contract("lic,cm->lim", WL[mu], Rc[d - 2 - mu]) for mu in range(d - 1)]
    # the last Kronecker core is W_0 of the reversed walk: Psi_{d-1}[l, i] = sum_c L_{d-2}[c, l] WR_0[0, i, c]
    Psi.append(contract("cl,ic->li", Lc[d - 2], WR[0][0]).reshape(Lc[d - 2].shape[1], tensor.shape[d - 1], 1))
    Omega = [contract("cl,cr->lr", Lc[mu], Rc[d - 2 - mu]) for mu in range(d - 1)]
    return Psi, Omega
