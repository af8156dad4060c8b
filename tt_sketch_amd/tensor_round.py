"""Gram-SVD rounding of tensor trains on the device (Al Daas, Ballard, Manning, "Parallel tensor train
rounding using Gram SVD", 2022).

Two Gram chains give the ``r x r`` Gram matrix of the left part and of the right part at every bond (``contract``, the two
directions on two library streams); ``ttsk_gram_round_bonds`` (``csrc/gram_round.hip``) truncates every bond at once from
them; the new cores are ``Q_k C_k P_{k+1}``.  ``TensorTrain.round_gram`` and ``TensorTrain.svdvals_gram`` call these.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from .device import DevArray, contract
from .tensor import TensorTrain
from .utils import TTRank, process_tt_rank

_MAX_RANK = 1024             # GRB_MAX_RANK of gram_round_plan.h: one workgroup per bond, the limit of round_dev
_MAX_BONDS = 64              # GRB_MAX_BONDS: the bonds of one ttsk_gram_round_bonds call
_HELPER = 1                  # the library stream of the right Gram chain; the left chain and everything else run on stream 0


def _left_grams(cores: List[DevArray], stream: int) -> List[DevArray]:
    """``GL_b``, b = 1 .. d - 1: ``GL_1 = C_0^T C_0`` and ``GL_{b+1}[c, e] = sum GL_b[a, a'] C_b[a, i, c] C_b[a', i, e]``, two
    ``contract`` calls per mode."""
    M = cores[0].reshape(cores[0].shape[1], cores[0].shape[2])
    out = [contract("ia,ib->ab", M, M, stream=stream)]
    for C in cores[1:-1]:
        T = contract("ab,bie->aie", out[-1], C, stream=stream)
        out.append(contract("aic,aie->ce", C, T, stream=stream))
    return out


def _right_grams(cores: List[DevArray], stream: int) -> List[DevArray]:
    """``GR_b``, b = 1 .. d - 1, the same construction from the other end."""
    M = cores[-1].reshape(cores[-1].shape[0], cores[-1].shape[1])
    out = [contract("ai,bi->ab", M, M, stream=stream)]
    for C in cores[-2:0:-1]:
        T = contract("aic,ce->aie", C, out[-1], stream=stream)
        out.append(contract("aie,bie->ab", T, C, stream=stream))
    return out[::-1]


def _grams(cores: List[DevArray]) -> Tuple[List[DevArray], List[DevArray]]:
    """Both chains, queued side by side: the right one on the helper stream behind whatever stream 0 holds so far (the
    cores may still be in flight there), and stream 0 waits for it before the bond solve."""
    from . import _native as nat
    nat.call("ttsk_stream_wait", _HELPER, 0)
    GR = _right_grams(cores, _HELPER)
    GL = _left_grams(cores, 0)
    nat.call("ttsk_stream_wait", 0, _HELPER)
    return GL, GR


def _bond_solve(GL: List[DevArray], GR: List[DevArray], ranks, caps, eps: float):
    """``ttsk_gram_round_bonds`` over all bonds (in calls of at most ``_MAX_BONDS``): ``(Pt, Q, Sigma, rho)`` with ``Pt[b]``
    and ``Q[b]`` ``(r, r)`` arrays of which the first ``rho[b]`` rows count, ``Sigma[b]`` ``(r,)`` and ``rho`` the chosen ranks
    as a device array of int32."""
    from . import _native as nat
    count = len(ranks)
    Pt = [DevArray.empty((r, r)) for r in ranks]
    Q = [DevArray.empty((r, r)) for r in ranks]
    S = [DevArray.empty((r,)) for r in ranks]
    rho = DevArray.empty((count,), dtype=np.int32)
    for lo in range(0, count, _MAX_BONDS):
        hi = min(count, lo + _MAX_BONDS)
        nat.call("ttsk_gram_round_bonds", nat.ptr_array(GL[lo:hi]), nat.ptr_array(GR[lo:hi]), nat.i64_array(ranks[lo:hi]),
                 nat.i64_array(caps[lo:hi]), hi - lo, float(eps), nat.ptr_array(Pt[lo:hi]), nat.ptr_array(Q[lo:hi]),
                 nat.ptr_array(S[lo:hi]), rho[lo:hi], 0)
    return Pt, Q, S, rho


def _solve(tt: TensorTrain, caps, eps: float):
    """The Gram chains and the bond solve of a train: its contiguous device cores and what ``_bond_solve`` returns."""
    if any(r > _MAX_RANK for r in tt.rank):
        raise ValueError(f"round_gram: TT rank {max(tt.rank)} > {_MAX_RANK} is beyond the one-workgroup SVD; use round()")
    if not (eps >= 0.0 and np.isfinite(eps)):
        raise ValueError(f"round_gram: eps = {eps} must be finite and not negative")
    cores = [c.contiguous() for c in tt.dev_cores()]
    GL, GR = _grams(cores)
    out = _bond_solve(GL, GR, list(tt.rank), list(caps), eps)
    return cores, out


def round_gram(tt: TensorTrain, eps: Optional[float] = None, max_rank: Optional[TTRank] = None) -> TensorTrain:
    """``TensorTrain.round_gram``: see there."""
    from . import _native as nat
    eps = 0.0 if eps is None else float(eps)
    caps = process_tt_rank(tt.rank if max_rank is None else max_rank, tt.shape, trim=True)
    if tt.ndim == 1:
        return TensorTrain([tt.dev_cores()[0].copy()])
    cores, (Pt, Q, _, rho_dev) = _solve(tt, caps, eps)
    rho = [int(r) for r in rho_dev.get()]                       # the one read-back
    nat.call("ttsk_sync", _HELPER)                              # idle since stream 0 waited for it: lets the pool reuse its buffers
    out = []
    for k, C in enumerate(cores):
        if k > 0:
            C = contract("ca,aib->cib", Q[k - 1][:rho[k - 1]], C)
        if k < tt.ndim - 1:
            C = contract("cib,eb->cie", C, Pt[k][:rho[k]])
        out.append(C)
    return TensorTrain(out)


def svdvals_gram(tt: TensorTrain) -> List[np.ndarray]:
    """``TensorTrain.svdvals_gram``: see there."""
    from . import _native as nat
    if tt.ndim == 1:
        return []
    _, (_, _, S, _) = _solve(tt, tt.rank, 0.0)
    feasible = process_tt_rank(tt.rank, tt.shape, trim=True)
    vals = [s.get()[:k] for s, k in zip(S, feasible)]
    nat.call("ttsk_sync", _HELPER)
    return vals
