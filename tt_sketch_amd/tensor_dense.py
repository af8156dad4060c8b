"""A ``TensorTrain`` against a dense tensor: the one pass of ``csrc/tt_dense_stats.hip`` (``ttsk_tt_dense_stats`` and its
slab form ``ttsk_tt_dense_stats_ld``) with its planning arithmetic.

Entry points: ``_dense_operand`` and ``_tt_dense_pass``, which ``TensorTrain.dense_stats`` / ``to_dense_dev`` call;
``_dense_split`` plans the cut and the slabs under the panel budget ``_PANEL_BYTES``.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from .device import DevArray, contract
from .tensor import DenseTensor, TensorTrain, _prod

_PANEL_BYTES = 256 << 20      # the panels L and R (or L, one slab of R and R') of a pass stay below this


def _dense_split(shape, ranks, budget_bytes: int = _PANEL_BYTES) -> dict:
    """Where to cut a train of the given ``shape`` and bond ``ranks`` (d - 1 of them) for the pass over a dense tensor:
    ``T^{<k>} = L R`` with L (M x rho) the modes before bond ``k`` and R (rho x N) the rest, ``k`` minimising
    ``(M + N) rho`` (the numbers that must exist beside the tensor; the first such bond on a tie).  If the two panels
    exceed ``budget_bytes`` the right group is cut into slabs of its leading mode k: for the values ``[j0, j1)`` of that
    mode ``R_J = G_k[:, j0:j1, :] R'`` with ``R' = G_{k+1} ... G_{d-1}``, and the plan keeps
    ``8 (M rho + (j1 - j0) N' rho + rho' N')`` under the budget (``N' = N / n_k``).  Pure arithmetic, no device call.
    Returns ``dict(k, M, N, rho, slabs)``, ``slabs`` the list of ``(j0, j1)`` (one entry covering the mode: no slabbing)."""
    shape = tuple(int(n) for n in shape)
    d = len(shape)
    rk = (1,) + tuple(int(r) for r in ranks) + (1,)
    if d < 1 or len(rk) != d + 1 or min(shape) < 1 or min(rk) < 1:
        raise ValueError(f"_dense_split: shape {shape} with bond ranks {tuple(ranks)}")
    best = None
    for k in (range(1, d) if d > 1 else (0,)):
        M, N = _prod(shape[:k]), _prod(shape[k:])
        cost = (M + N) * rk[k]
        if best is None or cost < best[0]:
            best = (cost, k, M, N)
    cost, k, M, N = best
    rho, n_k = rk[k], shape[k]
    plan = dict(k=k, M=M, N=N, rho=rho, slabs=[(0, n_k)])
    if 8 * cost <= budget_bytes:
        return plan
    Np = N // n_k
    fixed, per = 8 * (M * rho + rk[k + 1] * Np), 8 * Np * rho
    width = (budget_bytes - fixed) // per if budget_bytes > fixed else 0
    if width < 1:
        raise ValueError(f"_dense_split: a train of shape {shape} and ranks {rk[1:-1]} cut at bond {k} needs "
                         f"{fixed + per} bytes of panels (L {M} x {rho}, one slice of R {rho} x {Np}, R' {rk[k + 1]} x {Np}) "
                         f"for a single value of mode {k}: above the budget of {budget_bytes} bytes")
    width = min(width, n_k)
    plan["slabs"] = [(j, min(j + width, n_k)) for j in range(0, n_k, width)]
    return plan


def _dense_operand(X, shape):
    """The dense argument of ``dense_stats`` as (C-contiguous DevArray, transposed): checked against ``shape`` before
    anything touches the device.  A ``.T`` view of a contiguous buffer is returned as that buffer with ``transposed``
    set (the caller runs its own ``.T`` against it: no copy); any other layout is copied once."""
    if isinstance(X, np.ndarray):
        X = DenseTensor(X)
    if not isinstance(X, DenseTensor):
        raise TypeError(f"dense_stats: a DenseTensor or an ndarray expected, got {type(X).__name__}")
    if tuple(X.shape) != tuple(shape):
        raise ValueError(f"dense_stats: dense tensor of shape {tuple(X.shape)}, tensor train of shape {tuple(shape)}")
    if np.dtype(X.data.dtype) != np.float64:
        raise TypeError(f"dense_stats: float64 data expected, got {X.data.dtype}")
    arr = X.dev_data()
    if arr.is_contiguous():
        return arr, False
    if arr.T.is_contiguous():
        return arr.T, True
    return arr.contiguous(), False


def _core_chain(cores, from_right: bool) -> DevArray:
    """The product of consecutive cores as one (r_first, n ... n, r_last) array, built from the cheap end."""
    if from_right:
        acc = cores[-1]
        for c in cores[-2::-1]:
            acc = contract("ajb,bm->ajm", c, acc.reshape(acc.shape[0], -1)).reshape(c.shape[0], -1, acc.shape[2])
        return acc
    acc = cores[0]
    for c in cores[1:]:
        acc = contract("mb,bjc->mjc", acc.reshape(-1, acc.shape[2]), c).reshape(acc.shape[0], -1, c.shape[2])
    return acc


def _tt_dense_pass(tt: "TensorTrain", X: Optional[DevArray], want_out: bool, want_stats: bool):
    """``ttsk_tt_dense_stats`` over the whole tensor: (DevArray of ``tt.shape`` or None, the four sums ``x . t``,
    ``t . t``, ``|t - x|^2``, ``x . x`` as a host array or None).  ``X``: C-contiguous device array of ``tt.shape``, or
    None.  Slabs (``_dense_split``) are passed in order and their sums added on the device."""
    from . import _native as nat
    plan = _dense_split(tt.shape, tt.rank, _PANEL_BYTES)
    k, M, N, rho, slabs = plan["k"], plan["M"], plan["N"], plan["rho"], plan["slabs"]
    cores = [c.contiguous() for c in tt.dev_cores()]                # a .T train holds transposed views
    one = lambda: DevArray.from_host(np.ones((1, 1)))
    L = _core_chain(cores[:k], False).contiguous().reshape(M, rho) if k else one()
    out = DevArray.empty(tt.shape) if want_out else None
    stats = DevArray.empty((4,)) if want_stats else None
    if len(slabs) == 1:
        R = _core_chain(cores[k:], True).contiguous().reshape(rho, N)
        nat.call("ttsk_tt_dense_stats", L, M, R, N, rho, X, out, stats, 0)
    else:
        Np = N // tt.shape[k]
        Rp = _core_chain(cores[k + 1:], True).contiguous().reshape(-1, Np) if k + 1 < tt.ndim else one()
        slab = lambda a: None if a is None else a.reshape(M, N)[:, j0 * Np:j1 * Np]       # its columns, rows N apart
        for i, (j0, j1) in enumerate(slabs):
            RJ = contract("ajb,bn->ajn", cores[k][:, j0:j1, :], Rp)
            nat.call("ttsk_tt_dense_stats_ld", L, M, RJ, (j1 - j0) * Np, rho, slab(X), N, slab(out), N, stats,
                     1 if i else 0, 0)
    return out, (stats.get() if want_stats else None)
