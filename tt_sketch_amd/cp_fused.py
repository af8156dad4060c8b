"""CP input with tensor-train DRMs on the two one-pass kernels of ``csrc/cp_pass.hip``.

``chain_step`` (``ttsk_cp_chain_step``) is one step of ``TensorTrainDRM.sketch_cp``, ``psi_omega`` (``ttsk_cp_psi_omega``) a
Psi core and, in the same launch, an Omega matrix: the ``N x n x rank`` panels of the compositions in
``tensor_train_drm.py`` / ``cp_sketch.py`` are never stored.  Both return ``None`` where the entry's plan refuses the shape
(``TtskUnsupported``) or an operand's layout is not the entry's; the caller then runs its composition, which stays where it
was.

``try_cp_sketch`` is the fast path of ``general_sketch`` for a streaming sketch of a ``CPTensor`` with ``TensorTrainDRM``s
on both sides: the two chains on the library's streams 0 and 1, then one ``ttsk_cp_psi_omega`` per mode on stream 0 --
Psi_mu together with Omega_{mu-1}, which shares its left contraction -- 3 d - 2 launches in all while N <= 512 (DESIGN
section 14).

Routing: ``ttsk_cp_psi_omega`` wherever its plan accepts; the chain step by a cost rule (``chain_route_ms``), because one
workgroup per 128 rows loses to the two launch-bound GEMMs at small N.  ``route=`` and the ``forced`` context are the switch
of ``paths.py``: ``"kernel"`` / ``"composed"`` takes that route whatever the default is, and with ``"kernel"`` a refusal
raises instead of falling back, so a test knows which code it ran.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from . import _native as nat
from .device import DevArray, contract
from .paths import SketchMethod, drm_pair, forced, resolve, taken      # (`forced`: tests and profiles/scripts reach it here)
from .tensor import CPTensor


def _rows(A: Optional[DevArray]) -> bool:
    """a matrix the entries take as it is: rows a leading dimension apart, columns contiguous"""
    return A is None or (A.ndim == 2 and A.dtype == np.float64 and (A.shape[1] == 1 or A.strides[1] == 1)
                         and (A.shape[0] == 1 or A.strides[0] >= A.shape[1]))


def _ld(A: DevArray) -> int:
    return A.strides[0] if A.shape[0] > 1 else A.shape[1]


def _refused(route, what: str):
    if route == "kernel":
        raise nat.TtskUnsupported(f"cp_fused: {what}")
    return None


# Routing rule of the chain step (constants from profiles/cp_sketch_bench.json).  The kernel's grid is
# N / 128 workgroups that each walk all rho n / 4 k-blocks in turn, the composition's two GEMMs spread a small N over the
# chip but move the N x n x rho' panel through HBM twice.
CALL_MS = 0.019                # one queued call: half the two-contract composition at N = 100
KBLOCK_MS = 0.00062            # one k-block of the kernel's walk: (0.112 - CALL_MS) / 150 at N = 100, rho = 60, n = 10
PANEL_TB_S = 1.5               # rate at which the composition writes and reads its panel: 360 .. 480 MB in 0.14 .. 0.36 ms


def chain_route_ms(N: int, rho: int, n: int, rho1: int, first_mode: bool = False) -> Tuple[float, float]:
    """(kernel, composed) milliseconds the routing rule expects of one chain step"""
    kernel = CALL_MS + -(-rho * n // 4) * KBLOCK_MS
    composed = CALL_MS if first_mode else 2 * CALL_MS + 16.0 * N * n * rho1 / (PANEL_TB_S * 1e9)
    return kernel, composed


def chain_step(L: Optional[DevArray], V: DevArray, D: DevArray, route: Optional[str] = None, stream: int = 0) -> Optional[DevArray]:
    """``out[j, m] = sum_{a, k} L[j, a] V[k, j] D[a, k, m]`` as a new ``(N, rho')`` array; ``L`` None is the first mode
    (``rho = 1``).  ``V`` is taken with its strides, ``D`` is made contiguous.  None: the caller composes."""
    route = resolve(route)
    if route == "composed":
        return None
    n, N = V.shape
    rho, nd, rho1 = D.shape
    if nd != n or (L is not None and tuple(L.shape) != (N, rho)) or (L is None and rho != 1):
        raise ValueError(f"cp chain step: L {None if L is None else L.shape}, V {V.shape}, D {D.shape}")
    if not _rows(L):
        return _refused(route, f"chain of strides {L.strides}")
    if N == 0 or n == 0 or rho1 == 0:
        return _refused(route, "an empty operand")
    if route is None and taken(route, *chain_route_ms(N, rho, n, rho1, L is None)) == "composed":
        return None
    out = DevArray.empty((N, rho1), stream=stream)
    try:
        nat.call("ttsk_cp_chain_step", L, 0 if L is None else _ld(L), V, V.strides[0], V.strides[1], D.contiguous(stream), out, rho1,
                 N, rho, n, rho1, stream)
    except nat.TtskUnsupported:
        if route == "kernel":
            raise
        return None
    return out


def psi_omega(L: Optional[DevArray], R: Optional[DevArray], V: Optional[DevArray], R_om: Optional[DevArray] = None, psi: bool = True,
              omega: bool = False, route: Optional[str] = None, stream: int = 0) -> Optional[Tuple[Optional[DevArray], Optional[DevArray]]]:
    """``(Psi, Omega)`` of one launch: ``Psi[i, k, m] = sum_j L[j, i] V[k, j] R[j, m]`` as ``(l, n, r)`` and
    ``Omega[i, m] = sum_j L[j, i] R_om[j, m]`` (``R_om`` None: ``R``), each None unless asked for.  ``L`` / ``R`` None are the
    first / last mode (rank 1, all ones).  None instead of the pair: the caller composes."""
    route = resolve(route)
    if route == "composed":
        return None
    if not (psi or omega) or (psi and V is None):
        raise ValueError("cp psi_omega: nothing to compute, or Psi without a factor matrix")
    mats = [A for A in (L, R, R_om) if A is not None]
    N = V.shape[1] if V is not None else (mats[0].shape[0] if mats else 0)
    if any(A.ndim != 2 or A.shape[0] != N for A in mats):
        raise ValueError(f"cp psi_omega: {[A.shape for A in mats]} against CP rank {N}")
    if not all(_rows(A) for A in mats):
        return _refused(route, f"contractions of strides {[A.strides for A in mats]}")
    l = 1 if L is None else L.shape[1]
    r = 1 if R is None else R.shape[1]
    n = V.shape[0] if psi else 0
    r_om = r if R_om is None else R_om.shape[1]
    if N == 0 or l == 0 or r == 0 or (psi and n == 0) or (omega and r_om == 0):
        return _refused(route, "an empty operand")
    P = DevArray.empty((l, n, r), stream=stream) if psi else None
    O = DevArray.empty((l, r_om), stream=stream) if omega else None
    try:
        nat.call("ttsk_cp_psi_omega", L, 0 if L is None else _ld(L), R, 0 if R is None else _ld(R), V if psi else None,
                 V.strides[0] if psi else 0, V.strides[1] if psi else 0, P, R_om, 0 if R_om is None else _ld(R_om), r_om, O,
                 N, l, n, r, stream)
    except nat.TtskUnsupported:
        if route == "kernel":
            raise
        return None
    return P, O


def _chain(Vs: List[DevArray], drm, route, stream: int) -> List[DevArray]:
    """the d - 1 uncut contractions of one side, queued on ``stream``; a step that the routing rule or the plan gives to
    the composition is the two ``contract`` calls of ``TensorTrainDRM.sketch_cp`` on that stream"""
    out, L = [], None
    for V, D in zip(Vs, drm.dev_cores()):
        Lk = chain_step(L, V, D, route=route, stream=stream)
        if Lk is None and L is None:
            Lk = contract("ij,ik->jk", V, D[0], stream=stream)
        elif Lk is None:
            Lk = contract("ki,ikl->il", V, contract("ij,jkl->ikl", L, D, stream=stream), stream=stream)
        L = Lk
        out.append(L)
    return out


def try_cp_sketch(tensor, left_drm, right_drm, method, route: Optional[str] = None) -> Optional[Tuple[list, list]]:
    """(Psi, Omega) device arrays, or None if the path does not apply: a streaming sketch of a ``CPTensor`` with a left and
    a right ``TensorTrainDRM`` (rank slices of a blocked sketch included) whose shapes the two entries cover."""
    route = resolve(route)
    if route == "composed" or method != SketchMethod.streaming or type(tensor) is not CPTensor:
        return None
    if not drm_pair(tensor.shape, left_drm, right_drm):
        return None
    d = len(tensor.shape)
    Vs = tensor.dev_cores()
    for drm in (left_drm, right_drm):
        drm.dev_cores()                                   # uploads, if any, before the streams part
    nat.call("ttsk_stream_wait", 1, 0)                    # the right chain starts behind whatever made its operands
    try:
        Ls = _chain(Vs, left_drm, route, 0)
        Rs = _chain(Vs[::-1], right_drm, route, 1)
    finally:
        nat.call("ttsk_stream_wait", 0, 1)
    Ls = [left_drm._cut(mu, L) for mu, L in enumerate(Ls)]
    Rs = [right_drm._cut(mu, R) for mu, R in enumerate(Rs)][::-1]       # Rs[mu]: the modes behind mu
    Psi, Omega = [], []
    for mu in range(d):
        L = Ls[mu - 1] if mu else None
        R = Rs[mu] if mu < d - 1 else None
        out = psi_omega(L, R, Vs[mu], R_om=Rs[mu - 1] if mu else None, psi=True, omega=mu > 0, route=route, stream=0)
        if out is None:
            nat.call("ttsk_sync", 1)
            return None
        Psi.append(out[0])
        if mu:
            Omega.append(out[1])
    # stream 1 has drained before anything here is handed back to the pool: its buffers go to stream 0 users again
    nat.call("ttsk_sync", 1)
    return Psi, Omega
