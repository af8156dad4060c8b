"""Inner products of whole tensors on the device.

``tt_gram``: the Gram matrix of tensor trains in one pass (``csrc/tt_gram.hip``, ``ttsk_tt_gram``), its composed chain
and the measured rule that routes between them (``_gram_route_ms``).  ``cp_gram``: the inner product
of two CP tensors (``csrc/cp_gram.hip``, ``ttsk_cp_gram``), and ``_tt_cp_dot``, a train against a CP tensor by the chain
of ``ttsk_cp_chain_step``.  The resident ``dot`` / ``norm`` / ``error(fast=True)`` of ``TensorTrain``
and ``CPTensor`` call these.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

from .device import DevArray, contract
from .paths import resolve, taken
from .tensor import CPTensor, TensorTrain

_GRAM_MAX_TRAINS = 128       # K + M of one ttsk_tt_gram call
# The routing rule of DESIGN section 12, its constants measured on one MI355X (profiles/tt_gram_bench.json): the work
# of the pass beyond its launches against the time of the composed chain.
_GRAM_CUS = 256              # the chip the constants were measured on; the plan's chunks per pair follow the CU count
_GRAM_MAX_CHUNKS = 64        # GRAM_MAX_CHUNKS of tt_gram_plan.h
_GRAM_REDUCE_MS = 0.9e-6     # per partial a workgroup adds while it forms acc (chunks x ra x rb of them per mode)
_GRAM_WG_FLOPS_MS = 3e7      # flops per ms of one workgroup on its run of slices
_GRAM_CHAIN_MODE_MS = 0.045  # the chain per pair and mode: two launch-bound ``contract`` calls


def _gram_route_ms(ra: np.ndarray, rb: np.ndarray, shape) -> Tuple[float, float]:
    """(work of the Gram pass, time of the composed chain) in ms for the rank tables ``(K, d + 1)`` and ``(M, d + 1)``.
    The d + 1 launches and the one read-back of the pass never cost more than the 2 d launches and the read-back of
    one pair's chain, so only what a workgroup does in a launch can make the pass the slower path: the fused reduce
    of the previous mode's chunk partials and the two products over its run of slices, as many rounds of either as
    the grid (pairs x chunks) has workgroups per CU."""
    pairs = ra.shape[0] * rb.shape[0]
    a, b = ra.max(0).astype(np.float64), rb.max(0).astype(np.float64)
    work, prev = 0.0, 1
    for k, n in enumerate(shape):
        chunks = max(1, min(-(-_GRAM_CUS // pairs), _GRAM_MAX_CHUNKS, int(n)))
        slices = -(-int(n) // chunks)
        flops = slices * 2.0 * (a[k] * b[k] * a[k + 1] + a[k + 1] * b[k] * b[k + 1])
        rounds = -(-pairs * chunks // _GRAM_CUS)
        work += rounds * (_GRAM_REDUCE_MS * prev * a[k] * b[k] + flops / _GRAM_WG_FLOPS_MS)
        prev = chunks
    return work, pairs * len(shape) * _GRAM_CHAIN_MODE_MS


def _tt_dot_composed(x: TensorTrain, y: TensorTrain) -> float:
    """<x, y> of two resident trains as a chain of 2 d ``contract`` launches: what ``tt_gram`` falls back to beyond the
    cover of ``ttsk_tt_gram`` (a rank above 128) and where its routing rule expects the chain to be faster."""
    acc = None
    for a, b in zip(x.dev_cores(), y.dev_cores()):
        t = a.reshape(a.shape[1], a.shape[2]) if acc is None else contract("ij,ika->jka", acc, a)
        b = b.reshape(b.shape[1], b.shape[2]) if acc is None else b
        acc = contract("ka,kb->ab", t, b) if acc is None else contract("jka,jkb->ab", t, b)
    return float(acc.get().sum())


def _gram_composed(As, Bs, sym: bool) -> np.ndarray:
    G = np.empty((len(As), len(Bs)))
    for p, a in enumerate(As):
        for q, b in enumerate(Bs):
            G[p, q] = G[q, p] if sym and q < p else _tt_dot_composed(a, b)
    return G


def _gram_pass(As: Sequence[TensorTrain], Bs: Sequence[TensorTrain], sym: bool, route: Optional[str], out: DevArray) -> bool:
    """One block by ``ttsk_tt_gram`` into ``out``, a contiguous ``(K, M)`` on the device, nothing read back.  False, and
    nothing written, where the block goes to the composed chain: ``route`` says so, the rule does, or the entry refuses
    and the route is not ``"kernel"``."""
    from . import _native as nat
    if route == "composed":
        return False
    d = As[0].ndim
    cores = [[c.contiguous() for c in t.dev_cores()] for t in list(As) + list(Bs)]
    ranks = [[c.shape[0] for c in cs] + [cs[-1].shape[2]] for cs in cores]
    K, M = len(As), len(Bs)
    if route is None:
        work, chain = _gram_route_ms(np.array(ranks[:K]), np.array(ranks[K:]), As[0].shape)
        if taken(route, work, chain * (K + 1) / (2 * M) if sym else chain) == "composed":   # of a symmetric block the chain forms the upper triangle
            return False
    try:
        nat.call("ttsk_tt_gram", nat.ptr_array([c for cs in cores[:K] for c in cs]), nat.i64_array([r for rk in ranks[:K] for r in rk]), K,
                 nat.ptr_array([c for cs in cores[K:] for c in cs]), nat.i64_array([r for rk in ranks[K:] for r in rk]), M,
                 nat.i64_array(As[0].shape), d, out, 0)
    except nat.TtskUnsupported:
        if route == "kernel":
            raise
        return False
    return True


def _gram_block(As: Sequence[TensorTrain], Bs: Sequence[TensorTrain], sym: bool = False, route: Optional[str] = None) -> np.ndarray:
    route = resolve(route)
    if route == "composed":
        return _gram_composed(As, Bs, sym)
    out = DevArray.empty((len(As), len(Bs)))
    return out.get() if _gram_pass(As, Bs, sym, route, out) else _gram_composed(As, Bs, sym)


def tt_gram(As: Sequence[TensorTrain], Bs: Optional[Sequence[TensorTrain]] = None, route: Optional[str] = None) -> np.ndarray:
    """``G[p, q] = <As[p], Bs[q]>`` as a ``(K, M)`` array (``Bs=None``: ``As``).  The trains share one shape and have each
    their own ranks; a host train is uploaded once (``dev_cores``).

    On the device pass, ``ttsk_tt_gram``, that is one call (one launch per mode over all pairs) per block of at most
    ``_GRAM_MAX_TRAINS`` trains, and the same bits on every call.  Both hold on that pass only: beyond the cover of the
    entry (a rank above 128), and where the routing rule of DESIGN section 12 (``_gram_route_ms``: few pairs of large
    ranks) expects the chain to be faster, a block is composed pair by pair from ``contract``, 2 d launches and a
    read-back each.  With ``Bs=None`` a single block computes only its upper triangle on the composed path; lists cut
    into several blocks (``K + M > _GRAM_MAX_TRAINS``) compute every block in full, the lower ones too.

    ``route`` is the switch of ``paths.py``: None is the rule above with its fallback, ``"composed"`` the chain for every
    block, ``"kernel"`` the pass for every block, with the entry's ``TtskUnsupported`` where it refuses."""
    route = resolve(route)
    As = list(As)
    sym = Bs is None
    Bs = As if sym else list(Bs)
    if not As or not Bs:
        raise ValueError("tt_gram: an empty list of trains")
    for t in As + Bs:
        if not isinstance(t, TensorTrain):
            raise TypeError(f"tt_gram: {type(t).__name__} is not a TensorTrain")
        if t.shape != As[0].shape:
            raise ValueError(f"tt_gram: trains of shapes {As[0].shape} and {t.shape}")
    K, M, half = len(As), len(Bs), _GRAM_MAX_TRAINS // 2
    if K + M <= _GRAM_MAX_TRAINS:
        return _gram_block(As, Bs, sym, route)
    out = np.empty((K, M))
    for p in range(0, K, half):
        for q in range(0, M, half):
            out[p:p + half, q:q + half] = _gram_block(As[p:p + half], Bs[q:q + half], route=route)
    return out


def _cp_factor(F: DevArray) -> Tuple[DevArray, int]:
    """A factor matrix ``(n, N)`` as ``ttsk_cp_gram`` takes it -- columns contiguous, rows a leading dimension >= N
    apart, so a column slice goes as it is -- and that leading dimension."""
    n, N = F.shape
    if not ((N == 1 or F.strides[1] == 1) and (n == 1 or F.strides[0] >= N)):
        F = F.contiguous()
    return F, (F.strides[0] if n > 1 else N)


def cp_gram(a: "CPTensor", b: Optional["CPTensor"] = None) -> float:
    """``<a, b> = sum_{j, j'} prod_k (A_k^T B_k)[j, j']`` of two CP tensors of one shape (``b=None``: ``<a, a>``, of which
    only the tiles on and above the diagonal are formed).  Host factors are uploaded once (``dev_cores``); one call of
    ``ttsk_cp_gram``, which keeps the product over the modes in registers: no dense tensor and no ``N x M`` array, and
    the same bits on every call."""
    from . import _native as nat
    sym = b is None or b is a
    for t in (a,) if sym else (a, b):
        if not isinstance(t, CPTensor):
            raise TypeError(f"cp_gram: {type(t).__name__} is not a CPTensor")
    if not sym and tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"cp_gram: CP tensors of shapes {a.shape} and {b.shape}")
    fa = [_cp_factor(F) for F in a.dev_cores()]
    fb = fa if sym else [_cp_factor(F) for F in b.dev_cores()]
    out = DevArray.empty((1,))
    nat.call("ttsk_cp_gram", nat.ptr_array([F for F, _ in fa]), nat.i64_array([ld for _, ld in fa]), a.rank,
             nat.ptr_array([F for F, _ in fb]), nat.i64_array([ld for _, ld in fb]), a.rank if sym else b.rank,
             nat.i64_array(a.shape), a.ndim, int(sym), out, 0)
    return float(out.get()[0])


def _tt_cp_dot(tt: "TensorTrain", cp: "CPTensor", route: Optional[str] = None) -> float:
    """``<tt, cp>`` by the left-to-right chain ``L_k[j, a'] = sum_{a, i} L_{k-1}[j, a] V_k[i, j] C_k[a, i, a']``: the
    recurrence of ``TensorTrainDRM.sketch_cp`` with the train's cores in place of the DRM's, so each mode is one
    ``ttsk_cp_chain_step`` -- or, beyond that entry's cover (a train rank above 128) and where ``cp_fused.chain_route_ms``
    gives the step to it, the two ``contract`` calls of ``sketch_cp``.  The last mode leaves ``(N, 1)``, which
    ``ttsk_sum`` adds in the library's fixed order.  ``route``: the switch of ``paths.py``."""
    from . import _native as nat
    from .cp_fused import _chain
    if tuple(tt.shape) != tuple(cp.shape):
        raise ValueError(f"dot: a train of shape {tt.shape} against a CP tensor of shape {cp.shape}")
    L = _chain(cp.dev_cores(), tt, resolve(route), 0)[-1].contiguous()
    out = DevArray.empty((1,))
    nat.call("ttsk_sum", L, L.size, out, 0)
    return float(out.get()[0])
