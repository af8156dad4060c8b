"""Inner products of entrywise products of tensor trains that are never formed: ``<x o y, z>`` against
a train (``hadamard_tt_dot``) and ``<x o y, u o v>`` against another product (``hadamard_dot``), and with them the ``dot`` /
``norm`` / ``error(fast=True)`` of ``HadamardProduct``.  Nothing of the size of a Kronecker core ``(R r) x n x (R' r')`` is
formed, on the device or on the host.

Against a train ``z`` of ranks ``s`` the chain is ``G (R, r, s)``, ``G = 1`` before the first mode:

    W  = hadamard_apply(L = G, X_k, Y_k)                               (s, n, R' r')
    G'[(beta' a'), gamma'] = sum_{gamma, i} W[gamma, i, (beta' a')] Z_k[gamma, i, gamma']     one `contract`

Against a product ``u o v`` of ranks ``S`` and ``s`` the chain is ``G (R, r, S, s)``, in two halves per mode:

    A.  W[(gamma c), i, (beta' a')] = hadamard_apply(L = G.reshape(R, r, S s), X_k, Y_k)
    B.  G'[(beta' a'), gamma', c']  = sum_i sum_gamma U_k[gamma, i, gamma'] sum_c W[(gamma c), i, (beta' a')] V_k[c, i, c']

``8 n rho^5`` flops per mode at ranks ``rho`` against ``4 n rho^6`` through the formed cores.  B is ``hadamard_close``: one
``ttsk_hadamard_close`` call (csrc/hadamard_close.hip) or its composition from ``contract`` / ``copy_into`` calls.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from . import _native as nat
from .device import DevArray, axpby, contract, copy_into
from .hadamard_product import HadamardProduct, hadamard_apply
from .paths import resolve, taken
from .tensor import TensorTrain, _host, _on_device

# W of one mode is S s x n x R' r' doubles (s x n x R' r' against a train).  Past this many bytes the mode is cut into
# slices of i -- views of the cores -- whose partial G' are accumulated.  The figure is a bound on memory, not a tuning of
# speed: 2 GiB holds the whole W at ranks 32 x 32 against 32 x 32 and n = 200 (1.7 GB), the largest shape measured, and
# with the two W-sized temporaries of the composed route the step stays under 6 GiB of the device's 288 GB.
W_BUDGET_BYTES = 2 << 30

# The routing rule of half B, its constants measured on one MI355X (profiles/hadamard_gram_bench.json,
# the four shapes of step B alone).  A ttsk_hadamard_close call costs its floor (the kernel and the ttsk_sum_slices behind
# it) or the flops of its zero-padded tiles at the kernel's rate, whichever is more: the kernel multiplies whole tiles, s
# and S rounded up to 4, s', S' and P to 16, which at S = s = 50 is 1.55 times the flops asked for.  The composition costs
# its five launches and the flops asked for at the rate it reaches above them (W, its transposed copy and T1 pass through
# HBM: that rate is a bandwidth, not the GEMM's peak).  Measured, kernel / composed: 0.043 / 0.108, 0.395 / 0.416,
# 2.11 / 2.87 ms, and 5.96 / 4.90 ms at S = s = 50, n = 42, P = 2500, where the kernel loses and the rule takes the
# composition.
_CLOSE_FLOOR_MS = 0.042          # one call at S = s = n = 20, P = 400
_CLOSE_TFLOPS = 12.6             # at S = s = 32, n = 200, P = 1024, where every tile is full (of padded flops: 10.6 at S = 8, s = 64; 13.6 at S = s = 50)
_CLOSE_LAUNCH_MS = 0.0215        # hadamard_product._LAUNCH_MS; the composed B at S = s = n = 20 takes 0.108 ms, 5.0 of these
_CLOSE_COMPOSED_LAUNCHES = 5     # see `_close_composed`
_CLOSE_GEMM_TFLOPS = 9.4         # the composed B at S = s = 32, n = 200, P = 1024 above its five launches, the lowest of three (12.1 at S = 8, s = 64; 11.0 at S = s = 50)


def _up(x: int, m: int) -> int:
    return -(-x // m) * m


def close_route_ms(S: int, S1: int, s: int, s1: int, n: int, P: int) -> Tuple[float, float]:
    """(kernel, composed) milliseconds the rule expects for one ``hadamard_close``"""
    flops = 2.0 * n * P * (S * s * s1 + S * S1 * s1)
    padded = 2.0 * n * _up(P, 16) * _up(S, 4) * _up(s1, 16) * (_up(s, 4) + _up(S1, 16))
    return (max(_CLOSE_FLOOR_MS, padded / (_CLOSE_TFLOPS * 1e9)),
            _CLOSE_COMPOSED_LAUNCHES * _CLOSE_LAUNCH_MS + flops / (_CLOSE_GEMM_TFLOPS * 1e9))


def close_layout(S: int, S1: int, s: int, s1: int, n: int, P: int) -> Tuple[int, int]:
    """(ichunks, doubles of the slab) of one ``ttsk_hadamard_close`` call"""
    out = nat.i64_array((0, 0))
    nat.call("ttsk_hadamard_close_layout", nat.i64_array((S, S1, s, s1, n, P)), out)
    return int(out[0]), int(out[1])


def _close_composed(Wl: DevArray, U: DevArray, V: DevArray, out: DevArray, accumulate: bool, stream: int) -> None:
    """B from `contract` calls, T1 through HBM.  The mode index i is the batch index of the first product and (gamma, p) its
    rows, which the one batch dimension of the strided GEMM reads only from a copy of W with (gamma, p, c) in one run; the
    second product sums over (i, gamma) and leaves gamma' last, a strided copy puts it before c'.  For (i, gamma) to be ONE
    contracted index of both operands U is copied mode-major, the smallest operand: with U as it lies the strided GEMM gets
    a two-level contracted index, and that came out wrong on the device at some shapes.  Five launches
    (six when it accumulates), whatever n is."""
    S, n, S1 = U.shape
    s, _, s1 = V.shape
    P = Wl.shape[2]
    Wt = DevArray.empty((n, S, P, s), stream=stream)
    copy_into(Wt, Wl.reshape(S, s, n, P).transpose(2, 0, 3, 1), stream)
    T1 = contract("igpc,cid->igpd", Wt, V, stream=stream)                # (n, S, P, s')
    Ut = U.transpose(1, 0, 2).contiguous(stream)                        # (n, S, S'): (i, gamma) one run, as in T1
    Gt = contract("igpd,igh->pdh", T1, Ut, stream=stream)               # (P, s', S'): (p, c') are the rows, the long side
    if accumulate:
        tmp = DevArray.empty((P, S1, s1), stream=stream)
        copy_into(tmp, Gt.transpose(0, 2, 1), stream)
        axpby(out, tmp.reshape(P, S1 * s1), 1.0, 1.0, stream)
    else:
        copy_into(out.reshape(P, S1, s1), Gt.transpose(0, 2, 1), stream)


def hadamard_close(Wl: DevArray, U: DevArray, V: DevArray, out: Optional[DevArray] = None, accumulate: bool = False,
                   stream: int = 0, route: Optional[str] = None) -> DevArray:
    """``out[p, gamma' s' + c'] (+)= sum_i sum_gamma U[gamma, i, gamma'] sum_c Wl[(gamma s + c), i, p] V[c, i, c']``, ``(P, S' s')``:
    ``Wl (S s, n, P)`` as ``hadamard_apply`` wrote it, taken through the cores ``U (S, n, S')`` and ``V (s, n, s')`` and summed
    over the mode.  The cores may be strided views.  ``route="kernel"`` is one ``ttsk_hadamard_close`` call, ``"composed"`` the
    same from `contract` calls, None (or ``paths.forced``) what ``close_route_ms`` expects to be faster."""
    route = resolve(route)
    S, n, S1 = U.shape
    s, nv, s1 = V.shape
    if nv != n:
        raise ValueError(f"cores {U.shape} and {V.shape} differ in their mode size")
    if Wl.ndim != 3 or Wl.shape[:2] != (S * s, n):
        raise ValueError(f"W of shape {Wl.shape}, expected {(S * s, n)} and the rank of the other product")
    P = int(Wl.shape[2])
    if out is None:
        out, accumulate = DevArray.empty((P, S1 * s1), stream=stream), False
    elif out.shape != (P, S1 * s1) or not out.is_contiguous():
        raise ValueError(f"out of shape {out.shape}, expected a contiguous {(P, S1 * s1)}")
    if route is None:
        route = taken(route, *close_route_ms(S, S1, s, s1, n, P))
    Wl = Wl.contiguous(stream)
    if route == "composed":
        _close_composed(Wl, U, V, out, accumulate, stream)
        return out
    _, slab = close_layout(S, S1, s, s1, n, P)
    work = DevArray.empty((slab,), stream=stream)
    nat.call("ttsk_hadamard_close", Wl, U, V, nat.i64_array((S, S1, s, s1, n, P)), nat.i64_array(tuple(U.strides) + tuple(V.strides)),
             out, 1 if accumulate else 0, work, slab, stream)
    return out


def _slices(n: int, row_doubles: int) -> List[Tuple[int, int]]:
    """the ranges of i of one mode: as many i as W_BUDGET_BYTES holds of ``row_doubles`` doubles each, at least one"""
    step = max(1, W_BUDGET_BYTES // (8 * row_doubles))
    return [(i0, min(n, i0 + step)) for i0 in range(0, n, step)]


def _check(a, b) -> None:
    if tuple(a.shape) != tuple(b.shape):
        raise ValueError(f"inner product of tensors of shapes {tuple(a.shape)} and {tuple(b.shape)}")


def _host_only(*trains) -> bool:
    return not any(_on_device(t) for t in trains)


def _scalar(G: DevArray) -> float:
    """the chain after the last mode is 1 x 1: read back"""
    return float(G.get().reshape(-1)[0])


def hadamard_tt_dot(hp: HadamardProduct, z: TensorTrain) -> float:
    """``<x o y, z>`` by the three-index chain.  With every factor on the host the recurrence runs in NumPy on the host cores
    and the device is not touched."""
    if not isinstance(hp, HadamardProduct) or not isinstance(z, TensorTrain):
        raise TypeError(f"hadamard_tt_dot: a HadamardProduct and a TensorTrain expected, got {type(hp).__name__} and {type(z).__name__}")
    _check(hp, z)
    if _host_only(hp.x, hp.y, z):
        G = np.ones((1, 1, 1))
        for X, Y, Z in zip(hp.x.cores, hp.y.cores, z.cores):
            W = np.einsum("bal,bik,aic->likc", G, _host(X), _host(Y), optimize=True)
            G = np.einsum("likc,lig->kcg", W, _host(Z), optimize=True)
        return float(G.reshape(-1)[0])
    xs, ys = hp.dev_parts()
    G = DevArray.from_host(np.ones((1, 1, 1)))
    for X, Y, Z in zip(xs, ys, z.dev_cores()):
        R1, r1, s, s1 = X.shape[2], Y.shape[2], Z.shape[0], Z.shape[2]
        Gn = DevArray.empty((R1 * r1, s1))
        for q, (i0, i1) in enumerate(_slices(X.shape[1], s * R1 * r1)):
            W = hadamard_apply(G, X[:, i0:i1, :], Y[:, i0:i1, :])
            # (gamma, i) is one contracted index of W; a copy of the core's slice makes it one of Z too (see `_close_composed`)
            contract("gip,gih->ph", W, Z[:, i0:i1, :].contiguous(), out=Gn, accumulate=q > 0)
        G = Gn.reshape(R1, r1, s1)
    return _scalar(G)


def hadamard_dot(hp: HadamardProduct, hq: HadamardProduct, route: Optional[str] = None) -> float:
    """``<x o y, u o v>`` by the four-index chain, halves A and B per mode.  ``route`` is the switch of ``paths.py`` for half B
    (``hadamard_close``); half A keeps the routing of ``hadamard_apply``.  With every factor on the host the recurrence runs
    in NumPy on the host cores and the device is not touched."""
    route = resolve(route)
    for t in (hp, hq):
        if not isinstance(t, HadamardProduct):
            raise TypeError(f"hadamard_dot: {type(t).__name__} is not a HadamardProduct")
    _check(hp, hq)
    if _host_only(hp.x, hp.y, hq.x, hq.y):
        G = np.ones((1, 1, 1, 1))
        for X, Y, U, V in zip(hp.x.cores, hp.y.cores, hq.x.cores, hq.y.cores):
            W = np.einsum("bagc,bik,aie->gcike", G, _host(X), _host(Y), optimize=True)
            G = np.einsum("gcike,gih,cid->kehd", W, _host(U), _host(V), optimize=True)
        return float(G.reshape(-1)[0])
    xs, ys = hp.dev_parts()
    us, vs = hq.dev_parts()
    G = DevArray.from_host(np.ones((1, 1, 1)))
    for X, Y, U, V in zip(xs, ys, us, vs):
        R1, r1, S, S1, s, s1 = X.shape[2], Y.shape[2], U.shape[0], U.shape[2], V.shape[0], V.shape[2]
        Gn = DevArray.empty((R1 * r1, S1 * s1))
        for q, (i0, i1) in enumerate(_slices(X.shape[1], S * s * R1 * r1)):
            W = hadamard_apply(G, X[:, i0:i1, :], Y[:, i0:i1, :])                           # half A, l = S s
            hadamard_close(W, U[:, i0:i1, :], V[:, i0:i1, :], out=Gn, accumulate=q > 0, route=route)    # half B
        G = Gn.reshape(R1, r1, S1 * s1)
    return _scalar(G)
