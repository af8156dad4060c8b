"""Inner products of operator-times-train products that are never formed: ``<M x, z>`` against a
train (``op_tt_dot``) and ``<M x, N y>`` against another product (``op_dot``), and with them the ``dot`` / ``norm`` /
``error(fast=True)`` of ``OperatorProduct`` and ``TTLinearMapSum.residual``.  Nothing of the size of a product core
``(R r) x n x (R' r')`` is formed, on the device or on the host.

Against a train ``z`` of ranks ``s`` the chain is ``G (R, r, s)``, ``G = 1`` before the first mode:

    W  = op_apply([G], [M_k], [C_k])                                   (s, n_out, R' r')
    G'[(beta' a'), g'] = sum_{g, i} W[g, i, (beta' a')] Z_k[g, i, g']                          one `contract`

Against a product ``N y``, ``N`` of ranks ``S`` with cores ``(S, n_in, n_out, S')`` and ``y`` of ranks ``s``, the chain is
``G (R, r, s, S)``, flattened with the train rank of ``y`` major, ``l = c S + gamma``, in two halves per mode:

    A.  Wl[(c S + gamma), i, p] = op_apply(L = G.reshape(R, r, s S), M_k, C_k)                 p = (beta' a')
    B.  G'[p, c' S' + gamma']   = sum_j sum_c Y_k[c, j, c'] sum_gamma sum_i Wl[(c S + gamma), i, p] N_k[gamma, j, i, gamma']

With ``c`` major the rows of ``Wl`` are ``(c, (gamma, i))``: the pair ``(gamma, i)`` that is contracted against ``N`` is one run, which is
what the stages of csrc/hadamard_stages.h walk, and ``G'`` comes out in the same ``(c', gamma')`` order for the next mode.  B is
``op_close``: one ``ttsk_op_close`` call (csrc/op_close.hip) or its composition from ``contract`` / ``copy_into`` calls.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from . import _native as nat
from .device import DevArray, axpby, contract, copy_into
from .hadamard_gram import _check, _scalar, _slices, _up
from .operator_product import OperatorProduct, chain_start, op_apply
from .paths import resolve, taken
from .tensor import TensorTrain, _host, _on_device

# The routing rule of half B.  The forms are those of ``hadamard_gram.close_route_ms``: a ttsk_op_close
# call costs its floor (the kernel and the ttsk_sum_slices behind it) or the flops of its zero-padded tiles at the kernel's
# rate, whichever is more: the kernel multiplies whole tiles, S n_out and s rounded up to 4, P, S' and s' to 16, so with
# S' <= 8 at least half of every gamma' tile is padding.  The composition costs its launches and the flops asked for at the
# rate it reaches above them; its two products are batched GEMMs of full tiles, which is why that rate is four times the one
# of ``hadamard_gram``'s composition.  The constants are measured on one MI355X (profiles/operator_gram_bench.json, the two
# shapes of step B alone).  Measured, kernel / composed: 0.032 / 0.107 ms at S = 4, s = n = 20, P = 80 (the TT-GMRES shape),
# where the kernel wins 3.3 times over, and 8.80 / 1.35 ms at S = 8, s = 64, n = 100, P = 512, where the kernel multiplies
# twice the flops asked for (S' = 8 in a tile of 16) at 10.3 TFLOP/s of them, loses 6.5 times over, and the rule takes the
# composition.  Two shapes fix the constants and no more: between them the rule is not measured.
_CLOSE_FLOOR_MS = 0.032          # one call at S = 4, s = n = 20, P = 80
_CLOSE_TFLOPS = 10.3             # of padded flops, at S = 8, s = 64, n = 100, P = 512
_CLOSE_LAUNCH_MS = 0.0267        # the composed B at S = 4, s = n = 20, P = 80 takes 0.107 ms, four of these
_CLOSE_COMPOSED_LAUNCHES = 4     # see `_close_composed`, with contiguous cores as `op_dot` has them
_CLOSE_GEMM_TFLOPS = 36.5        # the composed B at S = 8, s = 64, n = 100, P = 512 above its four launches


def close_route_ms(S: int, S1: int, s: int, s1: int, n_in: int, n_out: int, P: int) -> Tuple[float, float]:
    """(kernel, composed) milliseconds the rule expects for one ``op_close``"""
    flops = 2.0 * n_in * P * S1 * (s * S * n_out + s * s1)
    padded = 2.0 * n_in * _up(P, 16) * _up(S1, 16) * (s * _up(S * n_out, 4) + _up(s, 4) * _up(s1, 16))
    return (max(_CLOSE_FLOOR_MS, padded / (_CLOSE_TFLOPS * 1e9)),
            _CLOSE_COMPOSED_LAUNCHES * _CLOSE_LAUNCH_MS + flops / (_CLOSE_GEMM_TFLOPS * 1e9))


def close_layout(S: int, S1: int, s: int, s1: int, n_in: int, n_out: int, P: int) -> Tuple[int, int]:
    """(jchunks, doubles of the slab) of one ``ttsk_op_close`` call"""
    out = nat.i64_array((0, 0))
    nat.call("ttsk_op_close_layout", nat.i64_array((S, S1, s, s1, n_in, n_out, P)), out)
    return int(out[0]), int(out[1])


def one_run(N) -> bool:
    """whether ``(gamma, i)`` of an operator core ``(S, n_in, n_out, S')`` is one run, as ``ttsk_op_close`` reads it (an extent of
    1 leaves the other index's stride as the run's)"""
    S, _, n_out, _ = N.shape
    return S == 1 or n_out == 1 or N.strides[0] == n_out * N.strides[2]


def pack(N: DevArray, stream: int = 0) -> DevArray:
    """the core with ``(gamma, i)`` one run: itself where it is, else a contiguous ``(S, n_out, n_in, S')`` copy -- the core of
    ``mpo.T`` -- viewed as ``(S, n_in, n_out, S')``"""
    return N if one_run(N) else N.transpose(0, 2, 1, 3).contiguous(stream).transpose(0, 2, 1, 3)


def packed_views(mpo) -> List[DevArray]:
    """``pack`` of every resident core of the operator, made once per list of cores (keyed by their identity, as
    ``MPO.dev_views`` is): a second product with the same operator packs nothing."""
    key = getattr(mpo, "_packed_key", None)
    if key is None or len(key) != len(mpo.cores) or not all(a is b for a, b in zip(key, mpo.cores)):
        mpo._packed = [pack(c) for c in mpo.dev_views()]
        mpo._packed_key = tuple(mpo.cores)
    return mpo._packed


def _close_composed(Wl: DevArray, N: DevArray, Y: DevArray, out: DevArray, accumulate: bool, stream: int) -> None:
    """B from `contract` calls, T1 through HBM: first ``(gamma, i)`` against N, one contracted run of both operands (N is packed),
    batched over c; then ``(c, j)`` against Y.  For ``(c, j)`` to be ONE contracted index of both operands T1 is copied with j
    next to c and Y is taken contiguous: a two-level contracted index is what ``hadamard_gram._close_composed`` avoids too.
    The second product leaves gamma' before c', a strided copy puts it behind.  Five launches (four where Y is contiguous, one
    more when it accumulates, one more for an N with padding between its runs), whatever n_in is."""
    S, n_in, n_out, S1 = N.shape
    s, _, s1 = Y.shape
    P = Wl.shape[2]
    Nk = N.transpose(0, 2, 1, 3).contiguous(stream).reshape(S * n_out, n_in, S1)        # a packed core as it lies; a padded one is copied
    T1 = contract("ckp,kjh->cpjh", Wl.reshape(s, S * n_out, P), Nk, stream=stream)       # (s, P, n_in, S')
    T1t = DevArray.empty((s, n_in, P, S1), stream=stream)
    copy_into(T1t, T1.transpose(0, 2, 1, 3), stream)
    Gt = contract("cjph,cjd->phd", T1t, Y.contiguous(stream), stream=stream)            # (P, S', s'): (p, gamma') are the rows
    if accumulate:
        tmp = DevArray.empty((P, s1, S1), stream=stream)
        copy_into(tmp, Gt.transpose(0, 2, 1), stream)
        axpby(out, tmp.reshape(P, s1 * S1), 1.0, 1.0, stream)
    else:
        copy_into(out.reshape(P, s1, S1), Gt.transpose(0, 2, 1), stream)


def op_close(Wl: DevArray, N: DevArray, Y: DevArray, out: Optional[DevArray] = None, accumulate: bool = False,
             stream: int = 0, route: Optional[str] = None) -> DevArray:
    """``out[p, c' S' + gamma'] (+)= sum_j sum_c Y[c, j, c'] sum_{gamma, i} Wl[(c S + gamma), i, p] N[gamma, j, i, gamma']``, ``(P, s' S')``:
    ``Wl (s S, n_out, P)`` as ``op_apply`` wrote it, taken through the operator core ``N (S, n_in, n_out, S')`` and the train core
    ``Y (s, n_in, s')`` and summed over both mode indices.  The cores may be strided views; an N whose ``(gamma, i)`` is not one
    run is packed first (``pack``).  ``route="kernel"`` is one ``ttsk_op_close`` call, ``"composed"`` the same from `contract`
    calls, None (or ``paths.forced``) what ``close_route_ms`` expects to be faster."""
    route = resolve(route)
    if N.ndim != 4 or Y.ndim != 3:
        raise ValueError(f"an operator core (S, n_in, n_out, S') and a train core (s, n_in, s') expected, got {N.shape} and {Y.shape}")
    S, n_in, n_out, S1 = N.shape
    s, ny, s1 = Y.shape
    if ny != n_in:
        raise ValueError(f"operator core {N.shape} does not act on a train core {Y.shape}")
    if Wl.ndim != 3 or Wl.shape[:2] != (s * S, n_out):
        raise ValueError(f"W of shape {Wl.shape}, expected {(s * S, n_out)} and the rank of the other product")
    P = int(Wl.shape[2])
    if out is None:
        out, accumulate = DevArray.empty((P, s1 * S1), stream=stream), False
    elif out.shape != (P, s1 * S1) or not out.is_contiguous():
        raise ValueError(f"out of shape {out.shape}, expected a contiguous {(P, s1 * S1)}")
    if route is None:
        route = taken(route, *close_route_ms(S, S1, s, s1, n_in, n_out, P))
    Wl = Wl.contiguous(stream)
    N = pack(N, stream)
    if route == "composed":
        _close_composed(Wl, N, Y, out, accumulate, stream)
        return out
    _, slab = close_layout(S, S1, s, s1, n_in, n_out, P)
    work = DevArray.empty((slab,), stream=stream)
    nat.call("ttsk_op_close", Wl, N, Y, nat.i64_array((S, S1, s, s1, n_in, n_out, P)), nat.i64_array(tuple(N.strides) + tuple(Y.strides)),
             out, 1 if accumulate else 0, work, slab, stream)
    return out


def _mpo_on_device(mpo) -> bool:
    return mpo.resident() or any(isinstance(c, DevArray) for c in mpo.cores)


def _host_only(*products) -> bool:
    """no factor of any product (an ``OperatorProduct`` or a ``TensorTrain``) lives in HBM"""
    for t in products:
        if isinstance(t, OperatorProduct):
            if _mpo_on_device(t.mpo) or _on_device(t.tt):
                return False
        elif _on_device(t):
            return False
    return True


def op_tt_dot(op: OperatorProduct, z: TensorTrain) -> float:
    """``<M x, z>`` by the three-index chain.  With every factor on the host the recurrence runs in NumPy on the host cores
    and the device is not touched."""
    if not isinstance(op, OperatorProduct) or not isinstance(z, TensorTrain):
        raise TypeError(f"op_tt_dot: an OperatorProduct and a TensorTrain expected, got {type(op).__name__} and {type(z).__name__}")
    _check(op, z)
    if _host_only(op, z):
        G = np.ones((1, 1, 1))
        for M, C, Z in zip(op.mpo.cores, op.tt.cores, z.cores):
            W = np.einsum("bal,bjik,ajc->likc", G, _host(M), _host(C), optimize=True)
            G = np.einsum("likc,lig->kcg", W, _host(Z), optimize=True)
        return float(G.reshape(-1)[0])
    Ms, Cs = op.dev_parts()
    G = chain_start()
    for M, C, Z in zip(Ms, Cs, z.dev_cores()):
        R1, r1, s, s1 = M.shape[3], C.shape[2], Z.shape[0], Z.shape[2]
        Gn = DevArray.empty((R1 * r1, s1))
        for q, (i0, i1) in enumerate(_slices(M.shape[2], s * R1 * r1)):
            W, _ = op_apply([G], [M[:, :, i0:i1, :]], [C])
            # (g, i) is one contracted index of W; a copy of the core's slice makes it one of Z too
            contract("gip,gih->ph", W, Z[:, i0:i1, :].contiguous(), out=Gn, accumulate=q > 0)
        G = Gn.reshape(R1, r1, s1)
    return _scalar(G)


def op_dot(op: OperatorProduct, oq: OperatorProduct, route: Optional[str] = None) -> float:
    """``<M x, N y>`` by the four-index chain, halves A and B per mode.  ``route`` is the switch of ``paths.py`` for half B
    (``op_close``); half A keeps the routing of ``op_apply``.  The cores of N are packed once per operator
    (``packed_views``).  With every factor on the host the recurrence runs in NumPy on the host cores and the device is not
    touched."""
    route = resolve(route)
    for t in (op, oq):
        if not isinstance(t, OperatorProduct):
            raise TypeError(f"op_dot: {type(t).__name__} is not an OperatorProduct")
    _check(op, oq)
    if _host_only(op, oq):
        G = np.ones((1, 1, 1, 1))
        for M, C, N, Y in zip(op.mpo.cores, op.tt.cores, oq.mpo.cores, oq.tt.cores):
            W = np.einsum("bacg,bjik,aje->cgike", G, _host(M), _host(C), optimize=True)
            G = np.einsum("cgike,gjih,cjd->kedh", W, _host(N), _host(Y), optimize=True)
        return float(G.reshape(-1)[0])
    Ms, Cs = op.dev_parts()
    Ns, Ys = packed_views(oq.mpo), oq.tt.dev_cores()
    G = chain_start()
    for M, C, N, Y in zip(Ms, Cs, Ns, Ys):
        R1, r1, S, S1, s, s1 = M.shape[3], C.shape[2], N.shape[0], N.shape[3], Y.shape[0], Y.shape[2]
        Gn = DevArray.empty((R1 * r1, s1 * S1))
        cuts = _slices(M.shape[2], s * S * R1 * r1)
        for q, (i0, i1) in enumerate(cuts):
            whole = len(cuts) == 1                                      # a slice of i of a packed core is not one run: packed again
            W, _ = op_apply([G], [M if whole else M[:, :, i0:i1, :]], [C])                 # half A, l = s S
            op_close(W, N if whole else N[:, :, i0:i1, :], Y, out=Gn, accumulate=q > 0, route=route)      # half B
        G = Gn.reshape(R1, r1, s1 * S1)
    return _scalar(G)
