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

``op_gram`` is the Gram matrix of lists of products and trains: every pair advances through a mode in
the same launches -- one ``op_apply`` per distinct ``l`` with the pairs as its terms, one ``ttsk_op_close_batch`` call for
half B of all of them (``close_batch``) -- and all closing scalars are read back once.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence, Tuple

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


# ---- the Gram matrix of lists of products and trains: every pair advances through a mode together
MAX_PAIRS = 23          # OP_CLOSE_MAX_PAIRS of csrc/op_close_batch_plan.h: the pairs of one ttsk_op_close_batch call


def close_batch(Wls: Sequence[DevArray], Ns: Sequence[DevArray], Ys: Sequence[DevArray], outs: Sequence[DevArray],
                accumulate: bool = False, stream: int = 0) -> None:
    """Half B of many pairs: ``outs[p] (+)=`` what ``op_close`` makes of ``Wls[p]``, ``Ns[p]`` and ``Ys[p]``, by one
    ``ttsk_op_close_batch`` call per ``MAX_PAIRS`` pairs and with the bits of that pair's ``ttsk_op_close`` call.  A
    ``Wls[p] (s S, n_out, P)`` is read in place: a column slice of the W of a many-term ``op_apply`` (rows one pitch apart,
    columns next to each other).  Every N is one run already (``pack``); the ``outs`` are contiguous ``(P, s' S')`` and do not
    overlap."""
    for a in range(0, len(Wls), MAX_PAIRS):
        b = min(a + MAX_PAIRS, len(Wls))
        dims, strides, ldws = [], [], []
        for Wl, N, Y, out in zip(Wls[a:b], Ns[a:b], Ys[a:b], outs[a:b]):
            S, n_in, n_out, S1 = N.shape
            s, ny, s1 = Y.shape
            P = int(Wl.shape[2])
            ldw = Wl.strides[1] if n_out > 1 else (Wl.strides[0] if s * S > 1 else P)
            if ny != n_in or Wl.shape[:2] != (s * S, n_out) or (P > 1 and Wl.strides[2] != 1) or (s * S > 1 and Wl.strides[0] != n_out * ldw):
                raise ValueError(f"W of shape {Wl.shape} and strides {Wl.strides} against cores {N.shape} and {Y.shape}")
            if out.shape != (P, s1 * S1) or not out.is_contiguous():
                raise ValueError(f"out of shape {out.shape}, expected a contiguous {(P, s1 * S1)}")
            dims += [S, S1, s, s1, n_in, n_out, P]
            strides += list(N.strides) + list(Y.strides)
            ldws.append(ldw)
        n = b - a
        offs = nat.i64_array([0] * (n + 1))
        nat.call("ttsk_op_close_batch_layout", n, nat.i64_array(dims), offs)
        slab = int(offs[n])
        work = DevArray.empty((slab,), stream=stream)
        nat.call("ttsk_op_close_batch", n, nat.ptr_array(Wls[a:b]), nat.ptr_array(Ns[a:b]), nat.ptr_array(Ys[a:b]), nat.i64_array(dims),
                 nat.i64_array(strides), nat.i64_array(ldws), nat.ptr_array(outs[a:b]), 1 if accumulate else 0, work, slab, stream)


def tt_close_route_ms(s: int, s1: int, n: int, P: int, alone: bool = False) -> Tuple[float, float]:
    """(in the batch, its own `contract`) milliseconds expected for closing a mode against a train core ``Z (s, n, s')``.  In
    the batch the pair is the degenerate one of ``_Side.right`` (``S = s``, ``s = n_in = 1``): it pays no launch of its own
    unless it is ``alone`` there, but with one row of ``c`` stage 1 has ONE tile per chunk, which one wave of the four forms
    (csrc/hadamard_stages.h), so its padded flops count four times, and stage 2 multiplies a padded 4 x 16 block by the one.
    The `contract` is one launch and the flops asked for.  Constants: those of ``close_route_ms``; measured at both shapes
    in profiles/operator_gram_batch_bench.json (``close_train``)."""
    padded = 2.0 * _up(P, 16) * _up(s1, 16) * (4 * _up(s * n, 4) + 4 * 16)
    return (max(_CLOSE_FLOOR_MS if alone else 0.0, padded / (_CLOSE_TFLOPS * 1e9)),
            _CLOSE_LAUNCH_MS + 2.0 * P * s1 * s * n / (_CLOSE_GEMM_TFLOPS * 1e9))


def _host_dot(a, b) -> float:
    """one pair on host factors: the NumPy recurrences"""
    if isinstance(a, OperatorProduct):
        return op_dot(a, b) if isinstance(b, OperatorProduct) else op_tt_dot(a, b)
    return op_tt_dot(b, a) if isinstance(b, OperatorProduct) else float(a.dot(b))


class _Step(NamedTuple):
    """one pair at one mode: the cores of half A (M, C) and of half B (N, Y), P = R' r', the columns s' S' of its G', and
    whether it closes in the batch"""
    M: DevArray
    C: DevArray
    N: DevArray
    Y: DevArray
    P: int
    cols: int
    kernel: Optional[bool]


class _Side:
    """a member's cores as one side of a pair reads them, fetched once per member"""

    def __init__(self, t) -> None:
        self.t = t
        self.product = isinstance(t, OperatorProduct)
        self._left = self._right = None

    def left(self) -> Tuple[List[DevArray], List[DevArray]]:
        """(operator cores, train cores) that half A carries the chain through"""
        if self._left is None:
            self._left = self.t.dev_parts()
        return self._left

    def right(self) -> Tuple[List[DevArray], List[DevArray]]:
        """(N, Y) per mode for half B.  A train z is the product of its cores Z (s, n, s') viewed as operator cores
        (S = s, n_in = 1, n_out = n, S' = s'), one run as a contiguous core lies, with the train of ones: stage 2 multiplies
        by exactly 1."""
        if self._right is None:
            if self.product:
                self._right = (packed_views(self.t.mpo), self.t.tt.dev_cores())
            else:
                cores = [c.contiguous() for c in self.t.dev_cores()]
                self._right = ([c.reshape(c.shape[0], 1, c.shape[1], c.shape[2]) for c in cores], [chain_start()] * len(cores))
        return self._right


def _device_gram(As, Bs, todo, sym: bool, route: Optional[str], G: np.ndarray) -> None:
    from .tensor_gram import _GRAM_MAX_TRAINS, _gram_pass, tt_gram
    sides_a = [_Side(t) for t in As]
    sides_b = sides_a if sym else [_Side(t) for t in Bs]
    # a pair (p, q, left, right): the left side is a product, carried by half A; a train on the left is the swapped pair
    pairs = []
    for p, q in todo:
        a, b = sides_a[p], sides_b[q]
        if a.product or b.product:
            pairs.append((p, q, a, b) if a.product else (p, q, b, a))
    ta = [p for p, a in enumerate(sides_a) if not a.product]
    tb = ta if sym else [q for q, b in enumerate(sides_b) if not b.product]
    block = len(ta) * len(tb)                                          # the train-train pairs: one tt_gram block
    d = len(As[0].shape)
    chains = [chain_start()] * len(pairs)                              # G_pq (R, r, s S) of every pair, side by side
    Gn, offs, at = None, [], 0
    for k in range(d):
        n_out = int(As[0].shape[k])
        parts, at = [], 0
        offs = []
        for (_, _, a, b), L in zip(pairs, chains):
            M, C = a.left()[0][k], a.left()[1][k]
            N, Y = b.right()[0][k], b.right()[1][k]
            P, cols = M.shape[3] * C.shape[2], Y.shape[2] * N.shape[3]
            dims = (N.shape[0], N.shape[3], Y.shape[0], Y.shape[2], N.shape[1], n_out, P)
            if route is not None:
                kernel = route == "kernel"
            elif b.product:
                kernel = taken(None, *close_route_ms(*dims)) == "kernel"
            else:
                kernel = None                                           # a train: decided below, once the product pairs are
            parts.append(_Step(M, C, N, Y, P, cols, kernel))
            offs.append(at)
            at += _up(P * cols, 2)                                     # every pair's G' starts on 16 bytes
        riding = any(pt.kernel for pt in parts)                         # the batch has a launch that a train's pair can ride on
        parts = [pt if pt.kernel is not None else
                 pt._replace(kernel=taken(None, *tt_close_route_ms(pt.N.shape[0], pt.N.shape[3], n_out, pt.P, alone=not riding)) == "kernel")
                 for pt in parts]
        # the G' of all pairs are slices of one allocation; behind the last mode they are the closing scalars, and the
        # block of the train-train pairs joins them: one read-back for everything
        Gn = DevArray.empty((at + (block if k == d - 1 else 0),))
        outs = [Gn[o:o + pt.P * pt.cols].reshape(pt.P, pt.cols) for o, pt in zip(offs, parts)]
        cuts = _slices(n_out, max(1, sum(L.shape[2] * pt.P for L, pt in zip(chains, parts))))
        whole = len(cuts) == 1                                          # a slice of i of a packed core is not one run: packed again
        for c, (i0, i1) in enumerate(cuts):
            batch = [x for x, pt in enumerate(parts) if pt.kernel]
            # ---- half A of the batch: one op_apply per l, the pairs (of one chain and one left product: once) as its terms
            Wls = {}
            for l in sorted({chains[x].shape[2] for x in batch}):
                terms, Ls, Ms, Cs = {}, [], [], []
                for x in batch:
                    if chains[x].shape[2] == l and (id(chains[x]), id(pairs[x][2])) not in terms:
                        terms[(id(chains[x]), id(pairs[x][2]))] = len(Ls)
                        Ls.append(chains[x])
                        Ms.append(parts[x].M if whole else parts[x].M[:, :, i0:i1, :])
                        Cs.append(parts[x].C)
                W, woffs = op_apply(Ls, Ms, Cs, route=route)
                W = W.contiguous()
                for x in batch:
                    if chains[x].shape[2] == l:
                        o = woffs[terms[(id(chains[x]), id(pairs[x][2]))]]
                        Wls[x] = W[:, :, o:o + parts[x].P]
            # ---- half B of the batch: every pair's Wl in place in the W of its l
            if batch:
                close_batch([Wls[x] for x in batch], [parts[x].N if whole else pack(parts[x].N[:, :, i0:i1, :]) for x in batch],
                            [parts[x].Y for x in batch], [outs[x] for x in batch], accumulate=c > 0)
            # ---- the others pair by pair, as op_dot and op_tt_dot compose them
            for x, (M, C, N, Y, P, cols, kernel) in enumerate(parts):
                if kernel:
                    continue
                W, _ = op_apply([chains[x]], [M if whole else M[:, :, i0:i1, :]], [C], route=route)
                if pairs[x][3].product:
                    op_close(W, N if whole else N[:, :, i0:i1, :], Y, out=outs[x], accumulate=c > 0, route="composed")
                else:                                                   # against a train: (g, i) one contracted index of W and of Z
                    Z = N.reshape(N.shape[0], N.shape[2], N.shape[3])
                    contract("gip,gih->ph", W, Z[:, i0:i1, :].contiguous(), out=outs[x], accumulate=c > 0)
        chains = [o.reshape(pt.M.shape[3], pt.C.shape[2], pt.cols) for o, pt in zip(outs, parts)]
    # ---- the train-train block
    tt_host = None
    if block:
        TA, TB = [As[p] for p in ta], [Bs[q] for q in tb]
        if Gn is None:
            Gn, at = DevArray.empty((block,)), 0
        if not (len(TA) + len(TB) <= _GRAM_MAX_TRAINS and _gram_pass(TA, TB, sym, route, Gn[at:at + block].reshape(len(ta), len(tb)))):
            tt_host = tt_gram(TA, None if sym else TB, route=route)
    flat = Gn.get()                                                     # the one read-back
    for (p, q, _, _), o in zip(pairs, offs):
        G[p, q] = flat[o]
    if block:
        G[np.ix_(ta, tb)] = flat[at:at + block].reshape(len(ta), len(tb)) if tt_host is None else tt_host


def op_gram(As, Bs=None, route: Optional[str] = None) -> np.ndarray:
    """``G[p, q] = <As[p], Bs[q]>`` as a ``(K, M)`` array for lists of ``OperatorProduct``s and ``TensorTrain``s of one shape
    (``Bs=None``: the symmetric Gram of ``As``, its upper triangle computed and mirrored).  No product is formed.

    Train-train pairs are one ``tt_gram`` block.  Every other pair carries its chain through the modes side by side with the
    others: per mode one ``op_apply`` per distinct ``l`` with the pairs as its terms, then ONE ``ttsk_op_close_batch`` call
    that reads every pair's ``Wl`` in place (``close_batch``); a product against a train rides along as the degenerate pair
    of ``_Side.right``.  All closing scalars lie in one device array and are read once.  A pair in the batch gets the bits
    ``op_dot`` gives it on the kernel route.

    ``route`` is the switch of ``paths.py``: None sends the pairs for which ``close_route_ms`` names the kernel into the
    batch and composes the others pair by pair as ``op_dot`` / ``op_tt_dot`` do; ``"kernel"`` sends every pair into the
    batch and half A to ``ttsk_op_apply``, with the entries' ``TtskUnsupported`` where they refuse; ``"composed"`` calls no
    entry of the batch.  With every factor of every member on the host the NumPy recurrences run pair by pair and the device
    is not touched."""
    route = resolve(route)
    As = list(As)
    sym = Bs is None
    Bs = As if sym else list(Bs)
    if not As or not Bs:
        raise ValueError("op_gram: an empty list")
    for t in As + ([] if sym else Bs):
        if not isinstance(t, (OperatorProduct, TensorTrain)):
            raise TypeError(f"op_gram: {type(t).__name__} is neither an OperatorProduct nor a TensorTrain")
        _check(As[0], t)
    G = np.empty((len(As), len(Bs)))
    todo = [(p, q) for p in range(len(As)) for q in range(len(Bs)) if not sym or q >= p]
    if _host_only(*As, *Bs):
        for p, q in todo:
            G[p, q] = _host_dot(As[p], Bs[q])
    else:
        _device_gram(As, Bs, todo, sym, route, G)
    if sym:
        for p, q in todo:
            G[q, p] = G[p, q]
    return G
