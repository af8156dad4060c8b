"""Evaluation of a ``TensorTrain`` / ``CPTensor`` at index lists: the device pass of ``csrc/tt_gather.hip``
(``ttsk_tt_gather`` / ``ttsk_cp_gather``) and, for train ranks beyond its cover, the chain from
``ttsk_sparse_ttdrm_step``.  Of a ``TuckerTensor``: ``ttsk_tucker_gather`` (``csrc/tucker_gather.hip``)
and, beyond its cover or under ``route="composed"``, column gathers of the factors and batched ``contract`` calls
(DESIGN section 20).

Entry point: ``_gather_device``, which ``gather_dev`` / ``support_error`` of the two classes and ``SparseTensor.dot``
call.  ``_PANEL_BYTES`` is the memory budget of the composed fallback.
"""
from __future__ import annotations

import numpy as np

from .device import DevArray, axpby, contract, copy_into
from .paths import resolve
from .tensor import SparseTensor, TensorTrain, TuckerTensor

_PANEL_BYTES = 256 << 20      # composed fallback: the two (chunk x rank) panels of a step stay below this
_GEMM_MAX_BATCH = 65535       # problems of one ``ttsk_gemm`` call: the Tucker composition's tuples ride in its batch index


def _gather_indices(idx, shape):
    """The index argument of ``gather_dev`` as (device index matrix, row stride, row order, N, device entries or None).
    A ``SparseTensor`` is read in place (``.T`` views through their row order); host arrays are checked against
    ``shape`` here, before anything is uploaded."""
    d = len(shape)
    if isinstance(idx, SparseTensor):
        if tuple(idx.shape) != tuple(shape):
            raise ValueError(f"gather: index tensor of shape {idx.shape}, tensor of shape {tuple(shape)}")
        return idx.dev_indices(), idx.nnz, tuple(idx.dev_row_order), idx.nnz, idx.dev_entries()
    arr = np.stack(idx) if isinstance(idx, (tuple, list)) else np.asarray(idx)
    if arr.ndim != 2 or arr.shape[0] != d:
        raise ValueError(f"gather: {d} index rows expected, got an array of shape {arr.shape}")
    arr = np.ascontiguousarray(arr, dtype=np.int64)
    if arr.size and (arr.min() < 0 or (arr.max(axis=1) >= np.asarray(shape, dtype=np.int64)).any()):
        raise IndexError(f"gather: an index lies outside the shape {tuple(shape)}")
    return DevArray.from_host(arr, dtype=np.int64), arr.shape[1], tuple(range(d)), arr.shape[1], None


def _tt_gather_composed(cores, dev_idx, stride, order, N, val, want_out, want_stats):
    """The chain from ``ttsk_sparse_ttdrm_step``, mode by mode, for ranks beyond the fused kernel's cover: chunks of the
    list small enough for the panel budget, the statistics from device products summed over the chunks in order."""
    from . import _native as nat
    widest = max(max(c.shape[0], c.shape[2]) for c in cores)
    chunk = max(1, _PANEL_BYTES // (16 * widest))
    out = DevArray.empty((N,)) if want_out else None
    stats = np.zeros(3) if want_stats else None
    for lo in range(0, N, chunk):
        m = min(chunk, N - lo)
        v = None
        for k, c in enumerate(cores):
            rho, n, rhop = c.shape
            nxt = DevArray.empty((m, rhop))
            nat.call("ttsk_sparse_ttdrm_step", v, rho, c, n, rhop, dev_idx[order[k], lo:lo + m], m, nxt, 0)
            v = nxt
        if want_out:
            copy_into(out[lo:lo + m], v.reshape(m))
        if want_stats:
            _chunk_stats(stats, v, val[lo:lo + m].reshape(m, 1))
    return out, stats


def _chunk_stats(stats, v, x):
    """adds (x . v, v . v, |v - x|^2) of a chunk, ``v`` and ``x`` device arrays (m, 1), to the host sums"""
    res = v.copy()
    axpby(res, x, -1.0, 1.0)                                           # v - x
    for j, (a, b) in enumerate(((x, v), (v, v), (res, res))):
        stats[j] += float(contract("ka,kb->ab", a, b).get()[0, 0])


def _tucker_gather_composed(factors, core, shape, dev_idx, stride, order, N, val, want_out, want_stats):
    """A Tucker tensor at an index list without the fused kernel: per mode the columns ``U_k[:, i_k(e)]`` by
    ``ttsk_sparse_densedrm_gather`` (one index row, ``m = 1``), the core contracted with them mode by mode with the tuple
    as the batch index.  Chunks of the list keep the widest panel (chunk x prod_{k >= 1} s_k) under ``_PANEL_BYTES`` and the
    batch of a ``contract`` call under ``_GEMM_MAX_BATCH``."""
    import ctypes
    from . import _native as nat
    ranks, d = core.shape, len(shape)
    rest = core.size // ranks[0]
    chunk = max(1, min(_GEMM_MAX_BATCH, _PANEL_BYTES // (16 * max(rest, max(ranks)))))
    out = DevArray.empty((N,)) if want_out else None
    stats = np.zeros(3) if want_stats else None
    for lo in range(0, N, chunk):
        m = min(chunk, N - lo)
        cols = []
        for k in range(d):
            G = DevArray.empty((m, ranks[k]))
            nat.call("ttsk_sparse_densedrm_gather", factors[k], ranks[k], shape[k], dev_idx[:, lo:lo + m], stride,
                     (ctypes.c_int * 1)(order[k]), nat.i64_array(shape[k:k + 1]), 1, m, G, 0)
            cols.append(G)
        v = contract("es,sr->er", cols[0], core.reshape(ranks[0], rest))
        for k in range(1, d):
            v = contract("esr,es->er", v.reshape(m, ranks[k], -1), cols[k])
        if want_out:
            copy_into(out[lo:lo + m], v.reshape(m))
        if want_stats:
            _chunk_stats(stats, v, val[lo:lo + m].reshape(m, 1))
    return out, stats


def _tucker_gather(tensor, dev_idx, stride, order, N, val, want_out, want_stats, route):
    import ctypes
    from . import _native as nat
    d = tensor.ndim
    factors = [U.contiguous() for U in tensor.dev_parts()[0]]
    core = tensor.dev_core_contiguous()
    if route != "composed":
        out = DevArray.empty((N,)) if want_out else None
        stats = DevArray.empty((3,)) if want_stats else None
        try:
            nat.call("ttsk_tucker_gather", core, nat.ptr_array(factors), nat.i64_array(tensor.rank), nat.i64_array(tensor.shape), d,
                     dev_idx, stride, (ctypes.c_int * d)(*order), N, val if want_stats else None, out, stats, 0)
            return out, (stats.get() if want_stats else None)
        except nat.TtskUnsupported:
            if route == "kernel":
                raise
    return _tucker_gather_composed(factors, core, tensor.shape, dev_idx, stride, order, N, val, want_out, want_stats)


def _gather_device(tensor, idx, want_out: bool, want_stats: bool, route=None):
    """One pass of ``ttsk_tt_gather`` / ``ttsk_cp_gather`` / ``ttsk_tucker_gather`` over an index list: (DevArray (N,) or
    None, the three sums (x . t, t . t, |t - x|^2) as a host array or None).  Nothing of the tensor or the list is
    downloaded.  ``route``: the switch of ``paths.py``, for a ``TuckerTensor``."""
    import ctypes
    from . import _native as nat
    route = resolve(route)
    dev_idx, stride, order, N, val = _gather_indices(idx, tensor.shape)
    if want_stats and val is None:
        raise ValueError("gather: the sums need the entries of a SparseTensor")
    d = tensor.ndim
    if isinstance(tensor, TuckerTensor):
        return _tucker_gather(tensor, dev_idx, stride, order, N, val, want_out, want_stats, route)
    cores = [c.contiguous() for c in tensor.dev_cores()]
    out = DevArray.empty((N,)) if want_out else None
    stats = DevArray.empty((3,)) if want_stats else None
    tail = (dev_idx, stride, (ctypes.c_int * d)(*order), N, val if want_stats else None, out, stats, 0)
    cptr = nat.ptr_array(cores)
    shape = nat.i64_array(tensor.shape)
    if isinstance(tensor, TensorTrain):
        ranks = nat.i64_array([c.shape[0] for c in cores] + [cores[-1].shape[2]])
        try:
            nat.call("ttsk_tt_gather", cptr, ranks, shape, d, *tail)
        except nat.TtskUnsupported:
            return _tt_gather_composed(cores, dev_idx, stride, order, N, val, want_out, want_stats)
    else:
        nat.call("ttsk_cp_gather", cptr, tensor.rank, shape, d, *tail)
    return out, (stats.get() if want_stats else None)
