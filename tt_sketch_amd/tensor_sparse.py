"""A ``SparseTensor`` against another explicit tensor: the sorted-key join of ``csrc/sparse_join.hip``
(``ttsk_sparse_key_index`` / ``ttsk_sparse_join`` / ``ttsk_dense_join``).

Entry points: ``_key_index`` (the index of a table tensor, built once per tensor and row order), ``_sparse_join`` and
``_dense_join`` (one lookup pass each), which ``SparseTensor.dot`` / ``gather`` / ``gather_dev`` call.
"""
from __future__ import annotations

import ctypes

import numpy as np

from .device import DevArray
from .paths import resolve, taken
from .tensor import DenseTensor, SparseTensor
from .tensor_gather import _gather_indices

# The routing rule of DESIGN section 19, its constants measured on one MI355X (profiles/sparse_join_bench.json): a join
# call with its read-back and the first call's index build against the host path's dict of the table and its Python loop
# over the queries.  Both sides grow linearly; the device's slope is a hundredth of the host's and is left out.
_JOIN_CALL_MS = 0.05         # one ttsk_sparse_join call and the read-back of its result
_JOIN_INDEX_MS = 0.1         # the first call on a table: ttsk_sparse_key_index into pooled buffers (a fresh allocation: 2-4 ms, once)
_HOST_TABLE_MS = 1.2e-4      # per nonzero of the table that enters the dict (once per tensor: it is cached)
_HOST_QUERY_MS = 1.0e-4      # per query looked up


def _join_route_ms(table: SparseTensor, nq: int):
    """(time of the device join, time of the host path) in ms for ``nq`` queries against ``table`` as both stand now:
    with or without the index, with or without the dict."""
    indexed = table._dev is not None and ("key_index", tuple(table.dev_row_order)) in table._dev[2]
    return (_JOIN_CALL_MS + (0.0 if indexed else _JOIN_INDEX_MS),
            _HOST_QUERY_MS * nq + (0.0 if "dict" in table.__dict__ else _HOST_TABLE_MS * table.nnz))


def _join_routed(table: SparseTensor, nq: int, route) -> bool:
    """Whether a lookup in ``table`` takes the device join: ``route`` as in ``paths.py`` (``"composed"`` is the host
    path), None the rule above."""
    route = resolve(route)
    return taken(route, *_join_route_ms(table, nq)) == "kernel" if route is None else route == "kernel"


def _layout(n_table: int, nq: int = 0) -> dict:
    """The plan's numbers for a table of ``n_table`` nonzeros and ``nq`` queries on this device."""
    from . import _native as nat
    out = (ctypes.c_int64 * 8)()
    nat.call("ttsk_sparse_join_layout", n_table, nq, 0, out)
    names = ("max_split", "stride", "n_split", "lds_steps", "seg_steps", "grid", "run", "depth")
    return dict(zip(names, (int(v) for v in out)))


def _key_index(sp: SparseTensor):
    """(sorted keys, entries in that order, splitters) of ``sp`` on the device: 16 bytes per nonzero plus the splitters,
    built once per tensor and row order and kept beside the mode permutations in ``sp._dev[2]`` (their keys are
    integers, this one is a tuple); a ``.T`` view shares the upload and has an index of its own."""
    from . import _native as nat
    idx, val = sp.dev_indices(), sp.dev_entries()
    order = tuple(sp.dev_row_order)
    cache = sp._dev[2]
    slot = ("key_index", order)
    if slot not in cache:
        N, d = sp.nnz, sp.ndim
        keys, vals = DevArray.empty((N,), dtype=np.int64), DevArray.empty((N,))
        spl = DevArray.empty((_layout(N)["n_split"],), dtype=np.int64)
        nat.call("ttsk_sparse_key_index", nat.i64_array(sp.shape), d, idx, N, (ctypes.c_int * d)(*order), N, val, 0,
                 keys, vals, spl, 0)
        cache[slot] = (keys, vals, spl)
    return cache[slot]


def _outputs(N: int, want_out: bool, want_dot: bool):
    return (DevArray.empty((N,)) if want_out else None), (DevArray.empty((1,)) if want_dot else None)


def _sparse_join(table: SparseTensor, idx, want_out: bool, want_dot: bool):
    """One pass of ``ttsk_sparse_join``: the entries of ``table`` at the index list ``idx`` (a ``SparseTensor`` of its
    shape, a ``(d, N)`` array or a tuple of ``d`` arrays) as (DevArray (N,) or None, ``sum_q entries_q(idx) * that`` or
    None).  Raises ``TtskUnsupported`` for a shape the entry refuses."""
    from . import _native as nat
    dev_idx, stride, order, N, val = _gather_indices(idx, table.shape)
    if want_dot and val is None:
        raise ValueError("gather: the dot needs the entries of a SparseTensor")
    d = table.ndim
    keys, vals, spl = _key_index(table)
    out, dot = _outputs(N, want_out, want_dot)
    nat.call("ttsk_sparse_join", keys, vals, spl, table.nnz, 0, nat.i64_array(table.shape), d, dev_idx, stride,
             (ctypes.c_int * d)(*order), N, val if want_dot else None, out, dot, 0)
    return out, (float(dot.get()[0]) if want_dot else None)


def _dense_join(dense: DenseTensor, idx, want_out: bool, want_dot: bool):
    """One pass of ``ttsk_dense_join``: the same against a dense tensor.  A ``.T`` view of a contiguous buffer is read in
    place (the keys are formed in the reversed shape with the rows in reverse order); any other layout is copied once."""
    from . import _native as nat
    if np.dtype(dense.data.dtype) != np.float64:
        raise TypeError(f"gather: float64 data expected, got {dense.data.dtype}")
    dev_idx, stride, order, N, val = _gather_indices(idx, dense.shape)
    if want_dot and val is None:
        raise ValueError("gather: the dot needs the entries of a SparseTensor")
    arr, shape = dense.dev_data(), tuple(dense.shape)
    if not arr.is_contiguous():
        if arr.T.is_contiguous():
            arr, shape, order = arr.T, shape[::-1], tuple(order)[::-1]
        else:
            arr = arr.contiguous()
    d = len(shape)
    out, dot = _outputs(N, want_out, want_dot)
    nat.call("ttsk_dense_join", arr, nat.i64_array(shape), d, dev_idx, stride, (ctypes.c_int * d)(*order), N,
             val if want_dot else None, out, dot, 0)
    return out, (float(dot.get()[0]) if want_dot else None)


def _join_dot(sp: SparseTensor, other, route=None):
    """``<sp, other>`` with ``sp`` as the queries (the reference's orientation: ``other.gather(sp.indices) . sp.entries``)
    in one device pass, or None where the caller keeps its host path: the rule or ``route`` says so (sparse tables
    only: the host path against a dense tensor densifies ``sp``), or the entry refuses the shape (under
    ``route="kernel"`` its ``TtskUnsupported`` propagates)."""
    from . import _native as nat
    if tuple(other.shape) != tuple(sp.shape):
        raise ValueError(f"dot: tensors of shape {sp.shape} and {tuple(other.shape)}")
    sparse = isinstance(other, SparseTensor)
    if resolve(route) == "composed" or (sparse and not _join_routed(other, sp.nnz, route)):
        return None
    if sp.nnz == 0 or (sparse and other.nnz == 0):
        return 0.0
    try:
        return (_sparse_join if sparse else _dense_join)(other, sp, False, True)[1]
    except nat.TtskUnsupported:
        if resolve(route) == "kernel":
            raise
        return None
