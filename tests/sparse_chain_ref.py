"""Host reference of the chain factor of the sparse pass (kind 4 of ttsk_sg_factor, csrc/sparse_pass.h stage 2b'), shared
by tests/test_gpu_sparse_chain.py and tests/test_sparse_chain_plan.py: the digits of a flat index by divmod and the rows
    t(e) D_0[:, i_0(e), :] ... D_{s-1}[:, i_{s-1}(e), lo:lo+w]
as an int64 einsum.  Nothing here needs a device."""
import numpy as np


def digits(flat, rows, ns, j=None):
    """(row of the start table, [index into each core]) of every flat index: ``rows`` first (0: no table, row 0), then the
    mode sizes ``ns`` in order -- the first the fastest digit; with ``j`` given it is the last digit and no part of ``flat``"""
    rest = np.asarray(flat, dtype=np.int64).copy()
    row = np.zeros_like(rest)
    if rows:
        row, rest = rest % rows, rest // rows
    out = []
    for s, n in enumerate(ns):
        if j is not None and s == len(ns) - 1:
            out.append(np.asarray(j, dtype=np.int64))
            break
        out.append(rest % n)
        rest = rest // n
    return row, out


def chain_rows(flat, table, rows, cores, lo, w, j=None):
    """the (N, w) rows of a chain factor in int64: ``table`` (rows, rank_0) or None (the vector (1)), ``cores`` a list of
    (rank_s, n_s, rank_{s+1}) integer arrays"""
    row, idx = digits(flat, rows if table is not None else 0, [c.shape[1] for c in cores], j)
    v = np.asarray(table, dtype=np.int64)[row] if table is not None else np.ones((len(row), 1), dtype=np.int64)
    for D, i in zip(cores, idx):
        v = np.einsum("ea,aeb->eb", v, np.asarray(D, dtype=np.int64)[:, i, :])
    return v[:, lo:lo + w]
