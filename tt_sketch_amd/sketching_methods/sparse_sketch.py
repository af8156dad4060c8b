"""Omega / Psi for sparse (COO) inputs (reference ``sparse_sketch.py:8-69``).

Omega is a skinny GEMM over the nonzeros with the entries folded in as a scale along the
contracted index; Psi is a scatter of rank-one updates into the slices selected by the mode
index, done by a run-reducing kernel (one atomic per slice change instead of the reference's
O(n_mu * nnz) boolean masks)."""
from .. import _native as nat
from ..device import DevArray, as_dev, contract


def _psi_call(tensor, Lv, l, Rv, r, n, idx_row, perm, out):
    nat.call("ttsk_sparse_psi", tensor.dev_entries(), idx_row, perm, tensor.nnz, Lv, l, Rv, r, n, out, 0)


def sketch_omega_sparse(left_sketch, right_sketch, *, tensor, **kwargs):
    """Omega = (L * entries) R^T with L (l, nnz), R (r, nnz): the Psi kernel with a single slice."""
    Lv, Rv = as_dev(left_sketch).T.contiguous(), as_dev(right_sketch).T.contiguous()
    l, r = Lv.shape[1], Rv.shape[1]
    out = DevArray.zeros((l, 1, r))
    _psi_call(tensor, Lv, l, Rv, r, 1, None, None, out)
    return out.reshape(l, r)


def sketch_psi_sparse(left_sketch, right_sketch, *, tensor, mu: int, psi_shape, **kwargs):
    """Psi[:, j, :] = sum_{e: idx_mu[e]=j} entries[e] L[:,e] R[:,e]^T, nonzeros visited in mode-index
    order (permutation cached on the tensor) so that each slice is one register-resident run."""
    l, n, r = (int(x) for x in psi_shape)
    out = DevArray.zeros((l, n, r))
    if left_sketch is None and right_sketch is None:
        raise ValueError("sketch_psi_sparse needs at least one side")
    Lv = None if left_sketch is None else as_dev(left_sketch).T.contiguous()
    Rv = None if right_sketch is None else as_dev(right_sketch).T.contiguous()
    idx_row = tensor.dev_indices()[tensor.dev_row_order[mu]]
    _psi_call(tensor, Lv, l, Rv, r, n, idx_row, tensor.dev_mode_perm(mu), out)
    return out
