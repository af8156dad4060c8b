"""Omega / Psi for CP inputs (reference ``cp_sketch.py:6-36``)."""
from ..device import as_dev, contract


def sketch_omega_cp(left_sketch, right_sketch, **kwargs):
    """Omega = L^T R.  In the generic path Omega is asked for before Psi and, with another left contraction than Psi's
    (L_mu against L_{mu-1}), shares no operand pair with it: a launch of its own here, ``ttsk_cp_psi_omega`` without Psi.
    ``cp_fused.try_cp_sketch`` is where Omega rides in Psi's launch."""
    from .. import cp_fused
    out = cp_fused.psi_omega(as_dev(left_sketch), as_dev(right_sketch), None, psi=False, omega=True)
    if out is not None:
        return out[1]
    return contract("ji,jk->ik", as_dev(left_sketch), as_dev(right_sketch))


def sketch_psi_cp(left_sketch, right_sketch, *, tensor, mu: int, **kwargs):
    """Psi[i,k,m] = sum_j L[j,i] V_mu[k,j] R[j,m] (one rank-1 slab per CP term): one ``ttsk_cp_psi_omega`` that forms
    V_mu o R in registers, or, where its plan refuses the shape, the compositions below with their N x n x r panel W."""
    from .. import cp_fused
    V = tensor.dev_cores()[mu]
    out = cp_fused.psi_omega(None if left_sketch is None else as_dev(left_sketch),
                             None if right_sketch is None else as_dev(right_sketch), V)
    if out is not None:
        return out[0]
    if left_sketch is None:
        return contract("ji,il->jl", V, as_dev(right_sketch))[None]
    if right_sketch is None:
        return contract("li,kl->ik", as_dev(left_sketch), V)[:, :, None]
    W = contract("kj,jm->jkm", V, as_dev(right_sketch))
    return contract("ji,jkm->ikm", as_dev(left_sketch), W)
