"""Omega / Psi for operator-times-train products that are never formed (``OperatorProduct``)."""
from ..device import as_dev, contract


def sketch_omega_operator_product(left_sketch, right_sketch, **kwargs):
    """Omega_mu = L_mu^T R_mu, both over the product's rank index (beta a)."""
    return contract("ji,jk->ik", as_dev(left_sketch), as_dev(right_sketch))


def sketch_psi_operator_product(left_sketch, right_sketch, *, tensor, mu: int, **kwargs):
    """Psi_mu = W_mu R_mu with W_mu = L_{mu-1} o (M_mu, C_mu) from ``op_apply`` (one ``ttsk_op_apply`` call, or composed
    from ``contract`` calls where its routing rule has it): (l, n_out, R' r'), never
    the (R r, n_out, R' r') product core.  Either side may be None at the ends."""
    from ..operator_product import chain_start, op_apply
    Ms, Cs = tensor.dev_parts()
    M, C = Ms[mu], Cs[mu]
    if left_sketch is None:
        L = chain_start()
    else:
        L = as_dev(left_sketch).contiguous()
        L = L.reshape(M.shape[0], C.shape[0], L.shape[1])
    W, _ = op_apply([L], [M], [C])
    if right_sketch is None:
        return W
    return contract("lic,cm->lim", W, as_dev(right_sketch))
