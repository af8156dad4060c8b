"""Omega / Psi for entrywise products of two tensor trains that are never formed (``HadamardProduct``)."""
from ..device import as_dev, contract


def sketch_omega_hadamard_product(left_sketch, right_sketch, **kwargs):
    """Omega_mu = L_mu^T R_mu, both over the product's rank index (beta a)."""
    return contract("ji,jk->ik", as_dev(left_sketch), as_dev(right_sketch))


def sketch_psi_hadamard_product(left_sketch, right_sketch, *, tensor, mu: int, **kwargs):
    """Psi_mu = W_mu R_mu with W_mu = L_{mu-1} o (X_mu, Y_mu) from ``hadamard_apply`` (one ``ttsk_hadamard_apply`` call, or
    composed from ``contract`` calls where its routing rule has it): (l, n, R' r'), never the (R r, n, R' r') Kronecker
    core.  Either side may be None at the ends."""
    from ..hadamard_product import hadamard_apply
    from ..operator_product import chain_start
    Xs, Ys = tensor.dev_parts()
    X, Y = Xs[mu], Ys[mu]
    if left_sketch is None:
        L = chain_start()
    else:
        L = as_dev(left_sketch).contiguous()
        L = L.reshape(X.shape[0], Y.shape[0], L.shape[1])
    W = hadamard_apply(L, X, Y)
    if right_sketch is None:
        return W
    return contract("lic,cm->lim", W, as_dev(right_sketch))
