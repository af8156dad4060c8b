"""Host reference of the Khatri-Rao DRM (tt_sketch_amd/drm/khatri_rao_drm.py), by its definition: the explicit sketching
matrices

    S_mu[m, i_0 .. i_mu] = prod_{s <= mu} mats[s][m, i_s],   rank_min[mu] <= m < rank_max[mu],

in the order the DRM walks the tensor, and the streaming sketch of a dense array with them.  NumPy only; shared by
tests/test_khatri_rao_host.py and tests/test_gpu_khatri_rao.py."""
import numpy as np


def level_matrices(mats, rank_min, rank_max):
    """[S_mu as an array (w_mu, n_0, ..., n_mu)], the modes in walk order"""
    out, K = [], None
    for mu, M in enumerate(mats):
        M = np.asarray(M, dtype=np.float64)
        K = M if K is None else K[..., None] * M.reshape((M.shape[0],) + (1,) * (K.ndim - 1) + (M.shape[1],))
        out.append(K[rank_min[mu]:rank_max[mu]])
    return out


def of_drm(drm):
    """``level_matrices`` of a KhatriRaoDRM (its rank bookkeeping is kept in walk order, as its matrices are)"""
    return level_matrices([np.asarray(m) for m in drm.mats], drm.rank_min, drm.rank_max)


def sketch(X, left, right):
    """(Psi, Omega) of the streaming sketch of the dense array X: ``left`` = level_matrices of the left DRM, ``right`` those of
    the right DRM (which walks the modes from the last one: level nu covers modes d - 1 .. d - 1 - nu)."""
    X = np.asarray(X, dtype=np.float64)
    d, shape = X.ndim, X.shape
    # A[mu]: (l_mu, prod n_{<=mu}); B[mu]: (r_mu, prod n_{>mu}), both with the modes in the tensor's C order
    A = [S.reshape(S.shape[0], -1) for S in left]
    B = [None] * (d - 1)
    for nu, S in enumerate(right):
        St = np.transpose(S, (0,) + tuple(range(S.ndim - 1, 0, -1)))
        B[d - 2 - nu] = St.reshape(S.shape[0], -1)
    Psi, Omega = [], []
    for mu in range(d):
        nl, nr = int(np.prod(shape[:mu], dtype=np.int64)), int(np.prod(shape[mu + 1:], dtype=np.int64))
        Xm = X.reshape(nl, shape[mu], nr)
        Lm = A[mu - 1] if mu else np.ones((1, 1))
        Rm = B[mu] if mu < d - 1 else np.ones((1, 1))
        Psi.append(np.einsum("ap,pjq,cq->ajc", Lm, Xm, Rm, optimize=True))
    for mu in range(d - 1):
        n = int(np.prod(shape[:mu + 1], dtype=np.int64))
        Omega.append(A[mu] @ X.reshape(n, -1) @ B[mu].T)
    return Psi, Omega
