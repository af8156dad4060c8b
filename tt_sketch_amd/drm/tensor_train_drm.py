"""Tensor-train DRM: sketches with partial contractions of a fixed random TT.

API of the reference's ``tt_sketch/drm/tensor_train_drm.py:23-145`` (constructor incl. the
``cores=`` injection kwarg, ``sketch_tt / sketch_cp / sketch_sparse / sketch_dense /
sketch_tucker``).  Cores are sampled on the device (hash -> ndtri generator keyed by
``seed`` and the core number; N(0,1)/sqrt(r_{mu-1}) as tensor.py:370-371 "norm-preserve",
last core never materialised) and every chain step is an MFMA contraction in HBM.
"""
from __future__ import annotations

import ctypes
import sys
from typing import List, Optional, Tuple, Union

import numpy as np

from .. import _native as nat
from ..device import DevArray, as_dev, contract
from ..drm_base import CanSlice, handle_transpose
from ..sketching_methods.abstract_methods import (CansketchCP, CansketchDense, CansketchHadamardProduct,
                                                  CansketchOperatorProduct, CansketchSparse, CansketchTT, CanSketchTucker)
from ..utils import random_normal_dev_many


class _PackedCores:
    """The chain images of a DRM's interior cores (``ttsk_drm_pack``) and the device cores they were made from.  Holding
    the cores keeps their buffers out of the pool until the images are dropped: a registration never outlives its core.
    Shared by a DRM and its copies (``.T``, ``copy.copy``); the images go when the last of them does, or on ``release``."""

    def __init__(self):
        self.cores: List[DevArray] = []

    def add(self, core: DevArray) -> None:
        if any(c is core for c in self.cores):
            return
        A, n, A2 = (int(x) for x in core.shape)
        try:
            nat.call("ttsk_drm_pack", ctypes.c_void_p(core.ptr), A, n, A2, 0)
        except nat.TtskUnsupported:
            return                       # ranks outside the fused chain step: nothing would read an image
        self.cores.append(core)

    def release(self) -> None:
        cores, self.cores = self.cores, []
        for c in cores:                  # before the buffers go back to the pool (``cores`` still holds them here)
            nat.call("ttsk_drm_unpack", ctypes.c_void_p(c.ptr))

    def __del__(self):
        if sys.is_finalizing():          # the process ends: its device memory goes with it
            return
        try:
            self.release()
        except Exception:
            pass


class TensorTrainDRM(CansketchSparse, CansketchTT, CansketchCP, CanSlice, CansketchDense,
                     CanSketchTucker, CansketchOperatorProduct, CansketchHadamardProduct):
    cores: list

    def __init__(self, rank: Union[Tuple[int, ...], int], shape: Tuple[int, ...], transpose: bool,
                 seed: Optional[int] = None, **kwargs) -> None:
        super().__init__(rank, shape, transpose, seed=seed, **kwargs)
        if "cores" in kwargs:
            self.cores = kwargs["cores"]
        else:
            walk = self.shape[::-1] if transpose else self.shape
            rk = (1,) + tuple(self.true_rank)
            k = len(walk) - 1
            self.cores = random_normal_dev_many([(rk[mu], walk[mu], rk[mu + 1]) for mu in range(k)],
                                                [(self.seed << 20) + mu for mu in range(k)],
                                                [1.0 / np.sqrt(rk[mu]) for mu in range(k)])
        self._dev: List[DevArray] = []
        self._dev_src: list = []          # the host objects the device copies were made from
        self._packed = _PackedCores()

    def pack_for_chain(self) -> None:
        """Stores the interior cores a second time in the layout the fused chain step loads them in (``ttsk_drm_pack``):
        its loader then copies each slice instead of gathering it.  Worth it where the DRM sketches many tensors -- the
        batched and summed one-call paths call this on first use; one sketch of a fresh DRM gains less than the pass over
        the cores costs and does not pack.  Idempotent.  A packed core takes about twice its device memory; ``close``
        (or the DRM's end) gives the images back, before the cores' buffers.

        Invariant: device cores are never written after they are made (every method here only reads them).  Code that
        does write one must call ``ttsk_drm_unpack`` on it first."""
        for k, c in enumerate(self.dev_cores()):
            if k >= 1 and c.ndim == 3 and c.is_contiguous():
                self._packed.add(c)

    def close(self) -> None:
        """Drops the packed chain images (the DRM stays usable; it packs again on the next batched use)."""
        self._packed.release()

    def dev_cores(self) -> List[DevArray]:
        """Device copies of ``self.cores`` (the list may grow: OrthogTTDRM appends)."""
        for k, c in enumerate(self.cores):
            if k < len(self._dev) and self._dev_src[k] is c:
                continue
            d = as_dev(c)
            if k < len(self._dev):
                self._dev[k], self._dev_src[k] = d, c
            else:
                self._dev.append(d)
                self._dev_src.append(c)
        return self._dev

    def _core(self, mu) -> DevArray:
        return self.dev_cores()[mu]

    def _cut(self, mu, mat: DevArray) -> DevArray:
        return mat[:, self.rank_min[mu]:self.rank_max[mu]]

    # ------------------------------------------------------------------ TT input
    @handle_transpose
    def sketch_tt(self, tensor):
        """L_mu[l,m] = sum L_{mu-1}[i,j] X_mu[i,k,l] D_mu[j,k,m] (reference :71-88)."""
        Xs = tensor.dev_cores()
        L = None
        for mu in range(len(self.shape) - 1):
            X, D = Xs[mu], self._core(mu)
            if mu == 0:
                L = contract("ijk,ijl->kl", X, D)
            elif X.strides[2] > X.strides[0]:       # view of a transposed core
                T = contract("ij,ikl->jlk", L, X)
                L = contract("jlk,jkm->lm", T, D)
            else:
                T = contract("ij,ikl->jkl", L, X)
                L = contract("jkl,jkm->lm", T, D)
            yield self._cut(mu, L)

    # ------------------------------------------------------------------ operator-times-train input
    @handle_transpose
    def sketch_operator_product(self, tensor):
        """L_mu[(b' a'), m] = sum_{l,i} W_mu[l, i, (b' a')] D_mu[l, i, m] with W_mu = L_{mu-1} o (M_mu, C_mu) from
        ``op_apply`` -- one ``ttsk_op_apply`` call, or W composed from two ``contract`` calls where its routing rule has it,
        which for one term it does at every measured shape: the product core of ``MPO.__call__`` (reference
        tt_gmres.py:90-101) is never formed either way."""
        from ..operator_product import chain_start, op_apply
        Ms, Cs = tensor.dev_parts()
        L = chain_start()
        for mu in range(len(self.shape) - 1):
            M, C = Ms[mu], Cs[mu]
            W, _ = op_apply([L], [M], [C])
            Lm = contract("lic,lim->cm", W, self._core(mu))
            yield self._cut(mu, Lm)
            L = Lm.reshape(M.shape[3], C.shape[2], Lm.shape[1])

    # ------------------------------------------------------------------ entrywise product of two trains
    @handle_transpose
    def sketch_hadamard_product(self, tensor):
        """L_mu[(b' a'), m] = sum_{l,i} W_mu[l, i, (b' a')] D_mu[l, i, m] with W_mu = L_{mu-1} o (X_mu, Y_mu) from
        ``hadamard_apply`` -- one ``ttsk_hadamard_apply`` call, or W composed from ``contract`` calls where its routing rule
        has it: the Kronecker core of the product is never formed either way."""
        from ..hadamard_product import hadamard_apply
        from ..operator_product import chain_start
        Xs, Ys = tensor.dev_parts()
        L = chain_start()
        for mu in range(len(self.shape) - 1):
            X, Y = Xs[mu], Ys[mu]
            W = hadamard_apply(L, X, Y)
            Lm = contract("lic,lim->cm", W, self._core(mu))
            yield self._cut(mu, Lm)
            L = Lm.reshape(X.shape[2], Y.shape[2], Lm.shape[1])

    # ------------------------------------------------------------------ CP input
    @handle_transpose
    def sketch_cp(self, tensor):
        """L_mu[i,l] = sum_{j,k} L_{mu-1}[i,j] V_mu[k,i] D_mu[j,k,l] (reference :90-107): one ``ttsk_cp_chain_step`` per mode
        that forms L_{mu-1} o V_mu in registers, or, where its plan refuses the shape, the two ``contract`` calls below with
        their N x n x rank panel W."""
        from ..cp_fused import chain_step
        Vs = tensor.dev_cores()
        L = None
        for mu in range(len(self.shape) - 1):
            V, D = Vs[mu], self._core(mu)
            Lk = chain_step(L, V, D)
            if Lk is not None:
                L = Lk
            elif mu == 0:
                L = contract("ij,ik->jk", V, D[0])
            else:
                W = contract("ij,jkl->ikl", L, D)
                L = contract("ki,ikl->il", V, W)
            yield self._cut(mu, L)

    # ------------------------------------------------------------------ sparse input
    @handle_transpose
    def sketch_sparse(self, tensor):
        """v_e <- v_e D_mu[:, idx_mu[e], :] per nonzero (reference :60-69); yields (rank, nnz)."""
        idx = tensor.dev_indices()
        order = tensor.dev_row_order
        N = tensor.nnz
        v = None
        for mu, _ in enumerate(self.cores):     # the list may grow while we walk it (OrthogTTDRM)
            D = self._core(mu).contiguous()
            rho, n, rhop = D.shape
            out = DevArray.empty((N, rhop))
            nat.call("ttsk_sparse_ttdrm_step", v, rho, D, n, rhop, idx[order[mu]], N, out, 0)
            v = out
            yield self._cut(mu, v).T

    # ------------------------------------------------------------------ dense input
    @handle_transpose
    def sketch_dense(self, tensor):
        """The DRM as dense matrices (rho_mu, prod n_{<=mu}) (reference :109-122).

        Handed out as ``ChainedUnfolding`` recipes (P_k = P_{k-1} x D_k): the dense Omega / Psi routines
        contract the tensor one mode at a time and never form the (rho x n^k) matrices; anything else that
        touches one gets the matrix (``as_dev`` / ``np.asarray`` / ``.get()`` materialise it)."""
        from ..sketching_methods.dense_sketch import ChainedUnfolding
        P = None
        for mu in range(len(self.shape) - 1):
            P = ChainedUnfolding(P, self._core(mu))
            yield P

    # ------------------------------------------------------------------ Tucker input
    @handle_transpose
    def sketch_tucker(self, tensor):
        """DRM against the Tucker factors (reference :124-145); yields (prod s_{<=mu}, rho_mu)."""
        Us, _ = tensor.dev_parts()
        P = contract("jk,lj->lk", self._core(0)[0], Us[0])
        yield P
        for mu in range(1, len(self.shape) - 1):
            red = contract("jkl,mk->jml", self._core(mu), Us[mu])
            P = contract("ij,jml->iml", P, red)
            P = P.reshape(-1, P.shape[-1])
            yield P
