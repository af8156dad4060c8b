"""Khatri-Rao DRM: column ``m`` of level ``mu`` is the Kronecker product of the ``m``-th columns of one small Gaussian
matrix per mode,

    S_mu[m, (i_0 .. i_mu)] = prod_{s <= mu} mats[s][m, i_s],        rank_min[mu] <= m < rank_max[mu],

the standard structured test matrix of the tensor-sketching literature.  It stores ``d - 1`` matrices ``mats[s]`` of
``(R, n_s)``, ``R = max(true_rank)``, in the order the DRM walks the tensor (``shape``, or ``shape[::-1]`` when
transposed).  Its columns are independent of each other, so a rank slice is a row range of the matrices and a rank increase
appends rows: unlike ``TensorTrainDRM`` it is ``CanIncreaseRank``, and unlike ``DenseGaussianDRM`` it sketches every tensor
kind and never stores anything of size ``prod n``.

The matrices are sampled on the device, row-major and keyed by (seed, mode, element), so the leading rows are unchanged when
``R`` grows (the property ``DenseGaussianDRM`` relies on); ``mats=`` injects them (the counterpart of ``cores=`` of the
train), and then construction touches no device.

Every step is an elementwise product of rows (``ttsk_kr_step``, ``csrc/khatri_rao.hip``).  The one-pass sparse path takes
the DRM as tables (``ttsk_kr_rows``) and diagonal chain factors (kind 5 of ``ttsk_sg_factor``): ``sparse_fused._Side``.
Dense inputs go through ``as_train``, the ``TensorTrainDRM`` with diagonal cores: correct, not fast -- a dense step through
a diagonal core spends ``R`` times the multiply-adds the product needs.  A Tucker tensor's factor matrices are contracted
with the small matrices directly and the rows multiplied by ``ttsk_kr_rows``.
"""
from __future__ import annotations

from typing import List, Optional, Tuple, Union

import numpy as np

from .. import _native as nat
from ..device import DevArray, as_dev, contract, to_host
from ..drm_base import CanIncreaseRank, handle_transpose
from ..sketching_methods.abstract_methods import (CansketchCP, CansketchDense, CansketchSparse, CansketchTT,
                                                  CanSketchTucker)
from ..utils import random_normal_dev
from .tensor_train_drm import TensorTrainDRM

SEED_TAG = 0x4B520000            # "KR": the sample streams of the modes, apart from those of the other DRMs of a seed


class KhatriRaoDRM(CansketchTT, CansketchCP, CansketchSparse, CansketchDense, CanSketchTucker, CanIncreaseRank):
    mats: list

    def __init__(self, rank: Union[Tuple[int, ...], int], shape: Tuple[int, ...], transpose: bool,
                 seed: Optional[int] = None, **kwargs) -> None:
        super().__init__(rank, shape, transpose, seed=seed, **kwargs)
        walk = self.shape[::-1] if self.transpose else self.shape
        R = max(self.true_rank) if self.true_rank else 0
        self._injected = "mats" in kwargs
        if self._injected:
            self.mats = list(kwargs["mats"])
            if len(self.mats) != len(walk) - 1:
                raise ValueError(f"KhatriRaoDRM: {len(self.mats)} matrices for {len(walk)} modes")
            for s, m in enumerate(self.mats):
                if len(m.shape) != 2 or m.shape[0] < R or m.shape[1] != walk[s]:
                    raise ValueError(f"KhatriRaoDRM: matrix {s} has shape {tuple(m.shape)}, ({R}, {walk[s]}) is needed")
        else:
            self.mats = [random_normal_dev((R, n), seed=(self.seed << 20) + SEED_TAG + s) for s, n in enumerate(walk[:-1])]
        # what is made from the matrices once: device copies, column cuts, the embedding (shared with slices and ``.T``)
        self._cache: dict = {}

    # ------------------------------------------------------------------ rank bookkeeping
    def slice(self, start_rank, end_rank) -> "KhatriRaoDRM":
        """the same matrices, other rows of them: nothing is sampled"""
        full = self.true_rank[::-1] if self.transpose else self.true_rank
        out = type(self)(rank=self.rank, shape=self.shape, transpose=self.transpose, seed=self.seed, rank_min=start_rank,
                         rank_max=end_rank, true_rank=full, mats=self.mats)
        out.mats, out._injected, out._cache = self.mats, self._injected, self._cache
        return out

    def increase_rank(self, new_rank, mats=None) -> "KhatriRaoDRM":
        """the DRM of ``new_rank`` whose leading columns are this one's: sampled matrices grow by rows of the same streams;
        injected ones cannot be resampled, the caller hands in the larger ``mats`` (leading rows unchanged)"""
        if mats is None and self._injected:
            raise ValueError("KhatriRaoDRM.increase_rank: the matrices were injected, pass the larger ones as mats=")
        extra = {} if mats is None else {"mats": mats}
        return type(self)(new_rank, self.shape, self.transpose, self.seed, **extra)

    def _window(self) -> Tuple[int, int]:
        """[c0, c1): the rows of the matrices any level hands out"""
        return min(self.rank_min), max(self.rank_max)

    def _mat(self, s: int) -> DevArray:
        key = ("mat", s)
        if key not in self._cache:
            self._cache[key] = as_dev(self.mats[s])
        return self._cache[key]

    def dev_cols(self, s: int, lo: int, hi: int) -> DevArray:
        """``mats[s][lo:hi]^T`` as a contiguous ``(n_s, hi - lo)`` device array: the table a step gathers its rows from"""
        key = ("cols", s, lo, hi)
        if key not in self._cache:
            self._cache[key] = self._mat(s)[lo:hi].T.contiguous()
        return self._cache[key]

    def _cut(self, mu: int, panel: DevArray) -> DevArray:
        c0, _ = self._window()
        return panel[:, self.rank_min[mu] - c0:self.rank_max[mu] - c0]

    # ------------------------------------------------------------------ the embedding
    def as_train(self) -> TensorTrainDRM:
        """The ``TensorTrainDRM`` with diagonal cores ``core_s[j, k, m] = delta_jm G_s[k, m]`` (``G_s = mats[s]^T``) that
        hands out exactly this DRM's columns.  Built on the host; a step through it costs ``R`` times the multiply-adds of
        the elementwise product it stands for."""
        key = ("train", self.transpose, tuple(self.rank_min), tuple(self.rank_max))
        if key not in self._cache:
            c0, c1 = self._window()
            R = c1 - c0
            cores = []
            for s, m in enumerate(self.mats):
                G = np.ascontiguousarray(to_host(m)[c0:c1].T)                    # (n_s, R)
                if s == 0:
                    cores.append(G[None, :, :].copy())
                else:
                    D = np.zeros((R, G.shape[0], R))
                    D[np.arange(R), :, np.arange(R)] = G.T
                    cores.append(D)
            train = TensorTrainDRM(R, self.shape, self.transpose, seed=self.seed, cores=cores)
            train.true_rank = (R,) * len(self.mats)
            train.rank_min = tuple(lo - c0 for lo in self.rank_min)
            train.rank_max = tuple(hi - c0 for hi in self.rank_max)
            train.rank = tuple(self.rank)
            self._cache[key] = train
        return self._cache[key]

    # ------------------------------------------------------------------ sparse input
    @handle_transpose
    def sketch_sparse(self, tensor):
        """v_e <- v_e * G_mu[idx_mu[e], :] per nonzero; yields (rank, nnz)."""
        idx = tensor.dev_indices()
        order = tensor.dev_row_order
        N = tensor.nnz
        c0, c1 = self._window()
        v = None
        for mu in range(len(self.mats)):
            G = self.dev_cols(mu, c0, c1)
            out = DevArray.empty((N, c1 - c0))
            nat.call("ttsk_kr_step", v, G, G.shape[0], c1 - c0, idx[order[mu]], N, out, 0)
            v = out
            yield self._cut(mu, v).T

    # ------------------------------------------------------------------ CP input
    @handle_transpose
    def sketch_cp(self, tensor):
        """L_mu = L_{mu-1} * (V_mu^T G_mu), elementwise: one ``contract`` and one ``ttsk_kr_step`` without an index per mode;
        yields (CP rank, rank)."""
        Vs = tensor.dev_cores()
        c0, c1 = self._window()
        L = None
        for mu in range(len(self.mats)):
            W = contract("ki,km->im", Vs[mu], self.dev_cols(mu, c0, c1))
            if L is not None:
                N, w = W.shape
                out = DevArray.empty((N, w))             # (not in place: the cut of L handed out before is still read)
                nat.call("ttsk_kr_step", L, W, N, w, None, N, out, 0)
                W = out
            L = W
            yield self._cut(mu, L)

    # ------------------------------------------------------------------ TT input
    @handle_transpose
    def sketch_tt(self, tensor):
        """L_mu[b, m] = sum_{a, k} L_{mu-1}[a, m] G_mu[k, m] X_mu[a, k, b]: column m is the chain of a rank-one CP term, so
        a step is ``cp_fused.chain_step`` with the train's core in the place of the DRM core (as ``tensor_gram._tt_cp_dot``),
        or, where its routing rule or its plan declines, two ``contract`` calls.  Kept as (rank, train rank); yields the
        transposed view."""
        from ..cp_fused import chain_step
        Xs = tensor.dev_cores()
        c0, c1 = self._window()
        Lt = None
        for mu in range(len(self.mats)):
            X, G = Xs[mu], self.dev_cols(mu, c0, c1)
            Lk = chain_step(Lt, G, X)
            if Lk is not None:
                Lt = Lk
            elif mu == 0:
                Lt = contract("km,kb->mb", G, X[0])
            else:
                W = contract("ma,akb->mkb", Lt, X)
                Lt = contract("km,mkb->mb", G, W)
            yield self._cut(mu, Lt.T)

    # ------------------------------------------------------------------ dense and Tucker input: through the embedding
    def _dense_core(self, s: int, first: bool, lo: int, hi: int) -> DevArray:
        """a core of the embedding for the dense recipes: mode s as the first core of a chain, (1, n_s, R), or as a later,
        diagonal one, (R, n_s, R); the columns [lo, hi) of the window"""
        key = ("dense core", s, first, self._window(), lo, hi)
        if key not in self._cache:
            c0, c1 = self._window()
            G = to_host(self.mats[s])[c0:c1].T                                   # (n_s, R)
            if first:
                D = G[None, :, lo:hi]
            else:
                D = np.zeros((c1 - c0, G.shape[0], c1 - c0))
                D[np.arange(c1 - c0), :, np.arange(c1 - c0)] = G.T
                D = D[:, :, lo:hi]
            self._cache[key] = as_dev(np.ascontiguousarray(D))
        return self._cache[key]

    @handle_transpose
    def sketch_dense(self, tensor):
        """The recipes of ``TensorTrainDRM.sketch_dense`` (``ChainedUnfolding``: the (rank x prod n) matrices are never
        formed) on the cores of the embedding; the last core of a level is cut to the columns the level hands out.

        A left DRM's chains are those of ``as_train``.  A right DRM's are not: the dense products pair a right matrix's
        columns with the tensor's trailing modes position by position, the last core's mode with the LAST mode
        (``dense_sketch._right_product``), so a train that walks the modes from the last one sketches with another matrix
        than S_mu.  The steps of this DRM commute, so each level is chained in the tensor's own mode order instead -- the
        level of the modes mu + 1 .. d - 1 starts at mode mu + 1 and ends at d - 1 -- and the product is S_mu itself."""
        from ..sketching_methods.dense_sketch import ChainedUnfolding
        c0, c1 = self._window()
        R = c1 - c0
        made: dict = {}
        for mu in range(len(self.mats)):
            lo, hi = self.rank_min[mu] - c0, self.rank_max[mu] - c0
            chain =list(range(mu, -1, -1)) if self.transpose else list(range(mu + 1))
            P = None
            for pos, s in enumerate(chain):
                last = pos == len(chain) - 1
                cut = (lo, hi) if last else (0, R)
                key = (tuple(chain[:pos + 1]), cut)      # (a left DRM's uncut prefixes are shared between its levels)
                if key not in made:
                    made[key] = ChainedUnfolding(P, self._dense_core(s, pos == 0, *cut))
                P = made[key]
            yield P

    @handle_transpose
    def sketch_tucker(self, tensor):
        """P_mu[(s_0 .. s_mu), m] = P_{mu-1}[(s_0 .. s_{mu-1}), m] (U_mu G_mu)[s_mu, m]: one ``contract`` and one
        ``ttsk_kr_rows`` per mode.  The rows are ordered as the Tucker core's unfolding is read where they are consumed
        (``tucker_sketch``: C order of the tensor's own modes): a left DRM appends its mode as the fastest digit, a right one,
        which walks the modes from the last, as the slowest.  (The embedding is not used here: ``TensorTrainDRM.sketch_tucker``
        orders a right DRM's rows by its walk, which sketches with another -- equally valid -- matrix than the S_mu above.)"""
        Us, _ = tensor.dev_parts()
        c0, c1 = self._window()
        w = c1 - c0
        P = None
        for mu in range(len(self.mats)):
            W = contract("sk,km->sm", Us[mu], self.dev_cols(mu, c0, c1))
            if P is not None:
                rows, s = P.shape[0], W.shape[0]
                out = DevArray.empty((rows * s, w))
                if self.transpose:
                    nat.call("ttsk_kr_rows", P.contiguous(), rows, W, s, w, out, 0)
                else:
                    nat.call("ttsk_kr_rows", W, s, P.contiguous(), rows, w, out, 0)
                W = out
            P = W
            yield self._cut(mu, P)
