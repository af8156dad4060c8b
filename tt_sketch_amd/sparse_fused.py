"""Fast path: SparseTensor input with hashed sparse DRMs (SparseGaussianDRM / SparseSignDRM) or TensorTrainDRM, any pair, on
both sides, streaming method.

One pass per mode over a resident, mode-ordered stream of the nonzeros (``csrc/sparse_fused.hip``): the DRM rows are
sampled (or gathered from a small per-prefix table) where they are consumed, Psi_mu and one Omega come out of the
same pass, nothing of size nnz x rank is ever written.  Numerically the same sums as
``SparseGaussianDRM.sketch_sparse`` / ``SparseSignDRM.sketch_sparse`` + ``sketch_omega_sparse`` / ``sketch_psi_sparse``
(reference sparse_gaussian_drm.py:29-44, sparse_sign_drm.py:34-51, sparse_sketch.py:8-69) with bit-identical samples; the summation order is fixed
(no atomics), so two runs agree bit for bit.

A TensorTrainDRM's row is a row of a table of its partial products (``_Side._tt_table``, up to the deepest level the table
rule allows) taken a few chain steps further inside the pass (kind 4 of ``ttsk_sg_factor``): the sums of
``TensorTrainDRM.sketch_sparse`` without its panels.  Pairs with a train are routed (``paths.resolve``; the rule is
``chain_route_ms``): "composed" declines, and the generic driver runs the panels.

A KhatriRaoDRM's row is the elementwise product of one row per mode of its small matrices: a row of a table of those
products (``_Side._kr_table``, built level by level with ``ttsk_kr_rows``) taken a few diagonal chain steps further inside
the pass (kind 5 of ``ttsk_sg_factor``) -- no hash, no ``ndtri``, no rank x rank step.  Pairs of Khatri-Rao and hashed DRMs
always take the passes; beside a train the route's rule decides, a Khatri-Rao step counted as its w multiply-adds.
"""
from __future__ import annotations

import ctypes
import os
from typing import List, Optional, Tuple

import numpy as np

from . import _native as nat
from . import paths
from .device import DevArray, axpby, contract, copy_into
from .drm.khatri_rao_drm import KhatriRaoDRM
from .drm.sparse_gaussian_drm import SparseGaussianDRM
from .drm.sparse_sign_drm import SparseSignDRM
from .drm.tensor_train_drm import TensorTrainDRM
from .paths import SketchMethod, drm_pair
from .tensor import SparseTensor, TensorSum

last_plan: dict = {}             # what the last sketch did (bench.py reads it): sampled columns per nonzero, table rows
MAX_WIDTH = 32                   # columns per DRM factor the pass kernel takes (one 16-column matrix tile, or two)
MAX_MODE = 1 << 24               # the mode-order sort key holds the mode index in 24 bits (ttsk_sparse_mode_order)
TABLE_BYTES = 32 << 20           # a per-prefix table larger than this is sampled per nonzero instead (it would leave the L2 / MALL)


CHAIN_MAX = 8                    # steps of a chain factor (TTSK_SG_CHAIN_MAX of include/ttsk.h)


class _Chain(ctypes.Structure):
    """ttsk_sg_chain: the cores a kind-4 factor walks from its start table (or, with ``rows`` = 0, from the first core); for
    kind 5 the (n, w) tables of its diagonal steps, every rank w"""
    _fields_ = [("steps", ctypes.c_int), ("rows", ctypes.c_uint64), ("core", ctypes.c_void_p * CHAIN_MAX),
                ("n", ctypes.c_int64 * CHAIN_MAX), ("rank", ctypes.c_int * (CHAIN_MAX + 1))]


class _Factor(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("w", ctypes.c_int), ("rank_min", ctypes.c_int), ("src", ctypes.c_int),
                ("mul", ctypes.c_uint64), ("seed", ctypes.c_uint64), ("table", ctypes.c_void_p),
                ("full", ctypes.c_int), ("nnz", ctypes.c_int), ("chain", ctypes.POINTER(_Chain))]


def _u64(vals):
    return (ctypes.c_uint64 * len(vals))(*[int(v) for v in vals])


def _flat_mult(shape) -> List[int]:
    out = (ctypes.c_uint64 * len(shape))()
    nat.call("ttsk_sparse_flat_mult", _u64(shape), len(shape), out)
    return [int(v) for v in out]


class _Side:
    """One DRM as the passes see it: factor k = the DRM's k-th sketching matrix (k + 1 index rows)."""

    def __init__(self, drm, shape: Tuple[int, ...], nnz: int):
        self.drm = drm
        self.sign = type(drm) is SparseSignDRM
        self.tt = type(drm) is TensorTrainDRM
        self.kr = type(drm) is KhatriRaoDRM
        self.chained = self.tt or self.kr                  # its deep levels are chain factors: 32-bit streams, routed beside a train
        self.shape = tuple(int(n) for n in shape)          # in the order the DRM walks the tensor
        self.nnz = nnz
        self.cache = drm.__dict__.setdefault("_sg_tables", {})

    def width(self, k: int) -> int:
        return int(self.drm.rank_max[k] - self.drm.rank_min[k])

    def full(self, k: int) -> int:
        """columns of a table of level k: a train's partial products keep the whole rank (a chain goes on from them; a
        rank slice cuts the last core only), a hashed DRM's rows only the columns it hands out"""
        return int(self.drm.true_rank[k]) if self.tt else self.width(k)

    def staged(self, k: int) -> int:
        """columns of the staged tile a factor sampled in the pass needs: a sign row is made whole (its swaps reach
        every position), a Gaussian row only where it is used"""
        return int(self.drm.true_rank[k]) if self.sign else self.width(k)

    def seed(self, k: int) -> int:
        return (k + int(self.drm.seed)) % 2**63            # sparse_gaussian_drm.py:34-36, sparse_sign_drm.py:39-41

    def prefixes(self, k: int) -> int:
        return int(np.prod([int(n) for n in self.shape[:k + 1]], dtype=object))

    def use_table(self, k: int) -> bool:
        P = self.prefixes(k)
        return P < 2**31 and 2 * P <= self.nnz and P * self.full(k) * 8 <= TABLE_BYTES

    # ---- a tensor-train DRM: tables of its partial products up to a start level, chain steps through its cores beyond
    def start_level(self, k: int) -> int:
        """the deepest level <= k that has a table of partial products, every level below it too (each table is built from
        the one before); -1: none, a chain starts at the first core"""
        k0 = -1
        while k0 < k and self.use_table(k0 + 1):
            k0 += 1
        return k0

    def _tt_table(self, k: int) -> DevArray:
        """T_k[flat, :] = D_0[0, i_0, :] D_1[:, i_1, :] ... D_k[:, i_k, :], flat = i_0 + n_0 (i_1 + n_1 (...)): from T_{k-1}
        and D_k by one ``contract``; once per DRM (and its copies, which share the dictionary) and level, keyed by the
        core objects, which the entry holds so that no other core takes their identity"""
        cores = tuple(self.drm.cores[:k + 1])
        key = ("tt", k, self.shape[:k + 1], tuple(id(c) for c in cores))
        if key not in self.cache:
            D = self.drm.dev_cores()[k]
            P, rho = self.prefixes(k), self.full(k)
            out = DevArray.zeros((P + 1, rho))             # (one spare row, as every table)
            if k == 0:
                copy_into(out[:P], D[0])
            else:
                Pp = self.prefixes(k - 1)
                contract("pa,aib->ipb", self._tt_table(k - 1)[:Pp], D, out=out[:P].reshape(self.shape[k], Pp, rho))
            self.cache[key] = (out, cores)
        return self.cache[key][0]

    def _tt_cut(self, k: int) -> DevArray:
        """columns rank_min:rank_max of T_k as a table of their own (a rank slice whose level has a table)"""
        lo, hi = int(self.drm.rank_min[k]), int(self.drm.rank_max[k])
        cores = tuple(self.drm.cores[:k + 1])
        key = ("tt cut", k, self.shape[:k + 1], tuple(id(c) for c in cores), lo, hi)
        if key not in self.cache:
            P = self.prefixes(k)
            out = DevArray.zeros((P + 1, hi - lo))
            copy_into(out[:P], self._tt_table(k)[:P, lo:hi])
            self.cache[key] = (out, cores)
        return self.cache[key][0]

    def _tt_factor(self, k: int, src: int, mul: int):
        lo, w = int(self.drm.rank_min[k]), self.width(k)
        k0 = self.start_level(k)
        if k0 == k:                                        # the level itself has a table: a plain table factor
            tab = self._tt_table(k) if w == self.full(k) else self._tt_cut(k)
            return _Factor(1, w, lo, src, mul, 0, tab.ptr, 0, 0), tab
        tab = self._tt_table(k0) if k0 >= 0 else None
        devs = [self.drm.dev_cores()[j].contiguous() for j in range(k0 + 1, k + 1)]
        ch = _Chain()
        ch.steps, ch.rows = k - k0, self.prefixes(k0) if k0 >= 0 else 0
        ch.rank[0] = self.full(k0) if k0 >= 0 else 1
        for s, D in enumerate(devs):
            ch.core[s], ch.n[s], ch.rank[s + 1] = D.ptr, self.shape[k0 + 1 + s], self.full(k0 + 1 + s)
        f = _Factor(4, w, lo, src, 0, 0, tab.ptr if tab is not None else None, 0, 0, ctypes.pointer(ch))
        return f, (tab, devs, ch)

    # ---- a Khatri-Rao DRM: tables of the rows of every prefix, per (level, columns), up to a start level; beyond, a chain
    # of diagonal steps (kind 5) through column cuts of its matrices.  Table and chain multiply in the same order, mode by
    # mode with one rounding each, so a row has the same bits wherever the table ends.
    def _kr_use_table(self, j: int, w: int) -> bool:
        P = self.prefixes(j)
        return P < 2**31 and 2 * P <= self.nnz and P * w * 8 <= TABLE_BYTES

    def _kr_start(self, k: int) -> int:
        """``start_level`` for the columns of level k: the tables below it hold those columns"""
        k0 = -1
        while k0 < k and self._kr_use_table(k0 + 1, self.width(k)):
            k0 += 1
        return k0

    def _kr_table(self, j: int, lo: int, hi: int) -> DevArray:
        """T_j[flat, :] = G_0[i_0, lo:hi] * G_1[i_1, lo:hi] * ... * G_j[i_j, lo:hi] (left to right), flat as ``_tt_table``:
        from T_{j-1} by one ``ttsk_kr_rows``; keyed by the matrices, which the entry holds"""
        mats = tuple(self.drm.mats[:j + 1])
        key = ("kr", j, self.shape[:j + 1], tuple(id(m) for m in mats), lo, hi)
        if key not in self.cache:
            G = self.drm.dev_cols(j, lo, hi)
            out = DevArray.zeros((self.prefixes(j) + 1, hi - lo))           # (one spare row, as every table)
            prev = self._kr_table(j - 1, lo, hi) if j else None
            nat.call("ttsk_kr_rows", prev, self.prefixes(j - 1) if j else 1, G, self.shape[j], hi - lo, out, 0)
            self.cache[key] = (out, mats)
        return self.cache[key][0]

    def _kr_factor(self, k: int, src: int, mul: int):
        lo, hi, w = int(self.drm.rank_min[k]), int(self.drm.rank_max[k]), self.width(k)
        k0 = self._kr_start(k)
        if k0 == k:                                        # the level itself has a table: a plain table factor
            tab = self._kr_table(k, lo, hi)
            return _Factor(1, w, lo, src, mul, 0, tab.ptr, 0, 0), tab
        tab = self._kr_table(k0, lo, hi) if k0 >= 0 else None
        devs = [self.drm.dev_cols(j, lo, hi) for j in range(k0 + 1, k + 1)]
        ch = _Chain()
        ch.steps, ch.rows = k - k0, self.prefixes(k0) if k0 >= 0 else 0
        ch.rank[0] = w
        for s, G in enumerate(devs):
            ch.core[s], ch.n[s], ch.rank[s + 1] = G.ptr, self.shape[k0 + 1 + s], w
        f = _Factor(5, w, 0, src, 0, 0, tab.ptr if tab is not None else None, 0, 0, ctypes.pointer(ch))
        return f, (tab, devs, ch)

    def table(self, k: int) -> DevArray:
        drm = self.drm
        key = (k, self.shape[:k + 1], int(drm.rank_min[k]), int(drm.rank_max[k]), int(drm.seed))
        if self.sign:
            key += (int(drm.true_rank[k]), int(drm.nnz[k]))
        if key not in self.cache:
            # (one spare row: the pass kernel fetches rows in 16-byte units, the last unit of an odd row reaches 8 bytes on)
            out = DevArray.empty((self.prefixes(k) + 1, self.width(k)))
            if self.sign:
                nat.call("ttsk_sparse_sign_table", _u64(self.shape[:k + 1]), k + 1, int(drm.true_rank[k]), int(drm.rank_min[k]),
                         int(drm.rank_max[k]), int(drm.nnz[k]), self.seed(k), out, 0)
            else:
                nat.call("ttsk_sparse_normal_table", _u64(self.shape[:k + 1]), k + 1, int(drm.rank_min[k]),
                         int(drm.rank_max[k]), self.seed(k), out, 0)
            self.cache[key] = out
        return self.cache[key]

    def factor(self, k: int, src: int, mul: int = 0) -> Tuple[_Factor, Optional[DevArray]]:
        """the factor of level k and what must outlive the pass that reads it"""
        if self.tt:
            return self._tt_factor(k, src, mul)
        if self.kr:
            return self._kr_factor(k, src, mul)
        tab = self.table(k) if self.use_table(k) else None
        kind = 1 if tab is not None else (3 if self.sign else 2)
        f = _Factor(kind, self.width(k), int(self.drm.rank_min[k]), src, mul, self.seed(k),
                    tab.ptr if tab is not None else None,
                    int(self.drm.true_rank[k]) if self.sign else 0, int(self.drm.nnz[k]) if self.sign else 0)
        return f, tab

    def cost(self, k: int) -> int:
        """what making the factor in the pass costs per nonzero (for choosing the side an Omega rides on): sampled columns;
        for a chain the multiply-adds of its steps, rank x rank each; w each for the diagonal steps of a Khatri-Rao DRM"""
        if self.tt:
            rk = [1] + [self.full(j) for j in range(k + 1)]
            return sum(rk[j] * rk[j + 1] for j in range(self.start_level(k) + 1, k + 1))
        if self.kr:
            return self.width(k) * (k - self._kr_start(k))
        return 0 if self.use_table(k) else self.width(k)

    def route_work(self, k: int) -> int:
        """``cost`` as the route's rule counts it: the steps through a core that does not stay in the L2 weigh more.  A
        Khatri-Rao step counts as its w multiply-adds -- by analogy with a train's step; nothing measured backs that count
        (the constants of ``chain_route_ms`` were fitted to train pairs only)."""
        if self.kr:
            return self.cost(k)
        rk = [1] + [self.full(j) for j in range(k + 1)]
        return sum(rk[j] * rk[j + 1] * (ROUTE_BIG_CORE_WEIGHT if rk[j] * self.shape[j] * rk[j + 1] * 8 > ROUTE_BIG_CORE_BYTES else 1)
                   for j in range(self.start_level(k) + 1, k + 1))

    def covered(self, k: int) -> bool:
        if not 1 <= self.width(k) <= MAX_WIDTH:
            return False
        if self.tt:                                       # every rank along the chain, the cores as the walk expects them
            rk = [1] + [self.full(j) for j in range(k + 1)]
            if max(rk) > MAX_WIDTH or int(self.drm.rank_max[k]) > rk[-1] or int(self.drm.rank_min[k]) < 0:
                return False
            if any(tuple(int(x) for x in self.drm.cores[j].shape) != (rk[j], self.shape[j], rk[j + 1]) for j in range(k + 1)):
                return False
            return k - self.start_level(k) <= CHAIN_MAX
        if self.kr:                                       # a matrix per level, as the walk expects it, with the rows the level hands out
            lo, hi = int(self.drm.rank_min[k]), int(self.drm.rank_max[k])
            if any(tuple(int(x) for x in m.shape)[1:] != (self.shape[j],) or not 0 <= lo < hi <= int(m.shape[0])
                   for j, m in enumerate(self.drm.mats[:k + 1])):
                return False
            return k - self._kr_start(k) <= CHAIN_MAX
        if self.sign and not self.use_table(k):
            return self.staged(k) <= MAX_WIDTH and 0 <= int(self.drm.nnz[k]) <= int(self.drm.true_rank[k])
        return True


def _small_stream(shape, mu: int) -> bool:
    """whether mode ``mu`` of a tensor of ``shape`` gets the 32-bit stream: every prefix and suffix extent below 2^31 (20
    instead of 28 bytes per record and pass; the only stream a chain factor takes)"""
    prod = lambda v: int(np.prod([int(n) for n in v] or [1], dtype=object))
    return prod(shape[:mu]) < 2**31 and prod(shape[mu + 1:]) < 2**31


def _mode_stream(tensor: SparseTensor, mu: int):
    """(fl, fr, j, val) of mode ``mu`` in mode order; built once per tensor and mode (shared with views)."""
    d, N = len(tensor.shape), tensor.nnz
    order = tensor.dev_row_order
    cache = tensor._upload()[2]
    key = ("stream", tuple(order), mu)
    if key not in cache:
        idx, val = tensor.dev_indices(), tensor.dev_entries()
        l_rows, l_shape = list(order[:mu]), list(tensor.shape[:mu])
        r_rows = [order[d - 1 - i] for i in range(d - 1 - mu)]
        r_shape = [tensor.shape[d - 1 - i] for i in range(d - 1 - mu)]
        ints = lambda v: (ctypes.c_int * max(len(v), 1))(*v)
        # mode order with the suffix as the secondary key (not the plain mode sort of dev_mode_perm): inside a slice the
        # rows of the right-hand DRM tables are then visited in ascending order
        perm = DevArray.empty((N,), dtype=np.int64)
        nat.call("ttsk_sparse_mode_order", idx, N, N, ints(r_rows), _u64(r_shape or [1]),
                 len(r_rows), int(order[mu]), int(tensor.shape[mu]), perm, 0)
        small = _small_stream(tensor.shape, mu)
        words = (N + 1) // 2 if small else N
        fl, fr = DevArray.empty((words,), dtype=np.int64), DevArray.empty((words,), dtype=np.int64)
        jj = DevArray.empty(((N + 1) // 2,), dtype=np.int64)          # int32 records
        vv = DevArray.empty((N,))
        nat.call("ttsk_sparse_mode_stream_u32" if small else "ttsk_sparse_mode_stream", idx, N, perm, N,
                 ints(l_rows), _u64(l_shape or [1]), len(l_rows), ints(r_rows), _u64(r_shape or [1]), len(r_rows), int(order[mu]),
                 val, fl, fr, jj, vv, 0)
        cache[key] = (fl, fr, jj, vv, small)
    return cache[key]


# The cost rule of the route, fitted to profiles/sparse_tt_bench.json (profiles/scripts/sparse_tt_bench.py; DESIGN.md
# section 17): milliseconds of a whole sketch.  The passes: a launch floor per mode, the stream, and the multiply-adds of the
# chain steps per nonzero; the panels: the launches of the generic driver per mode and the (nnz x rank) panels it writes
# and reads back.
ROUTE_MODE_MS = 0.06             # per mode, either route: launches, zeroing and read-back of a small Psi
ROUTE_STREAM_NS = 0.151          # passes, per nonzero and mode: the records and the products
ROUTE_FMA_NS = 0.000816          # passes, per nonzero and multiply-add of a chain step
ROUTE_MIN_NNZ = 500000           # passes: below this the waves' stretches are at their shortest and the time no longer falls
ROUTE_BIG_CORE_BYTES = 2 << 20   # a core beyond this does not stay in the L2: the rows a step gathers from it come from further away,
ROUTE_BIG_CORE_WEIGHT = 3        # and its multiply-adds count this many times (one measured shape: n = 10^4, ranks 10 and 15)
ROUTE_PANEL_NS = 0.01346         # panels, per nonzero and panel column: written by a step, read back by the products
ROUTE_PANEL_FMA_NS = 0.000547    # panels, per nonzero and multiply-add of a step


def chain_route_ms(nnz: int, d: int, chain_fma: int, panel_cols: int, panel_fma: int) -> Tuple[float, float]:
    """(ms of the passes, ms of the panel path) for a sparse tensor of ``nnz`` nonzeros and ``d`` modes sketched with a
    tensor-train DRM on at least one side; the other arguments are ``_route_inputs``'s"""
    kernel = d * ROUTE_MODE_MS + max(nnz, ROUTE_MIN_NNZ) * 1e-6 * (d * ROUTE_STREAM_NS + chain_fma * ROUTE_FMA_NS)
    composed = d * ROUTE_MODE_MS + nnz * 1e-6 * (panel_cols * ROUTE_PANEL_NS + panel_fma * ROUTE_PANEL_FMA_NS)
    return kernel, composed


def _riders(L: _Side, R: _Side, d: int) -> dict:
    """which pass carries Omega_mu: pass mu (with L_mu as the extra factor, sharing R_mu) or pass mu + 1 (with R_mu as
    the extra factor, sharing L_mu) -- whichever extra factor is cheaper to make; a pass carries one Omega"""
    rider = {}
    for mu in range(d - 1):
        nu = d - 2 - mu
        here = (mu not in rider, L.cost(mu))
        there = (R.cost(nu),)
        if here[0] and here[1] <= there[0]:
            rider[mu] = ("left", mu)
        else:
            rider[mu + 1] = ("right", mu)
    return rider


def _route_inputs(L: _Side, R: _Side, rider: dict, d: int) -> Tuple[int, int, int]:
    """what ``chain_route_ms`` is asked with, per nonzero: the (weighted) multiply-adds of the chain steps over all passes; the
    panel columns of both DRMs over all levels; the multiply-adds of the panel path's steps, rank x rank per level of a train"""
    work = sum(L.route_work(mu - 1) for mu in range(1, d) if L.chained) + sum(R.route_work(d - 2 - mu) for mu in range(d - 1) if R.chained)
    work += sum(S.route_work(k) for S, k in ((L, k) if side == "left" else (R, d - 2 - k) for side, k in rider.values()) if S.chained)
    panels = sum(S.full(k) for S in (L, R) for k in range(d - 1))
    panel_fma = sum((S.full(k - 1) if k else 1) * S.full(k) for S in (L, R) if S.tt for k in range(d - 1))
    panel_fma += sum(S.width(k) for S in (L, R) if S.kr for k in range(d - 1))      # (a Khatri-Rao panel step: w products)
    return work, panels, panel_fma


def try_sparse_gauss_sketch(tensor, left_drm, right_drm, method):
    """(Psi, Omega) device arrays through the one-pass-per-mode path, or None if it does not apply."""
    if method != SketchMethod.streaming or os.environ.get("TTSK_SPARSE_FUSED", "1") == "0":
        return None
    if type(tensor) is TensorSum and tensor.tensors and all(type(t) is SparseTensor for t in tensor.tensors):
        # a sum of sparse tensors (the nnz shards of distributed.shard_tensor, reference tensor.py:215-234): every summand
        # through the passes, summed in the order of the summands -- as the reference's += (sketch_dispatch.py:85-139)
        # and, like the passes themselves, the same bits in every run
        parts = [try_sparse_gauss_sketch(t, left_drm, right_drm, method) for t in tensor.tensors if t.nnz]
        if not parts or any(p is None for p in parts):
            return None
        Psi, Omega = parts[0]
        for P2, O2 in parts[1:]:
            for y, x in zip(Psi + Omega, P2 + O2):
                axpby(y, x)
        return Psi, Omega
    if type(tensor) is not SparseTensor:
        return None
    shape = tuple(int(n) for n in tensor.shape)
    d, N = len(shape), tensor.nnz
    if d < 2 or N == 0 or N >= 2**31:
        return None
    if max(shape) > MAX_MODE:
        return None
    if not drm_pair(shape, left_drm, right_drm, kinds=(SparseGaussianDRM, SparseSignDRM, TensorTrainDRM, KhatriRaoDRM), cores=False):
        return None
    L = _Side(left_drm, shape, N)
    R = _Side(right_drm, shape[::-1], N)          # factor nu of the right DRM = suffix of d - 1 - nu.. = R_mu with mu = d - 2 - nu
    if any(S.tt and len(S.drm.cores) != d - 1 for S in (L, R)) or any(S.kr and len(S.drm.mats) != d - 1 for S in (L, R)):
        return None
    if (L.chained or R.chained) and not all(_small_stream(shape, mu) for mu in range(d)):
        return None                               # a chain factor reads the digits of a flat index that did not wrap
    if any(not L.covered(k) or not R.covered(k) for k in range(d - 1)):
        return None
    rider = _riders(L, R, d)
    if (L.kr or R.kr) and not (L.tt or R.tt):
        # Khatri-Rao and hashed DRMs in any pairing take the passes, as pairs of hashed DRMs do; only a forced "composed"
        # (tests, benchmarks) gives the pair to the panels of the generic driver
        if paths.resolve(None) == "composed":
            return None
    if L.tt or R.tt:
        # the route (pairs of two hashed DRMs have this path only): "composed" is the panels of TensorTrainDRM.sketch_sparse
        # and the atomics of ttsk_sparse_psi -- a decline, the generic driver runs them
        route = paths.resolve(None)
        if route is None:
            route = paths.taken(None, *chain_route_ms(N, d, *_route_inputs(L, R, rider, d)))
        if route == "composed":
            return None
    tensor.prepare_device()
    multL, multR = _flat_mult(shape), _flat_mult(shape[::-1])
    lw = lambda mu: L.width(mu)
    rw = lambda mu: R.width(d - 2 - mu)
    Psi, Omega, keep = [], [None] * (d - 1), []
    sampled, chain_steps = 0, 0
    for mu in range(d):
        fl, fr, jj, vv, small = _mode_stream(tensor, mu)
        A = B = C = None
        if mu > 0:
            A, t = L.factor(mu - 1, 0)
            keep.append(t)
        if mu < d - 1:
            B, t = R.factor(d - 2 - mu, 1)
            keep.append(t)
        psi = DevArray.zeros((lw(mu - 1) if mu > 0 else 1, shape[mu], rw(mu) if mu < d - 1 else 1))
        om, c_left = None, 0
        if mu in rider:
            side, k = rider[mu]
            om = DevArray.zeros((lw(k), rw(k)))
            Omega[k] = om
            if side == "left":          # Omega_mu = L_mu (x) R_mu: L_mu's flat index = prefix + j * multiplier of mode mu
                C, t = L.factor(k, 2, multL[k])
                c_left = 1
            else:                       # Omega_{mu-1} = L_{mu-1} (x) R_{mu-1}: R_{mu-1}'s flat index = suffix + j * multiplier
                C, t = R.factor(d - 2 - k, 3, multR[d - 2 - k])
            keep.append(t)
        for f in (A, B, C):
            if f is not None and f.kind in (2, 3):
                sampled += f.w
            if f is not None and f.kind in (4, 5):
                chain_steps += f.chain.contents.steps
        ref = lambda f: None if f is None else ctypes.byref(f)
        nat.call("ttsk_sparse_gauss_pass_u32" if small else "ttsk_sparse_gauss_pass", fl, fr, jj, vv, N, int(shape[mu]),
                 ref(A), ref(B), ref(C), c_left, psi, om, 0)
        Psi.append(psi)
    last_plan.clear()
    last_plan.update(sampled_columns_per_nonzero=sampled, passes=d, stream_bytes_per_nonzero_and_pass=20 if small else 28,
                     riders={int(k): v for k, v in rider.items()}, chain_steps_per_nonzero=chain_steps)
    return Psi, Omega
