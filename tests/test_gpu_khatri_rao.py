"""KhatriRaoDRM on the device: the two entry points of csrc/khatri_rao.hip, the diagonal chain factor of the one-pass sparse
kernel (kind 5 of ttsk_sg_factor) and the DRM at the API.

Exact parts: integer data.  Tables and matrices with entries in [-2, 2], values in [-3, 3]: a row after a start table and
eight steps is at most 2^9 in size, a term of a sum at most 3 * 2^18, and there are fewer than 2^17 terms -- every partial
sum in any order is an exact double, so the device must give the int64 reference bit for bit.  Every table carries its spare
row filled with 2^40; outputs sit between guard bands; scratch is poisoned by the sentinel of tests/edge_kit.py where an
entry point writes a whole array.

The API parts compare against tests/khatri_rao_ref.py (the sketching matrices by their definition) at 1e-12 in the
Frobenius norm per array, the bar of DESIGN section 3."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

from tests import khatri_rao_ref as kref
from tests import sparse_cases as sc
from tests import sparse_chain_ref as cref
from tests.edge_kit import SENT, assert_guards, exact, guarded, rel_fro, same_bits, tsa  # noqa: F401

pytestmark = pytest.mark.gpu

SPARE = float(2 ** 40)
GUARD = 64
STRUCTURES = {s.name: s for s in sc.structures()}
P_OTHER = 13


# ================================================================== the two entry points
def _dev(a):
    from tt_sketch_amd.device import DevArray
    return DevArray.from_host(np.ascontiguousarray(a))


def _ints(rng, shape, lo=-2, hi=2):
    return rng.integers(lo, hi + 1, shape).astype(np.float64)


def _guarded_out(shape, extra_rows=0):
    """(device buffer, view of `shape` inside guard bands of sentinels; `extra_rows` more rows belong to the caller)"""
    size = int(np.prod(shape))
    host = guarded(np.full(size, SENT, dtype=np.uint64).view(np.float64), GUARD, GUARD + extra_rows * shape[-1])
    buf = _dev(host)
    return buf, buf[GUARD:GUARD + size].reshape(*shape)


def _read(buf, shape, what, extra=0):
    whole = buf.get()
    size = int(np.prod(shape))
    assert_guards(whole, [(GUARD, (size,), (1,))], what)
    return whole[GUARD:GUARD + size].reshape(shape)


@pytest.mark.parametrize("w", [1, 15, 16, 17, 32])
@pytest.mark.parametrize("n", [1, 2, 37])
def test_kr_rows_bit_for_bit(tsa, n, w):
    from tt_sketch_amd import _native as nat
    rng = np.random.default_rng(1000 * n + w)
    g = _ints(rng, (n, w))
    for P in (1, 31, 32, 33, 2049):
        prev = _ints(rng, (P, w))
        for with_prev in ((False, True) if P == 1 else (True,)):
            buf, out = _guarded_out((n * P, w), extra_rows=1)         # (the spare row of a table: the entry leaves it alone)
            nat.call("ttsk_kr_rows", _dev(prev) if with_prev else None, P, _dev(g), n, w, out, 0)
            got = _read(buf, (n * P, w), ("rows", n, w, P))
            want = ((prev if with_prev else np.ones((1, w)))[None, :, :] * g[:, None, :]).reshape(n * P, w)
            same_bits(got, want, ("ttsk_kr_rows", n, w, P, with_prev))


@pytest.mark.parametrize("w", [1, 15, 16, 17, 32])
@pytest.mark.parametrize("n", [1, 2, 37])
def test_kr_step_bit_for_bit(tsa, n, w):
    from tt_sketch_amd import _native as nat
    rng = np.random.default_rng(2000 * n + w)
    g = _ints(rng, (n, w))
    dg = _dev(g)
    for N in (1, 31, 32, 33, 2049):
        v = _ints(rng, (N, w), -3, 3)
        idx = rng.integers(0, n, N).astype(np.int64)
        idx[0], idx[-1] = n - 1, n - 1
        for with_v in (False, True):
            for with_idx in ((False, True) if N <= n else (True,)):
                buf, out = _guarded_out((N, w))
                nat.call("ttsk_kr_step", _dev(v) if with_v else None, dg, n, w, _dev(idx) if with_idx else None, N, out, 0)
                want = (v if with_v else 1.0) * (g[idx] if with_idx else g[:N])
                same_bits(_read(buf, (N, w), ("step", n, w, N)), want, ("ttsk_kr_step", n, w, N, with_v, with_idx))
        # in place: out is v
        host = guarded(v, GUARD, GUARD)
        buf = _dev(host)
        view = buf[GUARD:GUARD + N * w].reshape(N, w)
        nat.call("ttsk_kr_step", view, dg, n, w, _dev(idx), N, view, 0)
        same_bits(_read(buf, (N, w), ("step in place", n, w, N)), v * g[idx], ("ttsk_kr_step in place", n, w, N))


def test_kr_entry_refusals_write_nothing(tsa):
    from tt_sketch_amd import _native as nat
    g, v = _dev(np.ones((4, 3))), _dev(np.ones((5, 3)))
    idx = _dev(np.zeros(5, dtype=np.int64))
    for entry, args in (("ttsk_kr_rows", lambda out: (None, 2, g, 4, 3, out, 0)), ("ttsk_kr_rows", lambda out: (v, 5, g, 0, 3, out, 0)),
                        ("ttsk_kr_step", lambda out: (v, g, 4, 3, None, 5, out, 0)), ("ttsk_kr_step", lambda out: (v, g, 4, 0, idx, 5, out, 0))):
        buf, out = _guarded_out((20, 3))
        with pytest.raises(ValueError):
            nat.call(entry, *args(out))
        assert (buf.get().view(np.uint64) == SENT).all(), entry
    with pytest.raises(ValueError):
        nat.call("ttsk_kr_step", v, None, 4, 3, idx, 5, v, 0)


# ================================================================== the pass with kind-5 factors
# rows: of the start table (0: the vector of ones); modes: the mode size of every step -- None is the number of slices (a C
# factor's last digit is the record's mode index); [lo, lo + w) of the rho columns
Diag = namedtuple("Diag", "rows modes rho lo w")
Tab = namedtuple("Tab", "w")
Cfg = namedtuple("Cfg", "name A B C c_left", defaults=(None, 0))


def diag(rows, modes, rho, lo=0, w=None):
    return Diag(rows, tuple(modes), rho, lo, rho - lo if w is None else w)


def _packed(a, dtype):
    a = np.asarray(a, dtype=dtype)
    if a.size & 1:
        a = np.concatenate([a, np.zeros(1, dtype=dtype)])
    return _dev(a.view(np.int64))


def _extent(F, n):
    ns = [n if m is None else m for m in F.modes]
    if any(m is None for m in F.modes):
        ns = ns[:-1]
    return max(F.rows, 1) * int(np.prod(ns, dtype=object))


class Case:
    """one call of ttsk_sparse_gauss_pass_u32 with hand-made streams; ``embed`` states every kind-5 factor as the kind-4
    factor of its diagonal embedding (cores (rho, n, rho), the first one (1, n, rho) without a table)"""

    def __init__(self, cfg, st, seed, embed=False):
        from tt_sketch_amd.sparse_fused import _Chain, _Factor
        rng = np.random.default_rng(seed)
        self.cfg, self.st = cfg, st
        j, n = st.j.astype(np.int64), st.n
        N = self.N = j.size
        ext = [None, None]
        for F, side in ((cfg.A, 0), (cfg.B, 1), (cfg.C, 0 if cfg.c_left else 1)):
            if isinstance(F, Diag):
                e = _extent(F, n)
                assert ext[side] in (None, e), "two chain factors on one stream disagree about its extent"
                ext[side] = e
        Pl, Pr = (e if e is not None else P_OTHER for e in ext)
        fl, fr = rng.integers(0, Pl, N), rng.integers(0, Pr, N)
        fl[0] = fl[-1] = Pl - 1
        fr[0] = fr[-1] = Pr - 1
        self.v = rng.integers(-3, 4, N).astype(np.int64)
        self.keep, self.factors, self.rows = [], [], []
        for i, F in enumerate((cfg.A, cfg.B, cfg.C)):
            if F is None:
                self.factors.append(None)
                self.rows.append(np.ones((N, 1), dtype=np.int64))
                continue
            src = i if i < 2 else (2 if cfg.c_left else 3)
            base, P = (fr, Pr) if src & 1 else (fl, Pl)
            mul = P if src & 2 else 0
            if isinstance(F, Tab):
                nrows = P * n if src & 2 else P
                t = rng.integers(-2, 3, (nrows, F.w))
                dev = _dev(np.vstack([t, np.full((1, F.w), SPARE)]).astype(np.float64))
                self.keep.append(dev)
                self.factors.append(_Factor(1, F.w, 0, src, mul, 0, dev.ptr, 0, 0))
                self.rows.append(t[base + j * mul])
                continue
            ns = [n if m is None else m for m in F.modes]
            G = [rng.integers(-2, 3, (m, F.rho)) for m in ns]
            tab = rng.integers(-2, 3, (F.rows, F.rho)) if F.rows else None
            row, idx = cref.digits(base, F.rows, ns, j if src & 2 else None)
            r = tab[row] if tab is not None else np.ones((N, F.rho), dtype=np.int64)
            for Gs, i_s in zip(G, idx):
                r = r * Gs[i_s]
            self.rows.append(r[:, F.lo:F.lo + F.w])
            ch = _Chain()
            ch.steps, ch.rows = len(ns), F.rows
            for s in range(len(ns) + 1):
                ch.rank[s] = F.rho
            if embed and tab is None:
                ch.rank[0] = 1
            for s, Gs in enumerate(G):
                if embed:
                    rin = 1 if (s == 0 and tab is None) else F.rho
                    D = np.zeros((rin, ns[s], F.rho))
                    if rin == 1:
                        D[0] = Gs
                    else:
                        D[np.arange(F.rho), :, np.arange(F.rho)] = Gs.T
                    dev = _dev(D)
                else:
                    dev = _dev(Gs.astype(np.float64))
                self.keep.append(dev)
                ch.core[s], ch.n[s] = dev.ptr, ns[s]
            dtab = None
            if tab is not None:
                dtab = _dev(np.vstack([tab, np.full((1, F.rho), SPARE)]).astype(np.float64))
                self.keep.append(dtab)
            self.keep.append(ch)
            self.factors.append(_Factor(4 if embed else 5, F.w, F.lo, src, 0, 0, dtab.ptr if dtab is not None else None, 0, 0,
                                        ctypes.pointer(ch)))
        self.dev_j = _packed(st.j, np.int32)
        self.dev_v = _dev(self.v.astype(np.float64))
        self.dev_fl, self.dev_fr = _packed(fl, np.uint32), _packed(fr, np.uint32)

    def reference(self):
        A, B, C = self.rows
        v = self.v[:, None]
        psi = sc.segmented_outer(self.st.j, self.st.n, v * A, B)
        om = None
        if self.cfg.C is not None:
            om = (v * C).T @ B if self.cfg.c_left else (v * A).T @ C
        return psi, om

    def run(self):
        from tt_sketch_amd import _native as nat
        wA, wB, wC = (r.shape[1] for r in self.rows)
        shapes = [(wA, self.st.n, wB), None if self.cfg.C is None else ((wC, wB) if self.cfg.c_left else (wA, wC))]
        bufs = []
        for shape in shapes:
            if shape is None:
                bufs.append((None, None))
                continue
            size = int(np.prod(shape))
            buf = _dev(guarded(np.zeros(size), GUARD, GUARD))
            bufs.append((buf, buf[GUARD:GUARD + size].reshape(*shape)))
        byref = lambda f: None if f is None else ctypes.byref(f)
        A, B, C = self.factors
        nat.call("ttsk_sparse_gauss_pass_u32", self.dev_fl, self.dev_fr, self.dev_j, self.dev_v, self.N, self.st.n, byref(A), byref(B),
                 byref(C), self.cfg.c_left, bufs[0][1], bufs[1][1], 0)
        return [None if buf is None else _read(buf, shape, (self.cfg.name, "guards")) for (buf, _), shape in zip(bufs, shapes)]


def _check(cfg, st, seed, what):
    case = Case(cfg, st, seed)
    psi_ref, om_ref = case.reference()
    psi, om = case.run()
    assert np.abs(psi).max() < SPARE / 2 and (om is None or np.abs(om).max() < SPARE / 2), (what, "a spare table row reached a stored cell")
    exact(psi, psi_ref.astype(np.float64), "%s Psi" % (what,))
    if om_ref is not None:
        exact(om, om_ref.astype(np.float64), "%s Omega" % (what,))
    same_bits([psi, om], case.run(), "%s: a second call" % (what,))
    same_bits([psi, om], Case(cfg, st, seed, embed=True).run(), "%s: the kind-4 factor of the diagonal embedding" % (what,))


def _runs(N, n=1):
    return sc._st(f"N{N}-n{n}", np.sort(np.arange(N) % n), n)


def _positions(w, modes, rows):
    """a kind-5 factor of width w as A, as B, and as C with src 2 (c_left) and src 3; the C factor's last step is the
    record's mode"""
    rho = w
    f = diag(rows, modes, rho)
    fc = diag(rows, tuple(modes[:-1]) + (None,), rho)
    short = diag(rows, modes[:-1], rho) if (len(modes) > 1 or rows) else Tab(w)
    other = Tab(min(w, 6))
    return [Cfg("A-src0", f, other, None), Cfg("B-src1", other, f, None), Cfg("A-and-B", f, f, None),
            Cfg("C-src2", short if isinstance(short, Diag) else None, other, fc, 1),
            Cfg("C-src3", other, short if isinstance(short, Diag) else None, fc, 0)]


MODES = {1: (5,), 2: (4, 3), 8: (2, 3, 2, 2, 3, 2, 2, 3)}


@pytest.mark.parametrize("w", [1, 16, 17, 32])
@pytest.mark.parametrize("table", [False, True])
@pytest.mark.parametrize("steps", [1, 2, 8])
def test_diagonal_chain_exact_in_every_position(tsa, steps, table, w):
    """1, 2 and 8 steps after a start table and from the vector of ones, widths on either side of the two tile sizes, as A
    (src 0), B (src 1) and C (src 2 with c_left, src 3 without): over slices that straddle waves and a single slice"""
    rows = 7 if table else 0
    for k, cfg in enumerate(_positions(w, MODES[steps], rows)):
        for st in (STRUCTURES["runs57"], STRUCTURES["single257-equal"]):
            _check(cfg, st, 100 * steps + 10 * k + w, (cfg.name, steps, table, w, st.name))


@pytest.mark.parametrize("N", [1, 31, 32, 33, 2049])
def test_diagonal_chain_stream_lengths(tsa, N):
    for n in (1, 3):
        if n > N:
            continue
        for cfg in _positions(9, MODES[2], 7)[2:4]:
            _check(cfg, _runs(N, n), 300 + N, (cfg.name, N, n))


def test_diagonal_chain_over_many_workgroups(tsa):
    """sg_plan gives a wave 256 records while N <= 256 * (resident waves), so 66000 records are 258 waves in 65 workgroups;
    the first and last slices of most waves are shared"""
    st = sc._st("long", np.concatenate([np.zeros(30000), np.ones(1), np.full(35999, 2)]), 3)
    for cfg in _positions(10, MODES[2], 7)[2:5]:
        _check(cfg, st, 31, (cfg.name, st.name))


def test_diagonal_chain_rank_slice_zero_steps_and_slice_structures(tsa):
    cfgs = [Cfg("slice-3-8-of-9", diag(7, (4, 3), 9, lo=3, w=5), Tab(5), None),
            Cfg("table-0-steps", diag(17, (), 6, lo=1, w=4), Tab(5), Tab(7)),
            Cfg("mode-of-extent-1", diag(0, (1, 5, 1), 4), Tab(5), None),
            Cfg("three-wide", diag(7, (4,), 32), diag(5, (3,), 32), diag(7, (4, None), 32), 1)]
    for k, cfg in enumerate(cfgs):
        for st in (STRUCTURES["skewed"], STRUCTURES["tail-opens"], STRUCTURES["arange"], STRUCTURES["one"]):
            if isinstance(cfg.C, Tab) and st.n > 64:
                continue
            _check(cfg, st, 500 + k, (cfg.name, st.name))


def test_diagonal_chain_refusals_leave_psi_as_it_was(tsa):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    from tt_sketch_amd.sparse_fused import _Chain, _Factor
    N, n = 40, 3
    rng = np.random.default_rng(5)
    fl32, fr32 = (_packed(rng.integers(0, 5, N), np.uint32) for _ in range(2))
    fl64, fr64 = (DevArray.from_host(rng.integers(0, 5, N).astype(np.uint64)) for _ in range(2))
    jj = _packed(np.sort(rng.integers(0, n, N)), np.int32)
    val = _dev(np.ones(N))
    core, tab = _dev(np.ones((5, 40))), _dev(np.ones((6, 40)))
    fill = np.full((32, n, 32), 7.0)
    keep = []

    def factor(ranks, steps=1, rows=0, table=False, lo=0, w=2, n_mode=5, null=None):
        ch = _Chain()
        ch.steps, ch.rows = steps, rows
        for s in range(min(steps, len(ch.core))):
            ch.core[s], ch.n[s] = (None if s == null else core.ptr), n_mode
        for s, r in enumerate(ranks):
            ch.rank[s] = r
        keep.append(ch)
        return _Factor(5, w, lo, 0, 0, 0, tab.ptr if table else None, 0, 0, ctypes.pointer(ch))

    u32 = "ttsk_sparse_gauss_pass_u32"
    refused = {
        "unequal ranks": (u32, factor((4, 5)), ValueError),
        "unequal ranks behind a table": (u32, factor((4, 4, 3), steps=2, rows=6, table=True), ValueError),
        "rank 33": (u32, factor((33, 33)), nat.TtskUnsupported),
        "nine steps": (u32, factor((4,) * 9, steps=9), nat.TtskUnsupported),
        "64-bit streams": ("ttsk_sparse_gauss_pass", factor((4, 4)), nat.TtskUnsupported),
        "NULL core": (u32, factor((4, 4, 4), steps=2, null=1), ValueError),
        "no descriptor": (u32, _Factor(5, 2, 0, 0, 0, 0, None, 0, 0), ValueError),
        "neither a table nor a core": (u32, factor((4,), steps=0), ValueError),
        "rows without a table": (u32, factor((4, 4), rows=5), ValueError),
        "table without rows": (u32, factor((4, 4), table=True), ValueError),
        "columns beyond the rank": (u32, factor((4, 4), lo=3, w=2), ValueError),
        "kind 6": (u32, _Factor(6, 2, 0, 0, 0, 0, None, 0, 0), ValueError),
    }
    for what, (entry, A, exc) in refused.items():
        fl, fr = (fl32, fr32) if entry == u32 else (fl64, fr64)
        psi = DevArray.from_host(fill)
        with pytest.raises(exc):
            nat.call(entry, fl, fr, jj, val, N, n, ctypes.byref(A), None, None, 0, psi, None, 0)
        assert np.array_equal(psi.get(), fill), what


# ================================================================== the API
SHAPE = (6, 5, 4, 7)
LEFT, RIGHT = (4, 5, 6), (5, 6, 7)


@pytest.fixture(scope="module")
def inputs(tsa):
    """the five tensor kinds of shape (6, 5, 4, 7) and their dense images; the reference sketch of each is computed once"""
    rng = np.random.default_rng(42)
    tt = tsa.TensorTrain.random(SHAPE, 3, seed=1)
    cp = tsa.CPTensor.random(SHAPE, 3, seed=2)
    tk = tsa.TuckerTensor.random(SHAPE, 3, seed=3)
    X = tt.to_numpy()
    flat = rng.choice(int(np.prod(SHAPE)), 100, replace=False)            # 100 of 840 entries: the deepest level has no table
    idx = np.array(np.unravel_index(flat, SHAPE))
    Xs = np.zeros(SHAPE)
    Xs[tuple(idx)] = X[tuple(idx)]
    sp = tsa.SparseTensor(SHAPE, idx, X[tuple(idx)])
    tensors = {"tt": (tt, X), "cp": (cp, cp.to_numpy()), "tucker": (tk, tk.to_numpy()), "dense": (tsa.DenseTensor(X), X), "sparse": (sp, Xs)}
    left = tsa.KhatriRaoDRM(LEFT, SHAPE, False, seed=11)
    right = tsa.KhatriRaoDRM(RIGHT, SHAPE, True, seed=12)
    refs = {k: kref.sketch(D, kref.of_drm(left), kref.of_drm(right)) for k, (_, D) in tensors.items()}
    return tensors, left, right, refs


def _arrays(stt):
    return [np.asarray(a) for a in list(stt.Psi_cores) + list(stt.Omega_mats)]


def _close(got, want, what, bar=1e-12):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, (what, i, a.shape, b.shape)
        r = rel_fro(a, b)
        print("%s[%d]: %.3e" % (what, i, r))
        assert r <= bar, (what, i, r)


def test_sampled_matrices(tsa, inputs):
    """(R, n_s) per walked mode, the seeds of the issue, leading rows unchanged when R grows"""
    from tt_sketch_amd.utils import random_normal_dev
    _, left, right, _ = inputs
    for drm, walk in ((left, SHAPE), (right, SHAPE[::-1])):
        R = max(drm.true_rank)
        assert [tuple(m.shape) for m in drm.mats] == [(R, n) for n in walk[:-1]]
        for s, m in enumerate(drm.mats):
            want = random_normal_dev((R + 3, walk[s]), seed=(drm.seed << 20) + 0x4B520000 + s).get()
            same_bits(np.asarray(m), want[:R], ("mats", s))
    grown = left.increase_rank((6, 7, 9))
    for a, b in zip(left.mats, grown.mats):
        same_bits(np.asarray(a), np.asarray(b)[:a.shape[0]], "increase_rank")


@pytest.mark.parametrize("kind", ["tt", "cp", "tucker", "dense"])
def test_stream_sketch_against_the_definition(tsa, inputs, kind):
    tensors, left, right, refs = inputs
    stt = tsa.stream_sketch(tensors[kind][0], LEFT, RIGHT, left_drm=left, right_drm=right)
    _close(_arrays(stt), refs[kind][0] + refs[kind][1], kind)


def test_stream_sketch_of_a_train_on_both_chain_routes(tsa, inputs):
    """``cp_fused.chain_step`` with the train's core in the place of the DRM core, and the two ``contract`` calls"""
    from tt_sketch_amd import paths
    tensors, left, right, refs = inputs
    for route in ("kernel", "composed"):
        with paths.forced(route):
            stt = tsa.stream_sketch(tensors["tt"][0], LEFT, RIGHT, left_drm=left, right_drm=right)
        _close(_arrays(stt), refs["tt"][0] + refs["tt"][1], "tt " + route)


def test_sparse_on_both_routes_and_twice(tsa, inputs):
    from tt_sketch_amd import paths, sparse_fused
    tensors, left, right, refs = inputs
    sp = tensors["sparse"][0]
    want = refs["sparse"][0] + refs["sparse"][1]
    sparse_fused.last_plan.clear()
    with paths.forced("composed"):
        _close(_arrays(tsa.stream_sketch(sp, LEFT, RIGHT, left_drm=left, right_drm=right)), want, "sparse composed")
    assert not sparse_fused.last_plan, "the panels were asked for, the passes ran"
    runs = []
    for route in (None, "kernel"):
        sparse_fused.last_plan.clear()
        with paths.forced(route):
            runs.append(_arrays(tsa.stream_sketch(sp, LEFT, RIGHT, left_drm=left, right_drm=right)))
        assert sparse_fused.last_plan["passes"] == 4 and sparse_fused.last_plan["chain_steps_per_nonzero"] > 0, sparse_fused.last_plan
        assert sparse_fused.last_plan["sampled_columns_per_nonzero"] == 0
        _close(runs[-1], want, "sparse passes")
    same_bits(runs[0], runs[1], "two runs of the passes")


@pytest.mark.parametrize("other", ["TensorTrainDRM", "SparseGaussianDRM"])
def test_sparse_mixed_with_another_drm(tsa, inputs, other):
    """a Khatri-Rao DRM on one side, a train or a hashed DRM on the other: the passes against the panels of the generic
    driver (which run the two DRMs' own ``sketch_sparse``), and the passes twice"""
    from tt_sketch_amd import paths, sparse_fused
    tensors, left, right, _ = inputs
    sp = tensors["sparse"][0]
    cls = getattr(tsa, other)
    for L, R in ((left, cls(RIGHT, SHAPE, True, seed=21)), (cls(LEFT, SHAPE, False, seed=22), right)):
        with paths.forced("composed"):
            want = _arrays(tsa.stream_sketch(sp, LEFT, RIGHT, left_drm=L, right_drm=R))
        if other == "SparseGaussianDRM":                       # no route asked: a pair with a hashed DRM takes the passes
            sparse_fused.last_plan.clear()
            tsa.stream_sketch(sp, LEFT, RIGHT, left_drm=L, right_drm=R)
            assert sparse_fused.last_plan["passes"] == 4 and sparse_fused.last_plan["sampled_columns_per_nonzero"] > 0
        runs = []
        for _ in range(2):
            sparse_fused.last_plan.clear()
            with paths.forced("kernel"):
                runs.append(_arrays(tsa.stream_sketch(sp, LEFT, RIGHT, left_drm=L, right_drm=R)))
            assert sparse_fused.last_plan["passes"] == 4
        _close(runs[0], want, "mixed " + other)
        same_bits(runs[0], runs[1], "two runs")


@pytest.mark.parametrize("kind", ["tt", "cp", "sparse"])
def test_orthogonal_and_hmt_recover_the_tensor(tsa, inputs, kind):
    """a tensor of TT rank 3 (the sparse one: every entry of it stored), sketch ranks above 3: both one-sided orthogonalising
    sketches give the tensor back, compared as tensors at 1e-8"""
    tensors, _, _, _ = inputs
    T, X = tensors[kind]
    if kind == "sparse":
        T, X = tensors["dense"][0].to_sparse(), tensors["dense"][1]
    o = tsa.orthogonal_sketch(T, LEFT, RIGHT, seed=5, left_drm_type=tsa.KhatriRaoDRM, right_drm_type=tsa.KhatriRaoDRM)
    h = tsa.hmt_sketch(T, RIGHT, seed=5, drm_type=tsa.KhatriRaoDRM)
    for name, out in (("orthogonal", o), ("hmt", h)):
        r = rel_fro(out.to_numpy(), X)
        print(kind, name, "%.3e" % r)
        assert r <= 1e-8, (kind, name, r)


def test_exact_recovery_of_a_rank_3_train(tsa):
    shape = (12, 11, 10, 13)
    T = tsa.TensorTrain.random(shape, 3, seed=9)
    stt = tsa.stream_sketch(T, 3, 5, seed=9, left_drm_type=tsa.KhatriRaoDRM, right_drm_type=tsa.KhatriRaoDRM)
    err = stt.to_tt().error(T, relative=True)
    print("recovery error %.3e" % err)
    assert err < 1e-9, err


def test_rank_growth(tsa):
    """increase_rank of a train's sketch from (4, 6) to (6, 9) and the blocked sketch over the same cuts against the fresh
    sketch at (6, 9) of the same seeds"""
    shape = (12, 11, 10, 13)
    T = tsa.TensorTrain.random(shape, 3, seed=9)
    k = len(shape) - 1
    l0, r0, l1, r1 = (4,) * k, (6,) * k, (6,) * k, (9,) * k
    ld, rd = tsa.KhatriRaoDRM(l0, shape, False, seed=31), tsa.KhatriRaoDRM(r0, shape, True, seed=32)
    small = tsa.stream_sketch(T, l0, r0, left_drm=ld, right_drm=rd)
    grown = small.increase_rank(T, l1, r1)
    assert type(grown.left_drm) is tsa.KhatriRaoDRM and grown.left_drm.rank == l1 and grown.right_drm.rank == r1
    ld2, rd2 = ld.increase_rank(l1), rd.increase_rank(r1)
    fresh = tsa.stream_sketch(T, l1, r1, left_drm=ld2, right_drm=rd2)
    _close(_arrays(grown), _arrays(fresh), "increase_rank")
    zeros = (0,) * k
    blk = tsa.blocked_stream_sketch(T, ld2, rd2, [zeros, l0, l1], [zeros, r0, r1])
    _close([np.asarray(a) for a in list(blk.Psi_cores) + list(blk.Omega_mats)], _arrays(fresh), "blocked")
    # and the sparse pass: rank slices of tables and diagonal chains
    X = T.to_numpy()
    rng = np.random.default_rng(3)
    flat = rng.choice(X.size, 3000, replace=False)
    idx = np.array(np.unravel_index(flat, shape))
    sp = tsa.SparseTensor(shape, idx, X[tuple(idx)])
    fresh = tsa.stream_sketch(sp, l1, r1, left_drm=ld2, right_drm=rd2)
    blk = tsa.blocked_stream_sketch(sp, ld2, rd2, [zeros, l0, l1], [zeros, r0, r1])
    _close([np.asarray(a) for a in list(blk.Psi_cores) + list(blk.Omega_mats)], _arrays(fresh), "blocked sparse")
