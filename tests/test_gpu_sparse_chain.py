"""The chain factor of the one-pass sparse kernel (kind 4 of ttsk_sg_factor: csrc/sparse_pass.h stage 2b', planned by
csrc/sparse_plan.h) at the C ABI, ttsk_sparse_gauss_pass_u32 called directly with hand-made streams, as
tests/test_gpu_sparse_pass.py does for the other kinds.

Exact: cores, tables and sign rows with entries in {-1, 0, 1}, values in [-3, 3].  A chain row is at most 32^3 in size
(three steps of rank 32), a term at most 3 * 2^15 * 32 and there are at most 2^17 of them: every partial sum in any order is an
exact double and the device must give the int64 reference (tests/sparse_chain_ref.py) bit for bit.  Every table carries its
spare row filled with 2^40, Psi and Omega sit between guard bands."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

from tests import sparse_cases as sc
from tests import sparse_chain_ref as ref
from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

SPARE = float(2 ** 40)
GUARD, GUARD_FILL = 64, 7.0
STRUCTURES = {s.name: s for s in sc.structures()}
P_OTHER = 13                      # distinct flat indices of a stream no chain factor reads

# rows: of the start table (0: from the first core, r0 = 1); steps: (mode size, rank behind it) of every core -- a mode size
# None is the number of slices (a C factor's last digit is the record's mode index); [lo, lo + w) of the last rank
Chain = namedtuple("Chain", "rows r0 steps lo w")
Tab = namedtuple("Tab", "w")
Nrm = namedtuple("Nrm", "w lo")
Sgn = namedtuple("Sgn", "w lo full nnz")
Cfg = namedtuple("Cfg", "name A B C c_left", defaults=(None, 0))


def chain(rows, r0, *steps, lo=0, w=None):
    return Chain(rows, r0, steps, lo, steps[-1][1] - lo if w is None and steps else (r0 - lo if w is None else w))


def _packed(a, dtype):
    from tt_sketch_amd.device import DevArray
    a = np.asarray(a, dtype=dtype)
    if a.size & 1:
        a = np.concatenate([a, np.zeros(1, dtype=dtype)])
    return DevArray.from_host(a.view(np.int64))


def _guarded(shape):
    """(the whole buffer, the zeroed view inside its guard bands)"""
    from tt_sketch_amd.device import DevArray
    size = int(np.prod(shape))
    host = np.full(size + 2 * GUARD, GUARD_FILL)
    host[GUARD:GUARD + size] = 0.0
    buf = DevArray.from_host(host)
    return buf, buf[GUARD:GUARD + size].reshape(*shape)


def _extent(F, n):
    """distinct flat indices of the stream a chain factor reads (its last digit is j where it is C)"""
    ns = [n if m is None else m for m, _ in F.steps]
    if any(m is None for m, _ in F.steps):
        ns = ns[:-1]
    return max(F.rows, 1) * int(np.prod(ns, dtype=object))


class Case:
    def __init__(self, cfg, st, seed):
        from tt_sketch_amd.device import DevArray
        from tt_sketch_amd.drm.fast_lazy_gaussian import inds_to_normal, inds_to_sparse_sign
        from tt_sketch_amd.sparse_fused import _Chain, _Factor
        rng = np.random.default_rng(seed)
        self.cfg, self.st = cfg, st
        j, n = st.j.astype(np.int64), st.n
        N = self.N = j.size
        # extents of the two streams: what the chain factors on them need (C reads the stream of its side)
        ext = [None, None]
        for F, side in ((cfg.A, 0), (cfg.B, 1), (cfg.C, 0 if cfg.c_left else 1)):
            if isinstance(F, Chain):
                e = _extent(F, n)
                assert ext[side] in (None, e), "two chain factors on one stream disagree about its extent"
                ext[side] = e
        Pl, Pr = (e if e is not None else P_OTHER for e in ext)
        assert Pl < 2 ** 31 and Pr < 2 ** 31
        fl, fr = rng.integers(0, Pl, N), rng.integers(0, Pr, N)
        fl[0] = fl[-1] = Pl - 1                       # the largest flat index: first and last record
        fr[0] = fr[-1] = Pr - 1
        self.fl, self.fr = fl, fr
        self.v = rng.integers(-3, 4, N).astype(np.int64)
        self.keep, self.factors, self.rows, self.exact = [], [], [], True
        for i, F in enumerate((cfg.A, cfg.B, cfg.C)):
            if F is None:
                self.factors.append(None)
                self.rows.append(np.ones((N, 1), dtype=np.int64))
                continue
            src = i if i < 2 else (2 if cfg.c_left else 3)
            base, P = (fr, Pr) if src & 1 else (fl, Pl)
            mul = P if src & 2 else 0
            flat, nrows = base + j * mul, P * n if src & 2 else P
            fseed = 0x5EED0 + 17 * i + seed
            if isinstance(F, Chain):
                rk = [F.r0] + [r for _, r in F.steps]
                ns = [n if m is None else m for m, _ in F.steps]
                cores = [rng.integers(-1, 2, (rk[s], ns[s], rk[s + 1])) for s in range(len(ns))]
                tab = rng.integers(-1, 2, (F.rows, F.r0)) if F.rows else None
                ch = _Chain()
                ch.steps, ch.rows, ch.rank[0] = len(ns), F.rows, F.r0
                for s, D in enumerate(cores):
                    dev = DevArray.from_host(D.astype(np.float64))
                    self.keep.append(dev)
                    ch.core[s], ch.n[s], ch.rank[s + 1] = dev.ptr, ns[s], rk[s + 1]
                dtab = None
                if tab is not None:
                    dtab = DevArray.from_host(np.vstack([tab, np.full((1, F.r0), SPARE)]).astype(np.float64))
                    self.keep.append(dtab)
                self.keep.append(ch)
                self.factors.append(_Factor(4, F.w, F.lo, src, 0, 0, dtab.ptr if dtab is not None else None, 0, 0, ctypes.pointer(ch)))
                self.rows.append(ref.chain_rows(base, tab, F.rows, cores, F.lo, F.w, j if src & 2 else None))
            elif isinstance(F, Tab):
                t = rng.integers(-1, 2, (nrows, F.w))
                dev = DevArray.from_host(np.vstack([t, np.full((1, F.w), SPARE)]).astype(np.float64))
                self.keep.append(dev)
                self.factors.append(_Factor(1, F.w, 0, src, mul, fseed, dev.ptr, 0, 0))
                self.rows.append(t[flat])
            elif isinstance(F, Sgn):
                self.factors.append(_Factor(3, F.w, F.lo, src, mul, fseed, None, F.full, F.nnz))
                self.rows.append(inds_to_sparse_sign(flat[None, :], (nrows,), F.full, F.lo, F.lo + F.w, F.nnz, fseed).astype(np.int64))
            else:
                self.exact = False
                self.factors.append(_Factor(2, F.w, F.lo, src, mul, fseed, None, 0, 0))
                self.rows.append(inds_to_normal(flat[None, :], (nrows,), F.lo, F.lo + F.w, fseed))
        self.dev_j = _packed(st.j, np.int32)
        self.dev_v = DevArray.from_host(self.v.astype(np.float64))
        self.dev_fl, self.dev_fr = _packed(fl, np.uint32), _packed(fr, np.uint32)

    def reference(self):
        A, B, C = self.rows
        v = self.v[:, None]
        psi = sc.segmented_outer(self.st.j, self.st.n, v * A, B)
        om = None
        if self.cfg.C is not None:
            om = (v * C).T @ B if self.cfg.c_left else (v * A).T @ C
        return psi, om

    def run(self, entry="ttsk_sparse_gauss_pass_u32"):
        from tt_sketch_amd import _native as nat
        wA, wB, wC = (r.shape[1] for r in self.rows)
        pbuf, psi = _guarded((wA, self.st.n, wB))
        obuf = om = None
        if self.cfg.C is not None:
            obuf, om = _guarded((wC, wB) if self.cfg.c_left else (wA, wC))
        byref = lambda f: None if f is None else ctypes.byref(f)
        A, B, C = self.factors
        nat.call(entry, self.dev_fl, self.dev_fr, self.dev_j, self.dev_v, self.N, self.st.n, byref(A), byref(B), byref(C),
                 self.cfg.c_left, psi, om, 0)
        out = []
        for buf, view in ((pbuf, psi), (obuf, om)):
            if buf is None:
                out.append(None)
                continue
            whole = buf.get()
            assert np.all(whole[:GUARD] == GUARD_FILL) and np.all(whole[-GUARD:] == GUARD_FILL), "a guard band was written"
            out.append(whole[GUARD:-GUARD].reshape(view.shape))
        return out


def _check(case, what):
    psi_ref, om_ref = case.reference()
    psi, om = case.run()
    psi2, om2 = case.run()
    assert np.abs(psi).max() < SPARE / 2 and (om is None or np.abs(om).max() < SPARE / 2), (what, "a spare table row reached a stored cell")
    bad = np.argwhere(psi != psi_ref)
    assert np.array_equal(psi, psi_ref), (what, "Psi", len(bad), bad[:4].tolist(), [float(psi[tuple(b)]) for b in bad[:4]],
                                          [float(psi_ref[tuple(b)]) for b in bad[:4]])
    if om_ref is not None:
        assert case.exact
        bad = np.argwhere(om != om_ref)
        assert np.array_equal(om, om_ref), (what, "Omega", len(bad), bad[:4].tolist())
    assert psi.tobytes() == psi2.tobytes() and (om is None or om.tobytes() == om2.tobytes()), (what, "a second call gives other bits")


def _runs(N, n=1):
    return sc._st(f"N{N}-n{n}", np.sort(np.arange(N) % n), n)


# ------------------------------------------------------------------ the shapes of a chain, as A beside two tables
SHAPES = [
    Cfg("table-0-steps", chain(17, 6, lo=1, w=4), Tab(5), Tab(7)),
    Cfg("table-1-step", chain(17, 3, (5, 9)), Tab(5), Tab(7)),
    Cfg("table-2-steps-3-17-5", chain(6, 3, (4, 17), (5, 5)), Tab(5), Tab(7)),
    Cfg("table-3-steps", chain(5, 2, (3, 4), (2, 6), (7, 3)), Tab(5), Tab(7)),
    Cfg("first-core-only", chain(0, 1, (19, 6)), Tab(5), Tab(7)),
    Cfg("first-core-2-steps", chain(0, 1, (6, 4), (5, 9)), Tab(5), Tab(7)),
    Cfg("first-core-3-steps", chain(0, 1, (3, 2), (5, 7), (4, 3)), Tab(5), Tab(7)),
    Cfg("first-core-4-steps", chain(0, 1, (3, 2), (5, 7), (4, 3), (2, 5)), Tab(5), Tab(7)),
    Cfg("ranks-1-1", chain(9, 1, (4, 1)), Tab(5), Tab(7)),
    Cfg("ranks-32-32", chain(9, 32, (4, 32)), Tab(5), Tab(7)),
    Cfg("ranks-16-17", chain(9, 16, (4, 17)), Tab(5), Tab(7)),
    Cfg("rank-slice-5-13-of-16", chain(9, 4, (4, 16), lo=5, w=8), Tab(5), Tab(7)),
    Cfg("mode-of-extent-1", chain(7, 3, (1, 4), (5, 6)), Tab(5), Tab(7)),
    Cfg("mode-of-extent-1-last", chain(0, 1, (7, 4), (1, 6)), Tab(5), Tab(7)),
    Cfg("prefix-below-2^31", chain(0, 1, (46340, 2), (46340, 3)), Tab(5), Tab(7)),
    Cfg("prefix-2^31-1-table", chain(32768, 2, (32767, 3), (2, 4)), Tab(5), Tab(7)),
]
SHAPE_STRUCTURES = [STRUCTURES["one"], STRUCTURES["runs57"], _runs(2049, 3)]


@pytest.mark.parametrize("cfg", SHAPES, ids=lambda c: c.name)
def test_chain_shapes_exact(tsa, cfg):
    """every length of chain after a table and from the first core, the rank combinations on either side of 16, a rank
    slice, a mode of extent 1, flat indices up to 2^31 - 2: with an Omega riding on the right (c_left = 0, C a table)"""
    for k, st in enumerate(SHAPE_STRUCTURES):
        big = _extent(cfg.A, st.n) > 10 ** 6
        c = cfg._replace(C=None) if big or st.n > 64 else cfg       # (a C table has extent * n rows)
        _check(Case(c, st, 7000 + k), (cfg.name, st.name))


# ------------------------------------------------------------------ the positions of a chain and what stands beside it
CH_A = chain(6, 3, (4, 9), (5, 5))
CH_B = chain(5, 4, (3, 7), (4, 6))
POSITIONS = [
    Cfg("chain-A", CH_A, Tab(6), None),
    Cfg("chain-B", Tab(6), CH_B, None),
    Cfg("chain-A-and-B", CH_A, CH_B, None),
    Cfg("chain-first-mode", None, CH_B, None),
    Cfg("chain-last-mode", CH_A, None, None),
    Cfg("chain-C-src2", chain(6, 3, (4, 9), lo=0, w=9), Tab(6), chain(6, 3, (4, 9), (None, 5)), 1),
    Cfg("chain-C-src3", Tab(6), chain(5, 4, (3, 7)), chain(5, 4, (3, 7), (None, 6)), 0),
    Cfg("chain-C-src2-first-core", None, Tab(6), chain(0, 1, (None, 5)), 1),
    Cfg("chain-C-src3-table-0-steps-before-j", Tab(4), Tab(6), chain(P_OTHER, 4, (None, 6)), 0),
    Cfg("all-three-chains", chain(6, 3, (4, 9)), CH_B, chain(6, 3, (4, 9), (None, 5)), 1),
    Cfg("chain-beside-sign", CH_A, Sgn(8, 5, 24, 3), Tab(4), 0),
    Cfg("chain-beside-sign-C", CH_A, Tab(5), Sgn(6, 2, 12, 2), 0),
]


@pytest.mark.parametrize("cfg", POSITIONS, ids=lambda c: c.name)
def test_chain_positions_exact_on_every_slice_structure(tsa, cfg):
    """a chain as A, as B, as C with src 2 and with src 3, beside tables and sign rows, over the whole catalogue of slice
    structures (a C table addressed by prefix + j * mul has P n rows: only n <= 64 there)"""
    wide = isinstance(cfg.C, Tab)
    for k, st in enumerate(STRUCTURES.values()):
        if st.null_j or (wide and st.n > 64):
            continue
        _check(Case(cfg, st, 9000 + k), (cfg.name, st.name))


@pytest.mark.parametrize("N", [1, 31, 32, 33, 2049])
def test_chain_stream_lengths(tsa, N):
    for n in (1, 3):
        if n > N:
            continue
        _check(Case(POSITIONS[5], _runs(N, n), 100 + N), ("chain-C-src2", N, n))
        _check(Case(POSITIONS[2], _runs(N, n), 200 + N), ("chain-A-and-B", N, n))


def test_chain_over_more_than_256_waves(tsa):
    st = sc._st("long", np.concatenate([np.zeros(30000), np.ones(1), np.full(35999, 2)]), 3)
    _check(Case(POSITIONS[9], st, 31), ("all-three-chains", st.name))


def test_chain_beside_normals_sampled_in_the_pass(tsa):
    """one record per slice: Psi[a, j, c] = (v A)[j, a] B[j, c] is one product of an integer and a sampled normal, one
    rounding, whatever the order -- equal to the host's product bit for bit"""
    st = STRUCTURES["arange"]
    for cfg in (Cfg("chain-A-normal-B", CH_A, Nrm(13, 3), None), Cfg("normal-A-chain-B", Nrm(20, 0), CH_B, None)):
        case = Case(cfg, st, 77)
        A, B, _ = case.rows
        want = np.zeros((A.shape[1], st.n, B.shape[1]))
        want[:, st.j, :] = ((case.v[:, None] * A)[:, :, None] * B[:, None, :]).transpose(1, 0, 2)
        psi, _ = case.run()
        assert np.array_equal(psi, want), cfg.name
        assert psi.tobytes() == case.run()[0].tobytes()


def test_wide_chain_takes_the_16_record_tile(tsa):
    """three factors of 32 columns, the chain among them: sg_plan falls back to T = 16 (tests/test_sparse_chain_plan.py
    holds the plan to that)"""
    cfg = Cfg("wide", chain(6, 32, (4, 32)), Tab(32), Tab(32), 0)
    for st in (STRUCTURES["runs57"], STRUCTURES["skewed"], _runs(33)):
        _check(Case(cfg, st, 55), (cfg.name, st.name))
    cfg = Cfg("wide-C", Tab(32), Tab(32), chain(P_OTHER, 32, (None, 32)), 0)
    _check(Case(cfg, STRUCTURES["runs57"], 56), cfg.name)


def test_chain_refusals_leave_psi_as_it_was(tsa):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    from tt_sketch_amd.sparse_fused import _Chain, _Factor
    N, n = 40, 3
    rng = np.random.default_rng(5)
    fl32, fr32 = (_packed(rng.integers(0, 5, N), np.uint32) for _ in range(2))
    fl64, fr64 = (DevArray.from_host(rng.integers(0, 5, N).astype(np.uint64)) for _ in range(2))
    jj = _packed(np.sort(rng.integers(0, n, N)), np.int32)
    val = DevArray.from_host(np.ones(N))
    core = DevArray.from_host(np.ones((40, 5, 40)))
    tab = DevArray.from_host(np.ones((6, 40)))
    fill = np.full((32, n, 32), 7.0)
    keep = []

    def chain_factor(ranks, steps=1, rows=0, table=False, lo=0, w=2, n_mode=5):
        ch = _Chain()
        ch.steps, ch.rows = steps, rows
        for s in range(min(steps, len(ch.core))):
            ch.core[s], ch.n[s] = core.ptr, n_mode
        for s, r in enumerate(ranks):
            ch.rank[s] = r
        keep.append(ch)
        return _Factor(4, w, lo, 0, 0, 0, tab.ptr if table else None, 0, 0, ctypes.pointer(ch))

    no_desc = _Factor(4, 2, 0, 0, 0, 0, None, 0, 0)
    no_core = chain_factor((1, 2))
    no_core.chain.contents.core[0] = None
    u32 = "ttsk_sparse_gauss_pass_u32"
    refused = {
        "rank 33": (u32, chain_factor((1, 33), w=2), nat.TtskUnsupported),
        "inner rank 33": (u32, chain_factor((1, 33, 2), steps=2), nat.TtskUnsupported),
        "zero cores": (u32, chain_factor((1,), steps=0), ValueError),
        "nine steps": (u32, chain_factor((1,) * 9, steps=9), nat.TtskUnsupported),
        "no descriptor": (u32, no_desc, ValueError),
        "NULL core": (u32, no_core, ValueError),
        "first core behind rank 2": (u32, chain_factor((2, 2)), ValueError),
        "rows without a table": (u32, chain_factor((2, 2), rows=5), ValueError),
        "table without rows": (u32, chain_factor((1, 2), table=True), ValueError),
        "columns beyond the last rank": (u32, chain_factor((1, 4), lo=3, w=2), ValueError),
        "mode of size 0": (u32, chain_factor((1, 2), n_mode=0), ValueError),
        "64-bit streams": ("ttsk_sparse_gauss_pass", chain_factor((1, 2)), nat.TtskUnsupported),
    }
    for what, (entry, A, exc) in refused.items():
        fl, fr = (fl32, fr32) if entry == u32 else (fl64, fr64)
        psi = DevArray.from_host(fill)
        with pytest.raises(exc):
            nat.call(entry, fl, fr, jj, val, N, n, ctypes.byref(A), None, None, 0, psi, None, 0)
        assert np.array_equal(psi.get(), fill), what
