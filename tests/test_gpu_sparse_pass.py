"""The one-pass sparse kernel (csrc/sparse_pass.h, launched by csrc/sparse_fused.hip) at the C ABI, ttsk_sparse_gauss_pass and
ttsk_sparse_gauss_pass_u32 called directly with hand-made streams, so that the slice structure, the factor widths and therefore the kernel
instantiation of every case are chosen and not what a random tensor happens to give (tests/sparse_cases.py holds the
catalogues; test_host_logic.test_sparse_pass_configurations_reach_every_instantiation and tests/test_sparse_plan.py hold the
list against the launcher's plan, csrc/sparse_plan.h).

Reference: explicit row matrices A[e, :], B[e, :], C[e, :] (a table gathered at the factor's flat index, ones, or the host
sampler on that flat index) and
    Psi[a, j, c] = sum_{e: j_e = j} v_e A[e, a] B[e, c],
    Omega        = sum_e v_e C[e, a] B[e, c]  (c_left)   or   sum_e v_e A[e, a] C[e, c].

Exact family (tables and sign rows): entries in [-3, 3], table entries in [-4, 4], signs in {-1, 0, 1}: a term is at most 48
and there are at most 2^17 of them, so every partial sum in any order is an exact double and the device must give the int64
reference bit for bit.  Every table carries its spare row, filled with 2^40: should it reach a stored cell the cell is off
by at least 2^40.

Sampled family (normals made in the pass): against a longdouble reference, per element
    |got - ref| <= (n_j + 8) 2^-53 sum_e |v_e A B|
with n_j the terms of that element (one rounding for v A, one per addition, 8 for the additions of the partial blocks)."""
import ctypes

import numpy as np
import pytest

from tests import sparse_cases as sc
from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

SPARE = float(2 ** 40)
STRUCTURES = sc.structures()
P_LEFT, P_RIGHT = 11, 13          # distinct prefixes / suffixes of the hand-made streams


def _packed(a, dtype):
    """a 32-bit array as the int64 words DevArray carries (padded to an even count)"""
    from tt_sketch_amd.device import DevArray
    a = np.asarray(a, dtype=dtype)
    if a.size & 1:
        a = np.concatenate([a, np.zeros(1, dtype=dtype)])
    return DevArray.from_host(a.view(np.int64))


class Case:
    """One stream and the three row matrices of a configuration on it."""

    def __init__(self, cfg, st, seed):
        from tt_sketch_amd.device import DevArray
        from tt_sketch_amd.drm.fast_lazy_gaussian import inds_to_normal, inds_to_sparse_sign
        from tt_sketch_amd.sparse_fused import _Factor
        rng = np.random.default_rng(seed)
        self.cfg, self.st = cfg, st
        j, n = st.j.astype(np.int64), st.n
        N = self.N = j.size
        uses = lambda side: any(F is not None and (F.src & 1) == side for F in (cfg.A, cfg.B, cfg.C))
        # an absent A (B) is the first (last) mode: no prefix (suffix) stream, unless the Omega factor extends it by the
        # mode index -- then the one empty prefix, flat index 0
        Pl = P_LEFT if cfg.A is not None else 1
        Pr = P_RIGHT if cfg.B is not None else 1
        fl = rng.integers(0, Pl, N) if uses(0) else None
        fr = rng.integers(0, Pr, N) if uses(1) else None
        for f, P in ((fl, Pl), (fr, Pr)):
            if f is not None:                  # the last real row of every table: first and last record (the last has the largest j)
                f[0] = f[-1] = P - 1
        self.fl, self.fr = fl, fr
        self.v = rng.integers(-3, 4, N).astype(np.int64) if cfg.exact else rng.standard_normal(N)
        self.keep, self.factors, self.rows = [], [], []
        for i, F in enumerate((cfg.A, cfg.B, cfg.C)):
            if F is None:
                self.factors.append(None)
                self.rows.append(np.ones((N, 1), dtype=np.int64))
                continue
            base, P = (fr, Pr) if F.src & 1 else (fl, Pl)
            mul = P if F.src & 2 else 0
            flat = base + j * mul
            nrows = P * n if F.src & 2 else P
            fseed = 0x5EED0 + 17 * i + seed
            tab = None
            if F.kind == 1:
                t = rng.integers(-4, 5, (nrows, F.w)) if cfg.exact else rng.standard_normal((nrows, F.w))
                tab = DevArray.from_host(np.vstack([t, np.full((1, F.w), SPARE)]).astype(np.float64))
                self.keep.append(tab)
                rows = t[flat]
            elif F.kind == 2:
                rows = inds_to_normal(flat[None, :], (nrows,), F.lo, F.lo + F.w, fseed)
            else:
                rows = inds_to_sparse_sign(flat[None, :], (nrows,), F.full, F.lo, F.lo + F.w, F.nnz, fseed).astype(np.int64)
            self.factors.append(_Factor(F.kind, F.w, F.lo, F.src, mul, fseed, tab.ptr if tab is not None else None, F.full, F.nnz))
            self.rows.append(rows)
        self.dev_j = None if st.null_j else _packed(st.j, np.int32)
        self.dev_v = DevArray.from_host(self.v.astype(np.float64))

    def shapes(self):
        wA, wB, wC = (r.shape[1] for r in self.rows)
        om = None if self.cfg.C is None else ((wC, wB) if self.cfg.c_left else (wA, wC))
        return (wA, self.st.n, wB), om

    def reference(self, dtype):
        """(Psi, Omega, sum |terms| of Psi, of Omega, terms per element of Psi) in ``dtype``"""
        A, B, C = (r.astype(dtype) for r in self.rows)
        v = self.v.astype(dtype)[:, None]
        j, n = self.st.j, self.st.n
        psi = sc.segmented_outer(j, n, v * A, B)
        if self.cfg.exact:
            mag = None
        else:
            mag = sc.segmented_outer(j, n, np.abs(v * A), np.abs(B))
        om = om_mag = None
        if self.cfg.C is not None:
            L, R = (v * C, B) if self.cfg.c_left else (v * A, C)
            om = L.T @ R
            om_mag = None if self.cfg.exact else np.abs(L).T @ np.abs(R)
        return psi, om, mag, om_mag, np.bincount(j, minlength=n)

    def run(self, w32):
        """(Psi, Omega) of the 64-bit or the 32-bit entry point on zeroed outputs"""
        from tt_sketch_amd import _native as nat
        from tt_sketch_amd.device import DevArray
        if w32:
            fl = None if self.fl is None else _packed(self.fl, np.uint32)
            fr = None if self.fr is None else _packed(self.fr, np.uint32)
        else:
            fl = None if self.fl is None else DevArray.from_host(self.fl.astype(np.uint64))
            fr = None if self.fr is None else DevArray.from_host(self.fr.astype(np.uint64))
        ps, os_ = self.shapes()
        psi = DevArray.zeros(ps)
        om = None if os_ is None else DevArray.zeros(os_)
        ref = lambda f: None if f is None else ctypes.byref(f)
        A, B, C = self.factors
        nat.call("ttsk_sparse_gauss_pass_u32" if w32 else "ttsk_sparse_gauss_pass", fl, fr, self.dev_j, self.dev_v, self.N, self.st.n,
                 ref(A), ref(B), ref(C), self.cfg.c_left, psi, om, 0)
        return psi.get(), None if om is None else om.get()


def _structures_for(cfg):
    """every structure; a C table addressed by prefix + j * mul has P n rows, so only n <= 64 there"""
    wide_table = cfg.C is not None and cfg.C.kind == 1
    return [(k, st) for k, st in enumerate(STRUCTURES) if not wide_table or st.n <= 64]


def _same_bits(a, b):
    return a is b or (a.shape == b.shape and a.tobytes() == b.tobytes())


def _check_exact(case, what):
    psi_ref, om_ref, _, _, count = case.reference(np.int64)
    psi, om = case.run(False)
    psi32, om32 = case.run(True)
    assert np.abs(psi).max() < SPARE / 2 and (om is None or np.abs(om).max() < SPARE / 2), (what, "the spare table row reached a stored cell")
    assert not psi[:, count == 0, :].any(), (what, "a slice without a record is not zero")
    bad = np.argwhere(psi != psi_ref)
    assert np.array_equal(psi, psi_ref), (what, "Psi", len(bad), bad[:4].tolist(), [float(psi[tuple(b)]) for b in bad[:4]],
                                          [int(psi_ref[tuple(b)]) for b in bad[:4]])
    if om_ref is not None:
        bad = np.argwhere(om != om_ref)
        assert np.array_equal(om, om_ref), (what, "Omega", len(bad), bad[:4].tolist())
    assert _same_bits(psi, psi32) and _same_bits(om, om32), (what, "the 32-bit and the 64-bit entry point differ")


_EXACT = sc.TABLE_CONFIGS + sc.SIGN_CONFIGS


@pytest.mark.parametrize("ci", range(len(_EXACT)), ids=[c.name for c in _EXACT])
def test_pass_exact_on_every_slice_structure(tsa, ci):
    """Tables and sign rows with integer data over the whole catalogue of slice structures: equal to the int64 reference,
    empty slices zero, no trace of the spare row, both record widths the same bits."""
    cfg = _EXACT[ci]
    for k, st in _structures_for(cfg):
        _check_exact(Case(cfg, st, 1000 * ci + k), (cfg.name, st.name, sc.instantiation(cfg)))


@pytest.mark.parametrize("ci", range(len(sc.LONG_CONFIGS)), ids=[c.name for c in sc.LONG_CONFIGS])
def test_pass_exact_over_more_than_256_waves(tsa, ci):
    """N = 66 000 records in three slices, 258 waves: slices 0 and 2 span more than a hundred waves each (their partial
    blocks found by sg_psi_reduce_kernel's bisection), slice 1 is one record, and sg_om_reduce_kernel's loop over the waves
    takes a second trip."""
    cfg = sc.LONG_CONFIGS[ci]
    st = sc._st("long", np.concatenate([np.zeros(30000), np.ones(1), np.full(35999, 2)]), 3)
    _check_exact(Case(cfg, st, 900000 + ci), (cfg.name, st.name))


@pytest.mark.parametrize("ci", range(len(sc.SAMPLED_CONFIGS)), ids=[c.name for c in sc.SAMPLED_CONFIGS])
def test_pass_sampled_within_the_summation_bound(tsa, ci):
    """Normals sampled in the pass (rows from inds_to_normal on the same flat indices, which test_gpu_ndtri_edges pins to the
    pass bit for bit), real entries: every element within (n_j + 8) 2^-53 sum |terms| of the longdouble reference."""
    if np.finfo(np.longdouble).eps >= 2.0 ** -60:
        pytest.skip("np.longdouble is no wider than 60 bits of mantissa here: no reference to measure a 2^-53 bound against")
    cfg = sc.SAMPLED_CONFIGS[ci]
    u = np.longdouble(2.0) ** -53
    worst = 0.0
    for k, st in _structures_for(cfg):
        case = Case(cfg, st, 500000 + 1000 * ci + k)
        what = (cfg.name, st.name, sc.instantiation(cfg))
        psi_ref, om_ref, mag, om_mag, count = case.reference(np.longdouble)
        psi, om = case.run(False)
        psi32, om32 = case.run(True)
        pairs = [("Psi", psi, psi_ref, (count[None, :, None] + 8) * u * mag)]
        if om_ref is not None:
            pairs.append(("Omega", om, om_ref, (case.N + 8) * u * om_mag))
        for name, got, ref, bound in pairs:
            err = np.abs(got.astype(np.longdouble) - ref)
            ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)))
            worst = max(worst, ratio)
            print(f"[sparse pass] {cfg.name} {st.name} {name}: worst error / bound {ratio:.3f}")
            assert np.all(np.isfinite(got)) and np.all(err <= bound), (what, name, ratio)
        assert not psi[:, count == 0, :].any(), (what, "a slice without a record is not zero")
        assert _same_bits(psi, psi32) and _same_bits(om, om32), (what, "the 32-bit and the 64-bit entry point differ")
    print(f"[sparse pass] {cfg.name}: worst error / bound over all structures {worst:.3f}")


def test_pass_refuses_bad_arguments_before_any_launch(tsa):
    """Every refusal is a ValueError and leaves Psi as it was; N = 0 is accepted and leaves it as it was too."""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    from tt_sketch_amd.sparse_fused import _Factor
    N, n = 40, 3
    rng = np.random.default_rng(31)
    fl64, fr64 = (DevArray.from_host(rng.integers(0, 5, N).astype(np.uint64)) for _ in range(2))
    fl32, fr32 = (_packed(rng.integers(0, 5, N), np.uint32) for _ in range(2))
    jj = _packed(np.sort(rng.integers(0, n, N)), np.int32)
    val = DevArray.from_host(np.ones(N))
    tabs = {w: DevArray.from_host(np.ones((6, w))) for w in (4, 33)}            # five rows and the spare one
    om = DevArray.zeros((32, 32))
    fill = np.full((32, n, 32), 7.0)
    table = lambda w, src, with_table=True: _Factor(1, w, 0, src, 0, 1, tabs[w].ptr if with_table else None, 0, 0)
    sign = lambda w, lo, full, nnz: _Factor(3, w, lo, 1, 0, 1, None, full, nnz)
    ok = table(4, 0)
    # (A, B, C, Omega, fr given, j given, slices)
    refused = {
        "width 33": (table(33, 0), None, None, None, True, True, n),
        "table factor without a table": (table(4, 0, False), None, None, None, True, True, n),
        "sign row of 33": (ok, sign(8, 0, 33, 2), None, None, True, True, n),
        "rank_min + w > full": (ok, sign(8, 5, 12, 2), None, None, True, True, n),
        "C without an Omega": (ok, table(4, 1), table(4, 2), None, True, True, n),
        "suffix factor without a suffix stream": (ok, table(4, 1), None, None, False, True, n),
        "no mode index but several slices": (ok, table(4, 1), None, None, True, False, n),
    }
    ref = lambda f: None if f is None else ctypes.byref(f)
    for name, w32, fl, fr in (("ttsk_sparse_gauss_pass", False, fl64, fr64), ("ttsk_sparse_gauss_pass_u32", True, fl32, fr32)):
        for what, (A, B, C, omega, with_fr, with_j, slices) in refused.items():
            psi = DevArray.from_host(fill)
            with pytest.raises(ValueError):
                nat.call(name, fl, fr if with_fr else None, jj if with_j else None, val, N, slices, ref(A), ref(B), ref(C), 0, psi, omega, 0)
            assert np.array_equal(psi.get(), fill), (name, what)
        psi = DevArray.from_host(fill)
        nat.call(name, fl, fr, jj, val, 0, n, ref(ok), ref(table(4, 1)), ref(table(4, 2)), 1, psi, om, 0)      # N = 0
        assert np.array_equal(psi.get(), fill) and not om.get().any(), name
