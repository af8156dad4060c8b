"""Every kernel family behind ttsk_gemm (gemm.hip), at its dispatch edges, element by element.

Each case of CASES (tests/gemm_families_ref.py) names the family it is meant to reach, as a regular expression matched at the
start of the kernel name the launcher's profiling bracket records (csrc/prof.h ProfBracket), and the number of bracketed
launches.  An untagged ttsk_gemm call files under the last profiling class, 11.  Branches the name does not show (the skinny_r
operand variant, swap, rebase, nsub, the variant of the slab sum) are stated in the case's comment, by the field of the plan
(csrc/gemm_plan.h) that holds them, and in its coverage tags; tests/test_gemm_plan.py derives them from the plans on the host,
and test_family_table_covers_every_branch checks the union of the tags.

Every case runs twice, with guard bands around C (guard rows and columns, a gap between batch slices, 64 elements
before and after every buffer; all pre-filled with the sentinel -1/3) and with every operand element outside its view
set to 1e300:

- integer pass: A, B, k_scale and the starting C hold integers in [-4, 4], alpha is a small integer or +-1/2 and every
  partial sum stays far below 2^53, so the fp64 result is exact in any summation order (split-K slabs included).  C
  must EQUAL alpha * einsum(int64) + C0 (signed zeros are not told apart).
- Gaussian pass: standard normal A, B, k_scale and C0.  The reference is computed in np.longdouble and each element
  must satisfy |got - ref| <= C_BOUND (K + 3) 2^-53 (|alpha| (|A| |s| |B|)_ij + |C0_ij|), C_BOUND = 2: any order
  of the K products (fused or not, scaled by k_scale or not) and the alpha / accumulate step is within
  (K + 3) 2^-53 of that sum of magnitudes, up to second-order terms.  The Frobenius relative error is checked second.

Both passes then demand that every guard element still holds the sentinel and that A, B and k_scale read back
bit-identical to what was uploaded.

The mid-batch fall-back of the batched long-K path (gemm.hip, `rs == 0` inside the loop over the slice groups) is reached
by no input: tests/test_gemm_plan.py test_no_slice_group_is_refused_after_the_first checks that over a sweep of descriptors.

The families are reached through shapes and strides alone: the library has no switch that selects among them.
"""
import ctypes
import re

import numpy as np
import pytest

from tests.gemm_families_ref import CASES, POST, PRE, REQUIRED, V, Case, _derived_tags, _family, _sizes
from tests.edge_kit import C_BOUND, LD, PAD, PROF_OTHER, assert_guards, exact, sentinel_buffer, strided, tsa  # noqa: F401

pytestmark = pytest.mark.gpu

# Operand elements outside the view are PAD.  C guards and, with accumulate off, C itself before the call are the sentinel:
# finite and not a multiple of 1/2, so an unwritten element fails the integer pass and a stray accumulating store changes
# it (NaN + x would give the NaN back)
PROF_CLS = PROF_OTHER               # untagged ttsk_gemm calls


# ------------------------------------------------------------------ host side of one case
def _view(buf, v: V):
    return strided(buf, PRE + v.off, v.shape, v.strides)


def _operand(rng, v: V, integer):
    buf = np.full(PRE + v.nelem + POST, PAD)
    vals = rng.integers(-4, 5, size=v.shape).astype(np.float64) if integer else rng.standard_normal(v.shape)
    _view(buf, v)[...] = vals               # (a broadcast view: the last write wins; the reference reads it back)
    return buf


def _run(tsa, c: Case, integer: bool, seed: int):
    import tt_sketch_amd.device as dev
    from tt_sketch_amd import _native as nat
    rng = np.random.default_rng(seed)
    size, K = _sizes(c)
    hA, hB = _operand(rng, c.A, integer), _operand(rng, c.B, integer)
    hC = sentinel_buffer(c.C.nelem, PRE, POST)
    if c.acc:
        _view(hC, c.C)[...] = rng.integers(-4, 5, size=c.C.shape) if integer else rng.standard_normal(c.C.shape)
    ko_ki = (c.A.shape[2], c.A.shape[3]) if c.via == "desc" else None
    hS = None
    if c.ks:
        n = ko_ki[0] * ko_ki[1]
        hS = rng.integers(-4, 5, size=n).astype(np.float64) if integer else rng.standard_normal(n)
    dA, dB, dC = (dev.DevArray.from_host(h) for h in (hA, hB, hC))
    dS = dev.DevArray.from_host(hS) if hS is not None else None

    def dview(d, v):
        return dev.DevArray(d.buf, PRE + v.off, v.shape, v.strides)

    nat.call("ttsk_sync", -1)
    nat.call("ttsk_prof_enable", 1)
    try:
        if c.via == "contract":
            dev.contract(c.spec, dview(dA, c.A), dview(dB, c.B), out=dview(dC, c.C), alpha=c.alpha,
                         accumulate=bool(c.acc), split_k=c.split_k)
        else:
            d = nat.GemmDesc()
            d.batch, d.M, d.Ko, d.Ki = c.A.shape
            d.N = c.B.shape[3]
            d.a_b, d.a_m, d.a_ko, d.a_ki = c.A.strides
            d.b_b, d.b_ko, d.b_ki, d.b_n = c.B.strides
            d.c_b, d.c_m, d.c_n = c.C.strides
            d.alpha, d.accumulate, d.split_k = float(c.alpha), int(c.acc), int(c.split_k)
            P = ctypes.c_void_p
            nat.call("ttsk_gemm", ctypes.byref(d), P(dA.ptr + PRE * 8 + c.A.off * 8), P(dB.ptr + PRE * 8 + c.B.off * 8),
                     P(dC.ptr + PRE * 8 + c.C.off * 8), P(dS.ptr) if dS is not None else None, 0)
        nat.call("ttsk_sync", -1)
        name = ctypes.create_string_buffer(128)
        nat.call("ttsk_prof_kernel_name", PROF_CLS, name, ctypes.c_size_t(len(name)))
        launches = ctypes.c_int64()
        nat.call("ttsk_prof_read", PROF_CLS, ctypes.byref(launches), None, None)
    finally:
        nat.call("ttsk_prof_enable", 0)
    name = name.value.decode()
    gA, gB, gC = dA.get(), dB.get(), dC.get()
    gS = dS.get() if dS is not None else None

    what = f"{c.id} ({'integer' if integer else 'Gaussian'} pass)"
    # 1. the family that ran
    want_l = c.launches if c.launches is not None else (0 if c.fam is None else 1)
    assert launches.value == want_l, f"{what}: {launches.value} bracketed launches, expected {want_l} ({name!r})"
    if c.fam is not None:
        assert re.match(c.fam, name), f"{what}: reached {name!r}, expected {c.fam!r}"
    # 2. inputs untouched, guards untouched
    assert np.array_equal(gA.view(np.uint64), hA.view(np.uint64)), f"{what}: A was written"
    assert np.array_equal(gB.view(np.uint64), hB.view(np.uint64)), f"{what}: B was written"
    if gS is not None:
        assert np.array_equal(gS.view(np.uint64), hS.view(np.uint64)), f"{what}: k_scale was written"
    assert_guards(gC, [(PRE + c.C.off, c.C.shape, c.C.strides)], what + " C")
    # 3. values
    got = _view(gC, c.C).copy()
    C0 = _view(hC, c.C).copy() if c.acc else np.zeros(c.C.shape)
    Av, Bv = _view(hA, c.A), _view(hB, c.B)
    spec = c.spec
    if integer:
        Ai = Av.astype(np.int64)
        if hS is not None:
            Ai = Ai * hS.astype(np.int64).reshape(1, 1, *ko_ki)
        s = np.einsum(spec, Ai, Bv.astype(np.int64)) if got.size else np.zeros(c.C.shape, np.int64)
        assert np.abs(s).max(initial=0) < 2 ** 50
        ref = c.alpha * s.astype(np.float64) + C0
        exact(got, ref, what)
        return
    Al = Av.astype(LD)
    Aa = np.abs(Al)
    if hS is not None:
        sl = hS.astype(LD).reshape(1, 1, *ko_ki)
        Al, Aa = Al * sl, Aa * np.abs(sl)
    Bl = Bv.astype(LD)
    if got.size:
        ref = LD(c.alpha) * np.einsum(spec, Al, Bl) + C0.astype(LD)
        mag = abs(c.alpha) * np.einsum(spec, Aa, np.abs(Bl)) + np.abs(C0).astype(LD)
    else:
        ref = mag = np.zeros(c.C.shape, LD)
    tol = C_BOUND * (K + 3) * LD(2.0) ** -53 * mag
    err = np.abs(got.astype(LD) - ref)
    over = ~(err <= tol)
    if over.any():
        i = tuple(np.argwhere(over)[0])
        pytest.fail(f"{what}: {int(over.sum())} of {got.size} elements outside the bound, first at {i}: got {got[i]!r}, "
                    f"ref {float(ref[i])!r}, |err| {float(err[i]):.3e} > {float(tol[i]):.3e}")
    rn = float(np.linalg.norm(ref.astype(np.float64)))
    if rn > 0:
        assert float(np.linalg.norm((got - ref.astype(np.float64)))) <= 1e-13 * rn, what


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_gemm_family_case(tsa, case):
    seed = sum(map(ord, case.id))
    _run(tsa, case, True, seed)
    _run(tsa, case, False, seed + 1)


def test_family_table_covers_every_branch():
    """The table as a whole reaches every family and variant of the dispatch list, each family with odd and even
    extents and with alpha != 1 plus accumulate; ids are unique."""
    assert len({c.id for c in CASES}) == len(CASES)
    tags = set()
    for c in CASES:
        tags |= set(c.tags) | _derived_tags(c)
    missing = {fam: [t for t in ts if t not in tags] for fam, ts in REQUIRED.items()}
    missing = {k: v for k, v in missing.items() if v}
    assert not missing, f"branches no case reaches: {missing}"
    fams = {}
    for c in CASES:
        if c.fam is None:
            continue
        size, K = _sizes(c)
        ext = [n for n in size.values() if n > 1]
        f = fams.setdefault(_family(c), {"odd": False, "even": False, "alpha_acc": False})
        f["odd"] |= any(n % 2 for n in ext)
        f["even"] |= any(n % 2 == 0 for n in ext)
        f["alpha_acc"] |= c.alpha != 1.0 and bool(c.acc)
    want = {"rows_longk", "skinny_r", "skinny_s", "small_gemm", "batched long-K", "gemm_f64"}
    assert want <= set(fams), f"families without a case: {sorted(want - set(fams))}"
    lacking = {k: [p for p, ok in v.items() if not ok] for k, v in fams.items()}
    lacking = {k: v for k, v in lacking.items() if v}
    assert not lacking, f"families lacking a kind of case: {lacking}"
