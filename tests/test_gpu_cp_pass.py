"""The one-pass CP sketch kernels on the device: ``ttsk_cp_chain_step`` / ``ttsk_cp_psi_omega`` (csrc/cp_pass.hip) called
directly at every edge of tests/cp_pass_ref.py, and the Python surface built on them (``TensorTrainDRM.sketch_cp``,
``sketch_psi_cp`` / ``sketch_omega_cp``, ``cp_fused.try_cp_sketch``) with the kernels forced and with the compositions
forced, against each other, the oracle and the recorded runs of the reference.

Bars (tests/cp_pass_ref.py): entry by entry |out - ref| <= 2 (rho n + 2) 2^-53 out_abs for the chain step,
2 (N + 3) 2^-53 psi_abs for Psi, 2 (N + 2) 2^-53 omega_abs for Omega; two calls give the same bits; cells outside the
outputs keep their NaN.  Public API: 1e-11 for a sketch, 1e-9 for assembled (orthogonalised) cores.
"""
import ctypes
import os

import numpy as np
import pytest

from tests import cp_pass_ref as ref
from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

ERR_ARG, UNSUPPORTED = -2, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 8


def _ptr(x):
    return None if x is None else ctypes.c_void_p(x.ptr)


def _view(base, layout, N):
    """the device view of a factor matrix in the layout of the case"""
    from tt_sketch_amd.device import DevArray
    if base is None:
        return None
    dev = DevArray.from_host(base)
    return dev.T if layout == "transposed" else dev[:, 2:2 + N] if layout == "slice" else dev


def _cols(base, width):
    from tt_sketch_amd.device import DevArray
    return None if base is None else DevArray.from_host(base)[:, :width]


def _guarded(size):
    """a NaN-filled buffer with GUARD cells before and after the `size` cells of an output"""
    from tt_sketch_amd.device import DevArray
    return DevArray.from_host(np.full(size + 2 * GUARD, np.nan))


def _last_error():
    from tt_sketch_amd import _native as nat
    return nat.lib().ttsk_last_error().decode(errors="replace")


def c_chain(case, null=(), **over):
    """One direct call of ttsk_cp_chain_step: (status, the whole (N, rho' + pad) buffer of out or None)."""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    a = ref.chain_arrays(case)
    V = _view(a["V_base"], case.v, case.N)
    L = _cols(a["L_base"], case.rho)
    D = DevArray.from_host(a["D"])
    out = DevArray.from_host(np.full((case.N, case.rho1 + case.pad), np.nan))
    args = dict(L=_ptr(L), ldl=case.rho + case.pad, V=_ptr(V), v_k=V.strides[0], v_j=V.strides[1], D=_ptr(D), out=_ptr(out),
                ldo=case.rho1 + case.pad, N=case.N, rho=case.rho, n=case.n, rho1=case.rho1)
    args.update(over)
    for name in null:
        args[name] = None
    rc = nat.lib().ttsk_cp_chain_step(*[args[k] for k in ("L", "ldl", "V", "v_k", "v_j", "D", "out", "ldo", "N", "rho", "n", "rho1")], 0)
    nat.call("ttsk_sync", -1)
    return rc, (out.get() if rc == 0 else None)


def c_psi(case, null=(), **over):
    """One direct call of ttsk_cp_psi_omega: (status, psi buffer or None, omega buffer or None), the buffers with guards."""
    from tt_sketch_amd import _native as nat
    a = ref.psi_arrays(case)
    V = _view(a["V_base"], case.v, case.N)
    L, R, Ro = _cols(a["L_base"], case.l), _cols(a["R_base"], case.r), _cols(a["R_om_base"], case.omega or 0)
    r_om = 0 if case.omega is None else (case.omega or case.r)
    psi = _guarded(case.l * case.n * case.r) if case.n else None
    om = _guarded(case.l * r_om) if case.omega is not None else None
    args = dict(L=_ptr(L), ldl=case.l + case.pad, R=_ptr(R), ldr=case.r + case.pad, V=_ptr(V), v_k=V.strides[0] if V else 0,
                v_j=V.strides[1] if V else 0, psi=None if psi is None else _ptr(psi[GUARD:]), R_om=_ptr(Ro),
                ld_om=(case.omega or 0) + case.pad, r_om=case.omega or 0, omega=None if om is None else _ptr(om[GUARD:]),
                N=case.N, l=case.l, n=case.n, r=case.r)
    args.update(over)
    for name in null:
        args[name] = None
    rc = nat.lib().ttsk_cp_psi_omega(*[args[k] for k in ("L", "ldl", "R", "ldr", "V", "v_k", "v_j", "psi", "R_om", "ld_om", "r_om", "omega",
                                                        "N", "l", "n", "r")], 0)
    nat.call("ttsk_sync", -1)
    if rc:
        return rc, None, None
    return rc, (None if psi is None else psi.get()), (None if om is None else om.get())


def _inside(got, want, tol, what):
    off = np.abs(got - want)
    print(f"{what}: max |x - ref| / bound = {np.max(off / tol):.3f}")
    assert np.isfinite(got).all(), what
    assert (off <= tol).all(), what


# ---- 1. the C entries against the restatement, every edge
@pytest.mark.parametrize("case", ref.CHAIN_CASES, ids=lambda c: c.name)
def test_chain_step_entry_vs_restatement(tsa, case):
    a = ref.chain_arrays(case)
    rc, buf = c_chain(case)
    assert rc == 0                                           # in cover: the kernel itself, no fallback in between
    _inside(buf[:, :case.rho1], ref.chain_step(a["L"], a["V"], a["D"]), ref.chain_bound(a["L"], a["V"], a["D"]), case.name)
    assert np.isnan(buf[:, case.rho1:]).all()                # the cells past rho' of every row: untouched
    rc2, buf2 = c_chain(case)
    assert rc2 == 0 and np.array_equal(buf, buf2, equal_nan=True)       # the same bits on every call


@pytest.mark.parametrize("case", ref.PSI_CASES, ids=lambda c: c.name)
def test_psi_omega_entry_vs_restatement(tsa, case):
    a = ref.psi_arrays(case)
    rc, pbuf, obuf = c_psi(case)
    assert rc == 0
    if case.n:
        assert np.isnan(pbuf[:GUARD]).all() and np.isnan(pbuf[-GUARD:]).all()
        P = pbuf[GUARD:-GUARD].reshape(case.l, case.n, case.r)
        _inside(P, ref.psi(a["L"], a["R"], a["V"]), ref.psi_bound(a["L"], a["R"], a["V"]), case.name + " Psi")
    else:
        assert pbuf is None
    if case.omega is not None:
        Ro = a["R_om"] if case.omega else a["R"]
        assert np.isnan(obuf[:GUARD]).all() and np.isnan(obuf[-GUARD:]).all()
        O = obuf[GUARD:-GUARD].reshape(case.l, -1)
        _inside(O, ref.omega(a["L"], Ro, case.N), ref.omega_bound(a["L"], Ro, case.N), case.name + " Omega")
    else:
        assert obuf is None
    rc2, pbuf2, obuf2 = c_psi(case)
    assert rc2 == 0
    for x, y in ((pbuf, pbuf2), (obuf, obuf2)):
        assert (x is None and y is None) or np.array_equal(x, y, equal_nan=True)


def test_omega_in_the_launch_of_psi_equals_omega_alone(tsa):
    """the columns of Omega behind those of Psi and Omega as a call of its own: the same sums in the same order"""
    case = next(c for c in ref.PSI_CASES if c.name == "vslice_N1025")
    _, _, both = c_psi(case)
    rc, untouched, alone = c_psi(case, null=("psi", "V"))
    assert rc == 0 and np.isnan(untouched).all() and np.array_equal(both, alone, equal_nan=True)


# ---- 2. refusals
def test_refusals_of_the_entries(tsa):
    chain = next(c for c in ref.CHAIN_CASES if c.name == "N17_k32")
    for kw, status, word in ((dict(null=("out",)), ERR_ARG, "NULL"), (dict(null=("V",)), ERR_ARG, "NULL"), (dict(null=("D",)), ERR_ARG, "NULL"),
                             (dict(N=0), ERR_ARG, "N = 0"), (dict(rho1=129, ldo=200), UNSUPPORTED, "rank 129"),
                             (dict(rho=129, ldl=200), UNSUPPORTED, "rank 129"), (dict(ldo=chain.rho1 - 1), ERR_ARG, "leading dimension"),
                             (dict(null=("L",)), ERR_ARG, "rho = 1")):
        rc, _ = c_chain(chain, **kw)
        assert rc == status and word in _last_error() and _last_error().startswith("ttsk_cp_chain_step"), (kw, rc, _last_error())
    psi = next(c for c in ref.PSI_CASES if c.name == "N5_l17_r15_om_own")
    for kw, status, word in ((dict(null=("psi", "omega")), ERR_ARG, "NULL output"), (dict(null=("V",)), ERR_ARG, "NULL factor"),
                             (dict(N=0), ERR_ARG, "N = 0"), (dict(l=129, ldl=200), UNSUPPORTED, "rank 129"),
                             (dict(r=129, ldr=200), UNSUPPORTED, "rank 129"), (dict(r_om=129, ld_om=200), UNSUPPORTED, "rank 129"),
                             (dict(null=("R",)), ERR_ARG, "r = 1"), (dict(ld_om=psi.omega - 1), ERR_ARG, "Omega's right operand")):
        rc, _, _ = c_psi(psi, **kw)
        assert rc == status and word in _last_error() and _last_error().startswith("ttsk_cp_psi_omega"), (kw, rc, _last_error())


def _recorded_calls(fn):
    from tt_sketch_amd import _native as nat
    calls, real = [], nat.call
    try:
        nat.call = lambda name, *args: (calls.append(name), real(name, *args))[1]
        out = fn()
    finally:
        nat.call = real
    return out, calls


def test_past_the_cover_the_surface_composes(tsa):
    """right rank 129: both entries refuse, the sketch is the composition's and equals the oracle's"""
    from oracle import ttsk_oracle as orc
    from tt_sketch_amd import cp_fused
    from tt_sketch_amd.device import DevArray
    rng = np.random.default_rng(129)
    shape, N, l, r = (4, 5), 9, 3, 129
    factors = [rng.standard_normal((n, N)) for n in shape]
    ld, rd = orc.random_tt_drm(shape, l, False, rng), orc.random_tt_drm(shape, r, True, rng)
    left = tsa.TensorTrainDRM(l, shape, transpose=False, cores=ld.cores)
    right = tsa.TensorTrainDRM(r, shape, transpose=True, cores=rd.cores)
    stt, calls = _recorded_calls(lambda: tsa.stream_sketch(tsa.CPTensor(factors), (l,), (r,), left_drm=left, right_drm=right))
    assert "ttsk_gemm" in calls and "ttsk_cp_psi_omega" in calls                # asked, refused, composed
    Psis, Omegas = orc.general_sketch("cp", factors, ld, rd, "streaming")
    for got, want in zip(stt.Psi_cores + stt.Omega_mats, Psis + Omegas):
        assert got.shape == want.shape and np.linalg.norm(got - want) <= 1e-11 * np.linalg.norm(want)
    V, D = DevArray.from_host(factors[1]), DevArray.from_host(rd.cores[0])
    assert cp_fused.chain_step(None, V, D) is None
    with pytest.raises(tsa._native.TtskUnsupported, match="rank 129"):
        cp_fused.chain_step(None, V, D, route="kernel")


# ---- 3. the public API: kernels forced, compositions forced, the oracle
def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, (a.shape, b.shape)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def _run(tsa, method, make_tensor, left, right, route):
    """(list of arrays, tolerance, names of the C entries called): Psi + Omega of a streaming sketch, the cores otherwise"""
    from tt_sketch_amd import cp_fused

    def go():
        with cp_fused.forced(route):
            if method == "streaming":
                stt = tsa.stream_sketch(make_tensor(), left.rank, tuple(right.rank[::-1]), left_drm=left, right_drm=right)
                return list(stt.Psi_cores) + list(stt.Omega_mats)
            if method == "orthogonal":
                tt = tsa.orthogonal_sketch(make_tensor(), left.rank, tuple(right.rank[::-1]), left_drm=left, right_drm=right)
            else:
                tt = tsa.hmt_sketch(make_tensor(), tuple(right.rank[::-1]), drm=right)
            return [np.asarray(c) for c in tt.cores]
    out, calls = _recorded_calls(go)
    return out, (1e-11 if method == "streaming" else 1e-9), calls


def _three_ways(tsa, method, make_tensor, kind, data, ld, rd, cp_terms=True):
    from oracle import ttsk_oracle as orc
    left = tsa.TensorTrainDRM(ld.rank, ld.shape, transpose=False, cores=ld.cores)
    right = tsa.TensorTrainDRM(rd.rank[::-1], rd.shape, transpose=True, cores=rd.cores)
    kern, tol, kcalls = _run(tsa, method, make_tensor, left, right, "kernel")
    comp, _, ccalls = _run(tsa, method, make_tensor, left, right, "composed")
    assert "ttsk_cp_chain_step" in kcalls and "ttsk_cp_psi_omega" in kcalls
    assert not any(c.startswith("ttsk_cp_") for c in ccalls) and "ttsk_gemm" in ccalls
    Psis, Omegas = orc.general_sketch(kind, data, None if method == "hmt" else ld, rd, method)
    want = Psis + (Omegas if method == "streaming" else [])
    assert len(kern) == len(comp) == len(want)
    for k, (a, b, w) in enumerate(zip(kern, comp, want)):
        print(f"{method} array {k}: kernel against composition {_rel(a, b):.2e}, against the oracle {_rel(a, w):.2e}")
        assert _rel(a, b) <= tol and _rel(a, w) <= tol and _rel(b, w) <= tol, (method, k)
    return kcalls


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "cp_cases.npz"))


def _golden_case():
    from oracle import ttsk_oracle as orc
    z = _golden()
    d = int(z["d"])
    factors = [z[f"factor{k}"] for k in range(d)]
    shape = tuple(f.shape[0] for f in factors)
    ld = orc.TTDrm([z[f"left_core{k}"] for k in range(d - 1)], shape, False)
    rd = orc.TTDrm([z[f"right_core{k}"] for k in range(d - 1)], shape, True)
    return z, factors, ld, rd


@pytest.mark.parametrize("method", ["streaming", "orthogonal", "hmt"])
def test_d4_rank37_three_ways_and_the_recorded_reference(tsa, method):
    z, factors, ld, rd = _golden_case()
    assert tuple(f.shape for f in factors) == ((5, 37), (7, 37), (4, 37), (6, 37))
    calls = _three_ways(tsa, method, lambda: tsa.CPTensor([f.copy() for f in factors]), "cp", factors, ld, rd)
    if method == "streaming":                                # the fast path: 2 (d - 1) chain steps, d Psi launches, nothing else
        assert calls.count("ttsk_cp_chain_step") == 6 and calls.count("ttsk_cp_psi_omega") == 4 and "ttsk_gemm" not in calls
    # the device, kernels forced, against what the reference itself computed
    left = tsa.TensorTrainDRM(ld.rank, ld.shape, transpose=False, cores=ld.cores)
    right = tsa.TensorTrainDRM(rd.rank[::-1], rd.shape, transpose=True, cores=rd.cores)
    got, tol, _ = _run(tsa, method, lambda: tsa.CPTensor([f.copy() for f in factors]), left, right, "kernel")
    want = [z[f"{method}_psi{k}"] for k in range(4)] + ([z[f"{method}_omega{k}"] for k in range(3)] if method == "streaming" else [])
    for a, w in zip(got, want):
        assert _rel(a, w) <= tol


@pytest.mark.parametrize("method", ["streaming", "orthogonal", "hmt"])
def test_d2_three_ways(tsa, method):
    from oracle import ttsk_oracle as orc
    rng = np.random.default_rng(2)
    shape, N = (9, 8), 21
    factors = [rng.standard_normal((n, N)) / np.sqrt(n) for n in shape]
    ld, rd = orc.random_tt_drm(shape, 3, False, rng), orc.random_tt_drm(shape, 6, True, rng)
    _three_ways(tsa, method, lambda: tsa.CPTensor([f.copy() for f in factors]), "cp", factors, ld, rd)


@pytest.mark.parametrize("method", ["streaming", "orthogonal", "hmt"])
def test_sum_of_a_cp_and_a_tt_three_ways(tsa, method):
    from oracle import ttsk_oracle as orc
    rng = np.random.default_rng(3)
    shape, N = (5, 7, 4, 6), 37
    factors = [rng.standard_normal((n, N)) / np.sqrt(n) for n in shape]
    cores = orc.random_tt(shape, 3, rng)
    ld, rd = orc.random_tt_drm(shape, 3, False, rng), orc.TTDrm(
        [rng.standard_normal(s) / np.sqrt(s[0]) for s in ((1, 6, 6), (6, 4, 6), (6, 7, 5))], shape, True)
    make = lambda: tsa.TensorSum([tsa.CPTensor([f.copy() for f in factors]), tsa.TensorTrain([c.copy() for c in cores])])
    _three_ways(tsa, method, make, "sum", [("cp", factors), ("tt", cores)], ld, rd)


def test_rank_slices_of_a_blocked_drm(tsa):
    """slices of seeded DRMs through general_sketch: the fast path with cut contractions, the composition, the oracle"""
    from oracle import ttsk_oracle as orc
    from tt_sketch_amd import cp_fused
    from tt_sketch_amd.sketch_dispatch import SketchMethod, general_sketch
    rng = np.random.default_rng(4)
    shape, N = (5, 7, 4, 6), 37
    factors = [rng.standard_normal((n, N)) / np.sqrt(n) for n in shape]
    left = tsa.TensorTrainDRM((3, 6, 3), shape, transpose=False, seed=11).slice((1, 2, 0), (3, 5, 2))
    right = tsa.TensorTrainDRM((6, 7, 6), shape, transpose=True, seed=12).slice((2, 0, 3), (6, 4, 6))
    assert left.rank == (2, 3, 2) and right.rank[::-1] == (4, 4, 3)
    ld = orc.TTDrm([np.asarray(c) for c in left.cores], shape, False, left.rank_min, left.rank_max)
    rd = orc.TTDrm([np.asarray(c) for c in right.cores], shape, True, right.rank_min, right.rank_max)
    Psis, Omegas = orc.general_sketch("cp", factors, ld, rd, "streaming")
    outs = {}
    for route in ("kernel", "composed"):
        with cp_fused.forced(route):
            sk, calls = _recorded_calls(lambda: general_sketch(tsa.CPTensor([f.copy() for f in factors]), left, right, SketchMethod.streaming))
        assert ("ttsk_cp_psi_omega" in calls) == (route == "kernel") and ("ttsk_gemm" in calls) == (route == "composed")
        outs[route] = list(sk.Psi_cores) + list(sk.Omega_mats)
        for got, want in zip(outs[route], Psis + Omegas):
            assert _rel(got, want) <= 1e-11, route
    for a, b in zip(outs["kernel"], outs["composed"]):
        assert _rel(a, b) <= 1e-11


def test_forest_like_scaled_down(tsa):
    """d = 5, n = 6, N = 1000, l = 10, r = 20: two chunks of the sum over N, so Psi and Omega pass through the closing sum"""
    from oracle import ttsk_oracle as orc
    rng = np.random.default_rng(5)
    shape, N = (6,) * 5, 1000
    factors = [rng.standard_normal((n, N)) / np.sqrt(n) for n in shape]
    ld = orc.TTDrm([rng.standard_normal(s) / np.sqrt(s[0]) for s in ((1, 6, 6), (6, 6, 10), (10, 6, 10), (10, 6, 10))], shape, False)
    rd = orc.TTDrm([rng.standard_normal(s) / np.sqrt(s[0]) for s in ((1, 6, 20), (20, 6, 20), (20, 6, 20), (20, 6, 20))], shape, True)
    calls = _three_ways(tsa, "streaming", lambda: tsa.CPTensor([f.copy() for f in factors]), "cp", factors, ld, rd)
    assert calls.count("ttsk_cp_chain_step") == 8 and calls.count("ttsk_cp_psi_omega") == 5


def test_try_cp_sketch_declines_what_it_does_not_serve(tsa):
    from oracle import ttsk_oracle as orc
    from tt_sketch_amd import cp_fused
    from tt_sketch_amd.sketch_dispatch import SketchMethod
    rng = np.random.default_rng(6)
    shape = (5, 6, 4)
    cp = tsa.CPTensor([rng.standard_normal((n, 7)) for n in shape])
    tt = tsa.TensorTrain(orc.random_tt(shape, 2, rng))
    left, right = tsa.TensorTrainDRM(2, shape, transpose=False, seed=1), tsa.TensorTrainDRM(4, shape, transpose=True, seed=2)
    out = cp_fused.try_cp_sketch(cp, left, right, SketchMethod.streaming)
    assert out is not None and len(out[0]) == 3 and len(out[1]) == 2
    assert cp_fused.try_cp_sketch(cp, left, right, SketchMethod.streaming, route="composed") is None
    assert cp_fused.try_cp_sketch(tt, left, right, SketchMethod.streaming) is None
    assert cp_fused.try_cp_sketch(tsa.TensorSum([cp, cp]), left, right, SketchMethod.streaming) is None
    assert cp_fused.try_cp_sketch(cp, left, right, SketchMethod.orthogonal) is None
    assert cp_fused.try_cp_sketch(cp, left, right.T, SketchMethod.streaming) is None
    dense = tsa.DenseGaussianDRM(4, shape, transpose=True, seed=3)
    assert cp_fused.try_cp_sketch(cp, left, dense, SketchMethod.streaming) is None
    sparse = tsa.SparseGaussianDRM(2, shape, transpose=False, seed=4)
    assert cp_fused.try_cp_sketch(cp, sparse, right, SketchMethod.streaming) is None
    with pytest.raises(ValueError, match="Shape"):
        cp_fused.try_cp_sketch(cp, tsa.TensorTrainDRM(2, (5, 6, 5), transpose=False, seed=1), right, SketchMethod.streaming)
