"""Inner products with a CP tensor on the device: ``ttsk_cp_gram`` (csrc/cp_gram.hip), ``ttsk_sum`` and the Python surface
built on them (``cp_gram``, ``CPTensor.dot`` / ``norm``, ``TensorTrain.dot`` against a ``CPTensor`` on
``ttsk_cp_chain_step``, and through them ``error(fast=True)`` without a dense array).

Bars (tests/cp_gram_ref.py): |G - G_true| <= 2 L 2^-53 G_abs with G_true in np.longdouble, L the summation depth from
the plan's own numbers and G_abs the same sum on |factors|; the same with L = sum_k r_k n_k + N for <tt, cp>; two calls give
the same bits.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import cp_gram_ref as cr
from tests import gather_ref
from tests import tt_gram_ref
from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3
SENTINEL = 12345.678
U = 2.0 ** -53


@pytest.fixture(scope="module")
def n_cu(tsa):
    from tt_sketch_amd import _native as nat
    cu = ctypes.c_int(0)
    nat.call("ttsk_device_info", None, 0, ctypes.byref(cu), None)
    return cu.value


@functools.lru_cache(maxsize=None)
def truth(name):
    """(operands A, B, wide matrices, <a, b> in long double, sum of the |terms|) of a case: computed once"""
    case = next(c for c in cr.CASES if c.name == name)
    wa, wb = cr.case_factors(case)
    A, B = cr.operands(case, wa, wb)
    return A, B, wa, wb, cr.gram(A, B, dtype=np.longdouble), float(cr.gram(A, B, absolute=True))


def c_cp_gram(wa, wb, N, M, sym, *, d=None, N_arg=None, M_arg=None, lda=None, ldb=None, shape=None, null=(), b_like_a=None):
    """One direct call of the C entry: the factors are the first N (M) columns of the wide host matrices wa (wb).
    ``sym``: the pointers and leading dimensions of a are passed for b too.  The keyword arguments overwrite what the
    matrices say, for the argument tests.  (status, the double of dev_out, which starts as SENTINEL)."""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    dd = len(wa)
    da = [DevArray.from_host(np.ascontiguousarray(w, dtype=np.float64)) for w in wa]
    db = da if sym else [DevArray.from_host(np.ascontiguousarray(w, dtype=np.float64)) for w in wb]
    out = DevArray.from_host(np.full(1, SENTINEL))
    args = dict(a=nat.ptr_array(da), lda=nat.i64_array([w.shape[1] for w in wa] if lda is None else lda),
                b=nat.ptr_array(db), ldb=nat.i64_array([w.shape[1] for w in (wa if sym else wb)] if ldb is None else ldb),
                shape=nat.i64_array([w.shape[0] for w in wa] if shape is None else shape), out=ctypes.c_void_p(out.ptr))
    if b_like_a is not None:                       # b's pointers: a's, but for factor b_like_a one double further
        args["b"] = (ctypes.c_void_p * dd)(*[x.ptr + (8 if k == b_like_a else 0) for k, x in enumerate(da)])
    for name in null:
        if name in ("factor_a", "factor_b"):
            ptrs = [x.ptr for x in (da if name == "factor_a" else db)]
            ptrs[-1] = None
            args[name[-1]] = (ctypes.c_void_p * dd)(*ptrs)
        else:
            args[name] = None
    rc = nat.lib().ttsk_cp_gram(args["a"], args["lda"], N if N_arg is None else N_arg, args["b"], args["ldb"], M if M_arg is None else M_arg,
                                args["shape"], dd if d is None else d, int(sym), args["out"], 0)
    nat.call("ttsk_sync", -1)
    return rc, float(out.get()[0])


def run_case(case):
    A, B, wa, wb, ref, g_abs = truth(case.name)
    sym = case.M is None
    return c_cp_gram(wa, wb, case.N, case.N if sym else case.M, sym)


# ---- 1. the C entry against the long-double truth, every edge of N, M, modes, depth, slices, sym and the grid cap
@pytest.mark.parametrize("case", cr.CASES, ids=lambda c: c.name)
def test_c_entry_vs_longdouble(tsa, n_cu, case):
    A, B, wa, wb, ref, g_abs = truth(case.name)
    sym = case.M is None
    M = case.N if sym else case.M
    if "over_cap" in case.name:
        assert cr.run(case.N, M, sym, n_cu) >= 2                 # some workgroup does own two tiles on this chip
    rc, G = run_case(case)
    assert rc == 0
    tol = cr.bound(A, B, sym, n_cu)
    off = abs(float(G - ref))
    print(f"{case.name}: |G - G_true| / bound = {off / tol:.3f}, / G_abs = {off / g_abs:.2e}, L = {cr.depth(case.shape, case.N, M, sym, n_cu)}")
    assert np.isfinite(G) and off <= tol
    rc2, G2 = run_case(case)
    assert rc2 == 0 and np.float64(G).tobytes() == np.float64(G2).tobytes()       # the same bits on every call
    if sym:                                                      # against the unsymmetric call on the same data: both bounds
        rc3, G3 = c_cp_gram(wa, [w.copy() for w in wa], case.N, case.N, False)
        assert rc3 == 0 and abs(G - G3) <= tol + cr.bound(A, A, False, n_cu)
        assert G >= 0 or abs(G) <= tol


def test_sum_entry(tsa):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    rng = np.random.default_rng(8)
    for n in (0, 1, 255, 256, 257, 25_000):
        x = rng.standard_normal(n)
        out = DevArray.from_host(np.full(1, SENTINEL))
        dx = DevArray.from_host(x) if n else None
        for _ in range(2):
            nat.call("ttsk_sum", None if dx is None else ctypes.c_void_p(dx.ptr), ctypes.c_size_t(n), ctypes.c_void_p(out.ptr), 0)
            got = out.get()[0]
            # thread t adds ceil(n / 256) values, then 6 + 2 additions of the workgroup total
            assert abs(got - float(np.sum(x.astype(np.longdouble)))) <= 2 * (-(-n // 256) + 8) * U * float(np.sum(np.abs(x)))
            if _:
                assert got.tobytes() == first.tobytes()
            first = got
    out = DevArray.from_host(np.full(1, SENTINEL))
    assert nat.lib().ttsk_sum(None, ctypes.c_size_t(4), ctypes.c_void_p(out.ptr), 0) == nat.TTSK_ERR_ARG
    assert nat.lib().ttsk_sum(ctypes.c_void_p(out.ptr), ctypes.c_size_t(1), None, 0) == nat.TTSK_ERR_ARG
    assert nat.lib().ttsk_sum(ctypes.c_void_p(out.ptr), ctypes.c_size_t(2 ** 32), ctypes.c_void_p(out.ptr), 0) == UNSUPPORTED
    nat.call("ttsk_sync", -1)
    assert out.get()[0] == SENTINEL


# ---- 2. the ABI: every refusal returns its code and launches nothing
def test_every_refusal_leaves_the_output_untouched(tsa):
    from tt_sketch_amd import _native as nat
    rng = np.random.default_rng(1)
    shape, N, M = (4, 5), 6, 7
    wa, wb = [rng.standard_normal((n, N)) for n in shape], [rng.standard_normal((n, M)) for n in shape]
    rc, G = c_cp_gram(wa, wb, N, M, False)
    assert rc == 0 and G != SENTINEL
    ARG = nat.TTSK_ERR_ARG
    refused = [
        (ARG, dict(null=("a",))), (ARG, dict(null=("lda",))), (ARG, dict(null=("b",))), (ARG, dict(null=("ldb",))),
        (ARG, dict(null=("shape",))), (ARG, dict(null=("factor_a",))), (ARG, dict(null=("factor_b",))),
        (ARG, dict(d=0)), (ARG, dict(d=-3)),
        (ARG, dict(N_arg=0)), (ARG, dict(M_arg=0)), (ARG, dict(shape=[4, 0])), (ARG, dict(shape=[-1, 5])),
        (ARG, dict(lda=[N, N - 1])), (ARG, dict(ldb=[M - 1, M])),
        (UNSUPPORTED, dict(d=33)),
        (UNSUPPORTED, dict(N_arg=2 ** 31, lda=[2 ** 31] * 2)), (UNSUPPORTED, dict(M_arg=2 ** 31, ldb=[2 ** 31] * 2)),
        (UNSUPPORTED, dict(shape=[4, 2 ** 31])),
    ]
    for want, kw in refused:
        if kw.get("d") == 33:                                    # the pointer arrays must hold 33 entries for the call to be well formed
            w33a, w33b = [wa[0]] * 33, [wb[0]] * 33
            rc, G = c_cp_gram(w33a, w33b, N, M, False)
        else:
            rc, G = c_cp_gram(wa, wb, N, M, False, **kw)
        assert rc == want and G == SENTINEL, (kw, rc, G)
    assert c_cp_gram([wa[0]] * 32, [wb[0]] * 32, N, M, False)[0] == 0               # d = 32 is inside the cover
    rc, G = c_cp_gram(wa, wb, N, M, False, null=("out",))
    assert rc == ARG
    # sym: M != N, a factor of b that is not a's, a leading dimension that is not a's
    assert c_cp_gram(wa, wa, N, N, True)[0] == 0
    for kw in (dict(M_arg=N - 1), dict(b_like_a=1), dict(ldb=[N, N + 1])):
        rc, G = c_cp_gram(wa, wa, N, N, True, **kw)
        assert rc == ARG and G == SENTINEL, kw
    assert b"sym" in nat.lib().ttsk_last_error()


# ---- 3. <tt, cp> on ttsk_cp_chain_step and on the composition
@pytest.mark.parametrize("rank", [1, 16, 17, 128, 129])
def test_tt_dot_cp_on_both_routes(tsa, rank):
    from tt_sketch_amd import _native as nat, paths
    from tt_sketch_amd.device import DevArray
    rng = np.random.default_rng(rank)
    shape, N = (3, 4, 5), 65
    cores, V = cr.random_tt(rng, shape, (rank, rank)), [rng.standard_normal((n, N)) for n in shape]
    ref, tol = cr.tt_cp_dot(cores, V, dtype=np.longdouble), cr.tt_cp_bound(cores, V)
    tt = tsa.TensorTrain(cores).to_device()
    cp = tsa.CPTensor([DevArray.from_host(v) for v in V])
    got = {}
    calls = []
    real = nat.call
    try:
        nat.call = lambda name, *args: (calls.append(name), real(name, *args))[1]
        got["composed"] = tt.dot(cp, route="composed")
        assert "ttsk_cp_chain_step" not in calls and calls.count("ttsk_sum") == 1
        del calls[:]
        if rank <= cr.CHAIN_MAX_RANK:
            got["kernel"] = tt.dot(cp, route="kernel")
            assert calls.count("ttsk_cp_chain_step") == len(shape) and calls.count("ttsk_gemm") == 0 and calls.count("ttsk_sum") == 1
            got["kernel, cp first"] = cp.dot(tt, route="kernel")
            with paths.forced("kernel"):
                assert tt.dot(cp) == got["kernel"]
        else:
            with pytest.raises(nat.TtskUnsupported):
                tt.dot(cp, route="kernel")
    finally:
        nat.call = real
    got["rule"] = tt.dot(cp)
    got["rule, cp first"] = cp.dot(tt)
    with paths.forced("composed"):
        assert tt.dot(cp) == got["composed"]
    for what, g in got.items():
        print(f"rank {rank}, {what}: |g - true| / bound = {abs(float(g - ref)) / tol:.3f}")
        assert abs(float(g - ref)) <= tol, what
    if "kernel" in got:
        assert got["kernel"] == got["kernel, cp first"]


def test_tt_dot_cp_with_one_mode_and_transposes(tsa):
    from tt_sketch_amd.device import DevArray
    rng = np.random.default_rng(4)
    for shape, ranks, N in (((7,), (), 1), ((7,), (), 65), ((3, 1, 4), (5, 2), 17)):
        cores, V = cr.random_tt(rng, shape, ranks), [rng.standard_normal((n, N)) for n in shape]
        ref, tol = cr.tt_cp_dot(cores, V, dtype=np.longdouble), cr.tt_cp_bound(cores, V)
        tt, cp = tsa.TensorTrain(cores).to_device(), tsa.CPTensor([DevArray.from_host(v) for v in V])
        for route in ("kernel", "composed", None):
            assert abs(float(tt.dot(cp, route=route) - ref)) <= tol, (shape, route)
            assert abs(float(tt.T.dot(cp.T, route=route) - ref)) <= tol, (shape, route, "T")
    with pytest.raises(ValueError):
        tt.dot(tsa.CPTensor([DevArray.from_host(rng.standard_normal((n, 2))) for n in (3, 2, 4)]))


# ---- 4. the API end to end, with the host detour closed
def test_api_without_host_detour(tsa, n_cu, monkeypatch):
    from tt_sketch_amd import tensor as tmod
    from tt_sketch_amd.device import DevArray
    rng = np.random.default_rng(6)
    shape, Na, Nb, nnz = (4, 3, 5, 2), 7, 5, 20
    cores, cores2 = cr.random_tt(rng, shape, (3, 4, 2)), cr.random_tt(rng, shape, (2, 2, 3))
    A, B = [rng.standard_normal((n, Na)) for n in shape], [rng.standard_normal((n, Nb)) for n in shape]
    flat = rng.choice(int(np.prod(shape)), size=nnz, replace=False)
    idx, val = np.stack(np.unravel_index(flat, shape)).astype(np.int64), rng.standard_normal(nnz)
    tt, tt2 = tsa.TensorTrain(cores).to_device(), tsa.TensorTrain(cores2).to_device()
    cp, cp2 = tsa.CPTensor([DevArray.from_host(f) for f in A]), tsa.CPTensor([DevArray.from_host(f) for f in B])
    sp = tsa.SparseTensor(shape, idx, val)
    total = tsa.TensorSum([tt2, cp, sp])
    assert tt.resident() and cp.resident()

    def closed(a):
        raise AssertionError("host detour: tensor._host was called")

    with monkeypatch.context() as mp:
        mp.setattr(tmod, "_host", closed)
        got = dict(norm=cp.norm(), dot_cp=cp.dot(cp2), dot_cp_tt=cp.dot(tt), dot_tt_cp=tt.dot(cp), gram=tsa.cp_gram(cp, cp2),
                   gram_sym=tsa.cp_gram(cp), err=tt.error(cp, fast=True), err_rel=tt.error(cp, fast=True, relative=True),
                   err_cp_tt=cp.error(tt, fast=True, relative=True), err_sum=tt.error(total, fast=True),
                   err_sum_rel=tt.error(total, fast=True, relative=True))
    # ---- the truth: dense NumPy at this tiny shape
    T, T2, C, C2 = (tsa.TensorTrain(cores).to_numpy(), tsa.TensorTrain(cores2).to_numpy(), tsa.CPTensor(A).to_numpy(),
                    tsa.CPTensor(B).to_numpy())
    S = np.zeros(shape)
    S[tuple(idx)] = val
    b_aa, b_ab = cr.bound(A, A, True, n_cu), cr.bound(A, B, False, n_cu)
    b_tc = cr.tt_cp_bound(cores, A)
    # norm() is sqrt(abs(g)): squared again it carries three more roundings
    assert abs(got["norm"] ** 2 - np.sum(C * C)) <= b_aa + 4 * U * np.sum(C * C)
    assert got["gram_sym"] >= 0 and got["norm"] == float(np.sqrt(got["gram_sym"]))
    assert abs(got["dot_cp"] - np.sum(C * C2)) <= b_ab and got["gram"] == got["dot_cp"]
    assert abs(got["dot_cp_tt"] - np.sum(T * C)) <= b_tc and abs(got["dot_tt_cp"] - np.sum(T * C)) <= b_tc
    # ---- error(fast=True): err^2 = <t, t> + <x, x> - 2 <t, x>, each sum inside its bound; the host arithmetic that
    # combines them (fewer than 32 operations on numbers no larger than the sum of the |terms|) adds 64 u of that sum
    b_tt = tt_gram_ref.bound([cores], [cores], n_cu)[0, 0]       # the QR sweep of norm() is held to the Gram chain's bound
    tot = np.sum(T * T) + np.sum(C * C)
    true2 = np.sum((T - C) ** 2)
    slack = b_tt + b_aa + 2 * b_tc + 64 * U * (tot + 2 * abs(np.sum(T * C)))
    print(f"fast error^2 {got['err'] ** 2:.15e}, dense {true2:.15e}, allowed gap {slack:.1e}")
    assert slack < 1e-9 * true2                                  # the checks below do resolve the error
    assert abs(got["err"] ** 2 - true2) <= slack
    assert abs((got["err_rel"] * np.sqrt(np.sum(C * C))) ** 2 - true2) <= slack + 8 * U * true2
    assert abs((got["err_cp_tt"] * np.sqrt(np.sum(T * T))) ** 2 - true2) <= slack + 8 * U * true2
    # ---- against the sum tt2 + cp + sp: <x, x> is nine inner products, <t, x> three
    gabs = lambda cs, absolute=True: gather_ref.tt_gather(cs, idx, absolute=absolute)
    s_tt = lambda cs: 1e-12 * float(np.sum(np.abs(val) * gabs(cs)))                      # the bar of the gather sums
    s_cp = 1e-12 * float(np.sum(np.abs(val) * gather_ref.cp_gather(A, idx, absolute=True)))
    b_22 = tt_gram_ref.bound([cores2], [cores2], n_cu)[0, 0]
    b_t2 = tt_gram_ref.bound([cores], [cores2], n_cu)[0, 0]
    b_2c = cr.tt_cp_bound(cores2, A)
    b_ss = 2 * nnz * U * float(np.sum(val * val))
    b_xx = b_22 + b_aa + b_ss + 2 * (b_2c + s_tt(cores2) + s_cp)
    b_tx = b_t2 + b_tc + s_tt(cores)
    X = T2 + C + S
    tot = np.sum(T * T) + np.sum(X * X)
    mags = sum(abs(np.sum(P * Q)) for P in (T2, C, S) for Q in (T2, C, S)) + 2 * sum(abs(np.sum(T * Q)) for Q in (T2, C, S)) + np.sum(T * T)
    true2 = np.sum((T - X) ** 2)
    slack = b_tt + b_xx + 2 * b_tx + 64 * U * mags
    print(f"fast error^2 against the sum {got['err_sum'] ** 2:.15e}, dense {true2:.15e}, allowed gap {slack:.1e}")
    assert slack < 1e-9 * true2
    assert abs(got["err_sum"] ** 2 - true2) <= slack
    assert abs((got["err_sum_rel"] * np.sqrt(np.sum(X * X))) ** 2 - true2) <= slack + 8 * U * true2
    # ---- the condition of the device path: a host tensor against a resident one goes there and is uploaded once; two
    # host objects stay on the host
    host_cp, host_tt = tsa.CPTensor(A), tsa.TensorTrain(cores)
    assert abs(host_cp.dot(cp2) - np.sum(C * C2)) <= b_ab and host_cp._dev is not None
    assert abs(host_cp.norm() ** 2 - np.sum(C * C)) <= b_aa + 4 * U * np.sum(C * C)
    assert abs(host_tt.dot(cp) - np.sum(T * C)) <= b_tc and host_tt._dev is not None
    fresh_cp, fresh_tt = tsa.CPTensor(A), tsa.TensorTrain(cores)
    assert fresh_cp.dot(fresh_tt) == float(np.dot(T.ravel(), C.ravel())) and fresh_cp._dev is None and fresh_tt._dev is None
    with pytest.raises(ValueError):
        tsa.cp_gram(cp, tsa.CPTensor([DevArray.from_host(f) for f in A[:3]]))
    with pytest.raises(TypeError):
        tsa.cp_gram(cp, tt)


def test_cp_gram_takes_slices_and_copies_other_views(tsa, n_cu):
    """device factors that are column slices go to the entry as they are (lda > N); a transposed view is copied"""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    case = next(c for c in cr.CASES if c.name == "d5_slices")
    A, B, wa, wb, ref, g_abs = truth(case.name)
    a = tsa.CPTensor([DevArray.from_host(w)[:, :case.N] for w in wa])
    b = tsa.CPTensor([DevArray.from_host(np.ascontiguousarray(x.T)).T for x in B])
    calls = []
    real = nat.call
    try:
        nat.call = lambda name, *args: (calls.append(name), real(name, *args))[1]
        g = tsa.cp_gram(a, b)
    finally:
        nat.call = real
    # (the transposed view of a one-row factor is contiguous as it is)
    assert calls.count("ttsk_cp_gram") == 1 and calls.count("ttsk_copy_strided") == sum(n > 1 for n in case.shape)
    assert abs(float(g - ref)) <= cr.bound(A, B, False, n_cu)
    assert g == run_case(case)[1]                                # the same bits as the direct call


# ---- 5. against runs of the reference
@pytest.mark.parametrize("case", cr.load_cases(), ids=lambda c: c["name"])
def test_api_vs_reference_fixtures(tsa, n_cu, case):
    from tt_sketch_amd.device import DevArray
    A, B, cores = case["factors_a"], case["factors_b"], case["cores"]
    a, b = tsa.CPTensor([DevArray.from_host(f) for f in A]), tsa.CPTensor([DevArray.from_host(f) for f in B])
    tt = tsa.TensorTrain(cores).to_device()
    # the reference sums dense arrays in float64: it is held to 1e-12 of the |terms|, the device to its bound
    aa, ab, ta = float(cr.gram(A, A, absolute=True)), float(cr.gram(A, B, absolute=True)), float(cr.tt_cp_dot(cores, A, absolute=True))
    assert abs(a.norm() ** 2 - case["norm_a"] ** 2) <= cr.bound(A, A, True, n_cu) + 1e-12 * aa
    assert abs(a.dot(b) - case["dot_ab"]) <= cr.bound(A, B, False, n_cu) + 1e-12 * ab
    assert abs(b.dot(a) - case["dot_ab"]) <= cr.bound(B, A, False, n_cu) + 1e-12 * ab
    assert abs(a.dot(tt) - case["dot_a_tt"]) <= cr.tt_cp_bound(cores, A) + 1e-12 * ta
    assert abs(tt.dot(a) - case["dot_tt_a"]) <= cr.tt_cp_bound(cores, A) + 1e-12 * ta
    # the reference's own fast formula is the yardstick of the error value; the recorded errors are far above its floor
    assert case["error_tt_a"] > 1e-2
    assert abs(tt.error(a, fast=True, relative=True) - case["error_tt_a"]) <= 1e-9 * case["error_tt_a"]
    assert abs(a.error(tt, fast=True, relative=True) - case["error_a_tt"]) <= 1e-9 * case["error_a_tt"]
