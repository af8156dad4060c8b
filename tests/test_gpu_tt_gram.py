"""Gram matrix of tensor trains on the device: ``ttsk_tt_gram`` (csrc/tt_gram.hip) and the Python surface built on it
(``tt_gram``, resident ``TensorTrain.dot`` / ``gram_norm`` / ``error(fast=True)``).

Bar (tests/tt_gram_ref.py): entry by entry |G - G_ref| <= 2 L 2^-53 G_abs with L the summation depth of the pair and
G_abs the same chain on |cores|; two calls give the same bits.
"""
import ctypes

import numpy as np
import pytest

from tests import tt_gram_ref as gr
from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3


@pytest.fixture(scope="module")
def n_cu(tsa):
    from tt_sketch_amd import _native as nat
    cu = ctypes.c_int(0)
    nat.call("ttsk_device_info", None, 0, ctypes.byref(cu), None)
    return cu.value


def c_gram(A, B, shape=None, d=None, K=None, M=None, ranks_a=None, ranks_b=None, null=()):
    """One direct call of the C entry on host cores: (status, G (K, M) or None).  The keyword arguments overwrite what
    the cores say, for the argument tests."""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    shape = [c.shape[1] for c in A[0]] if shape is None else shape
    dd = len(A[0])
    dev = [[DevArray.from_host(np.ascontiguousarray(c, dtype=np.float64)) for c in t] for t in list(A) + list(B)]
    rk = [[c.shape[0] for c in t] + [t[-1].shape[2]] for t in list(A) + list(B)]
    ka, kb = len(A), len(B)
    ra = [r for row in rk[:ka] for r in row] if ranks_a is None else ranks_a
    rb = [r for row in rk[ka:] for r in row] if ranks_b is None else ranks_b
    out = DevArray.from_host(np.full((ka, kb), np.nan))
    args = dict(ca=nat.ptr_array([c for t in dev[:ka] for c in t]), ra=nat.i64_array(ra), cb=nat.ptr_array([c for t in dev[ka:] for c in t]),
                rb=nat.i64_array(rb), shape=nat.i64_array(shape), out=ctypes.c_void_p(out.ptr))
    for name in null:
        args[name] = None
    rc = nat.lib().ttsk_tt_gram(args["ca"], args["ra"], ka if K is None else K, args["cb"], args["rb"], kb if M is None else M,
                                args["shape"], dd if d is None else d, args["out"], 0)
    nat.call("ttsk_sync", -1)
    return rc, (out.get() if rc == 0 else None)


def check(G, A, B, n_cu, what):
    ref, tol = gr.gram(A, B), gr.bound(A, B, n_cu)
    off = np.abs(G - ref)
    print(f"{what}: max |G - G_ref| / bound = {np.max(off / tol):.3f}, max |G - G_ref| / G_abs = {np.max(off / gr.gram(A, B, absolute=True)):.2e}")
    assert np.isfinite(G).all(), what
    assert (off <= tol).all(), what


# ---- 1. the C entry against the NumPy chain, every edge of ranks, modes, depth and batch
@pytest.mark.parametrize("case", gr.CASES, ids=lambda c: c.name)
def test_c_entry_vs_restatement(tsa, n_cu, case):
    A, B = gr.case_cores(case)
    rc, G = c_gram(A, B)
    assert rc == 0                                           # in cover: the kernel itself, no fallback in between
    check(G, A, B, n_cu, case.name)
    rc2, G2 = c_gram(A, B)
    assert rc2 == 0 and np.array_equal(G, G2)                # the same bits on every call
    if case.ranks_b is None:                                 # tt_gram(As): symmetric within the bound, diagonal >= 0
        assert (np.abs(G - G.T) <= gr.bound(A, B, n_cu)).all() and (np.diag(G) >= 0).all()


def test_tt_gram_surface(tsa, n_cu):
    case = next(c for c in gr.CASES if c.name == "sym_4")
    A, _ = gr.case_cores(case)
    res = [tsa.TensorTrain(a).to_device() for a in A]
    G = tsa.tt_gram(res)
    assert G.shape == (4, 4) and G.dtype == np.float64
    check(G, A, A, n_cu, "tt_gram(As)")
    assert (np.abs(G - G.T) <= gr.bound(A, A, n_cu)).all() and (np.diag(G) >= 0).all()
    assert np.array_equal(G, tsa.tt_gram(res, res))
    host = [tsa.TensorTrain(a) for a in A]                   # host trains are uploaded once through dev_cores()
    G13 = tsa.tt_gram(host[:1], res[1:])
    check(G13, A[:1], A[1:], n_cu, "tt_gram(host, resident)")
    assert host[0]._dev is not None
    with pytest.raises(ValueError):
        tsa.tt_gram(res, [tsa.TensorTrain(gr.random_cores(np.random.default_rng(0), (2, 7, 2, 6), (2, 2, 2)))])


def test_lists_longer_than_one_call_are_cut_into_blocks(tsa, n_cu):
    """130 against 130 rank-1 trains: K + M = 260 is past the 128 trains of one ttsk_tt_gram call, so tt_gram makes nine
    calls on blocks of at most 64 x 64 and places them; every entry against the NumPy chain, and the same bits again."""
    from tt_sketch_amd import _native as nat
    rng = np.random.default_rng(130)
    shape = (2, 3)
    A = [gr.random_cores(rng, shape, (1,)) for _ in range(130)]
    res = [tsa.TensorTrain(a).to_device() for a in A]
    calls = []
    real = nat.call
    try:
        nat.call = lambda name, *args: (calls.append(name), real(name, *args))[1]
        G = tsa.tt_gram(res)
    finally:
        nat.call = real
    assert calls.count("ttsk_tt_gram") == 9 and G.shape == (130, 130)
    ref, off = gr.gram(A, A), np.zeros((130, 130))
    for p in range(0, 130, 64):                              # the bound of each block as its own call sees it
        for q in range(0, 130, 64):
            off[p:p + 64, q:q + 64] = gr.bound(A[p:p + 64], A[q:q + 64], n_cu)
    assert (np.abs(G - ref) <= off).all()
    assert np.array_equal(G, tsa.tt_gram(res, res))
    G2 = tsa.tt_gram(res[:3], res)                           # 3 + 130 trains: blocks along one side only
    assert G2.shape == (3, 130)
    for q in range(0, 130, 64):
        assert (np.abs(G2[:, q:q + 64] - ref[:3, q:q + 64]) <= gr.bound(A[:3], A[q:q + 64], n_cu)).all()


# ---- 2. the API on resident trains against the host path
def test_dot_norm_error_on_resident_trains(tsa, n_cu):
    rng = np.random.default_rng(12)
    shape = (5, 7, 6, 4)
    a = gr.random_cores(rng, shape, (6, 17, 5))
    pert = gr.random_cores(rng, shape, (2, 3, 2))
    ha, hp = tsa.TensorTrain(a), tsa.TensorTrain(pert)
    scale = 1e-3 * ha.norm() / hp.norm()
    hb = ha.add(hp * scale)                                  # relative error about 1e-3: far above the formula's 1e-8 floor
    b = [np.asarray(c) for c in hb.cores]
    da, db = ha.to_device(), tsa.TensorTrain(b).to_device()
    assert da.resident() and db.resident()
    tol = gr.bound([a], [b], n_cu)[0, 0]
    assert abs(da.dot(db) - ha.dot(hb)) <= 2 * tol           # both sides carry the chain's rounding
    naa = gr.dot(a, a)
    assert abs(da.gram_norm() - np.sqrt(naa)) <= gr.bound([a], [a], n_cu)[0, 0] / np.sqrt(naa)
    assert abs(da.gram_norm() - ha.norm()) <= 1e-12 * ha.norm()
    # error(fast=True): the reference formula (tensor.py:68-72) on NumPy norms and dot
    na, nb, ab = ha.norm(), hb.norm(), ha.dot(hb)
    tot = na ** 2 + nb ** 2
    want = np.sqrt(tot) * np.sqrt(abs(1 - 2 * ab / tot))
    true = ha.error(hb)
    assert 0.5e-3 < true / nb < 2e-3
    # err^2 = <a, a> + <b, b> - 2 <a, b>: the device's three sums are off by at most their bounds T, the NumPy dot of
    # `want` by T[0, 1] again (the QR norms are good to a few ulp), and d(err) = d(err^2) / (2 err)
    T = gr.bound([a, b], [a, b], n_cu)                       # error() makes one 2 x 2 call
    slack = (T[0, 0] + T[1, 1] + 4 * T[0, 1]) / (2 * min(want, true))
    got, got_rel = da.error(db, fast=True), da.error(db, fast=True, relative=True)
    print(f"fast error {got:.6e}, formula on NumPy {want:.6e}, true {true:.6e}, allowed gap {slack:.1e}")
    assert slack < 1e-2 * true                               # the check below does resolve the error
    assert abs(got - want) <= slack
    assert abs(got_rel - want / nb) <= slack / nb * (1 + 1e-9)
    assert abs(da.error(db, fast=True, rmse=True) - want / np.sqrt(np.prod(shape))) <= slack / np.sqrt(np.prod(shape))
    assert abs(got - true) <= slack
    # fast=False keeps the QR sweep of the direct sum
    assert abs(da.error(db) - true) <= 1e-9 * true
    assert abs(da.error(db, relative=True) - true / nb) <= 1e-9 * true / nb


def test_rank_past_the_cover_is_refused_by_c_and_composed_by_python(tsa, n_cu):
    rng = np.random.default_rng(3)
    shape = (3, 4, 3)
    a, b = gr.random_cores(rng, shape, (130, 5)), gr.random_cores(rng, shape, (4, 7))
    assert c_gram([a], [b])[0] == UNSUPPORTED
    da, db = tsa.TensorTrain(a).to_device(), tsa.TensorTrain(b).to_device()
    ref, tol = gr.dot(a, b), gr.bound([a], [b], n_cu)[0, 0]
    assert abs(da.dot(db) - ref) <= 2 * tol                  # the composed chain and NumPy: each within half the bound
    assert abs(db.dot(da) - ref) <= 2 * tol
    G = tsa.tt_gram([da, db])
    assert abs(G[0, 1] - ref) <= 2 * tol and abs(G[1, 0] - ref) <= 2 * tol


def test_route_keyword_and_forced_context(tsa, n_cu):
    """``route=`` of tt_gram: the pass itself under "kernel" (ranks on both sides of 16: the FMA and the matrix-instruction
    body), the chain under "composed" and under ``forced("composed")``, and past the cover a refusal instead of the chain."""
    from tt_sketch_amd import _native as nat, paths, tensor_gram as tmod
    rng = np.random.default_rng(21)
    shape = (3, 4, 3)
    A = [gr.random_cores(rng, shape, rk) for rk in ((1, 15), (16, 17))]
    B = [gr.random_cores(rng, shape, rk) for rk in ((17, 1), (15, 16), (16, 16))]
    dA, dB = [tsa.TensorTrain(a).to_device() for a in A], [tsa.TensorTrain(b).to_device() for b in B]
    G = tsa.tt_gram(dA, dB, route="kernel")
    assert G.shape == (2, 3)
    check(G, A, B, n_cu, "tt_gram(route='kernel')")
    assert np.array_equal(G, tsa.tt_gram(dA, dB, route="kernel"))
    composed = tsa.tt_gram(dA, dB, route="composed")
    assert np.array_equal(composed, tmod._gram_composed(dA, dB, False))
    with paths.forced("composed"):
        assert np.array_equal(tsa.tt_gram(dA, dB), composed)
    w = gr.random_cores(rng, shape, (129, 5))
    wide = tsa.TensorTrain(w).to_device()
    with pytest.raises(nat.TtskUnsupported):
        tsa.tt_gram([wide], dB, route="kernel")
    # None still composes, as in the test above: the chain and NumPy each within half the bound
    assert (np.abs(tsa.tt_gram([wide], dB) - gr.gram([w], B)) <= 2 * gr.bound([w], B, n_cu)).all()


# ---- 3. the ABI
def test_argument_errors(tsa):
    from tt_sketch_amd import _native as nat
    rng = np.random.default_rng(1)
    shape = (4, 5, 6)
    a, b = gr.random_cores(rng, shape, (2, 3)), gr.random_cores(rng, shape, (3, 2))
    assert c_gram([a], [b])[0] == 0
    for name in ("ca", "ra", "cb", "rb", "shape", "out"):
        assert c_gram([a], [b], null=(name,))[0] == nat.TTSK_ERR_ARG, name
    assert c_gram([a], [b], d=0)[0] == nat.TTSK_ERR_ARG
    assert c_gram([a], [b], K=0)[0] == nat.TTSK_ERR_ARG
    assert c_gram([a], [b], M=0)[0] == nat.TTSK_ERR_ARG
    assert c_gram([a], [b], ranks_a=[2, 2, 3, 1])[0] == nat.TTSK_ERR_ARG          # boundary rank
    assert b"boundary" in nat.lib().ttsk_last_error()
    assert c_gram([a], [b], ranks_b=[1, 3, 2, 2])[0] == nat.TTSK_ERR_ARG
    assert c_gram([a], [b], ranks_a=[1, 0, 3, 1])[0] == nat.TTSK_ERR_ARG          # a rank below 1
    assert c_gram([a], [b], ranks_b=[1, 129, 2, 1])[0] == UNSUPPORTED             # past the cover: nothing is launched
    assert b"129" in nat.lib().ttsk_last_error()
    assert c_gram([a], [b], shape=[4, 5, 2 ** 31])[0] == UNSUPPORTED
