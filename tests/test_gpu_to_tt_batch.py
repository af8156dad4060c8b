"""to_tt_batch / ttsk_tt_assemble_batch: the assembly of many streaming sketches at once (reference sketch.py:400-443).

Parity in TT form against the oracle's ``assemble`` (gelsd) on the device sketch's own Psi / Omega, at small odd shapes,
at C3 (d = 6, n = 200, TT rank 100, l = 50, r = 100) over a whole batch of 32, with rank-deficient and ill-conditioned
Omega inside a batch, the fused apply kernel element by element at the edges of its cover, and the C ABI's argument
errors.
"""
import ctypes

import numpy as np
import pytest

from oracle import ttsk_oracle as orc

from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

TENSOR_TOL = 1e-10          # full-rank Omega (tests/test_gpu_c3_solves.py)
ROBUST_TOL = 1e-9           # rank-deficient / ill-conditioned Omega (the Jacobi path)
TILE = 32                   # rows of a tile of the fused apply (AB_TM in assemble_batch.hip)
COVER_MIN, COVER_MAX = 56, 112


def tt_norm(cores):
    carry = np.ones((1, 1))
    for c in cores:
        m = np.tensordot(carry, c, axes=(1, 0)).reshape(-1, c.shape[2])
        carry = np.linalg.qr(m, mode="r")
    return float(np.linalg.norm(carry))


def tt_rel_diff(a, b):
    """|| A - B || / || B || for two TTs given as core lists (QR sweep over the direct sum)."""
    d = len(a)
    out = []
    for k, (x, y) in enumerate(zip(a, b)):
        x, y = np.asarray(x), np.asarray(y)
        r1 = 1 if k == 0 else x.shape[0] + y.shape[0]
        r2 = 1 if k == d - 1 else x.shape[2] + y.shape[2]
        blk = np.zeros((r1, x.shape[1], r2))
        blk[:x.shape[0], :, :x.shape[2]] = x
        blk[r1 - y.shape[0]:, :, r2 - y.shape[2]:] = -y if k == 0 else y
        out.append(blk)
    return tt_norm(out) / tt_norm([np.asarray(c) for c in b])


def host_sketch(stt):
    """Psi / Omega of a sketch on the host without moving the container off the device."""
    from tt_sketch_amd.device import to_host
    Psi, Om = stt.sketch_.device_arrays()
    return [np.array(to_host(p)) for p in Psi], [np.array(to_host(o)) for o in Om]


def drms(tsa, shape, l, r, rng):
    ld, rd = orc.random_tt_drm(shape, l, False, rng), orc.random_tt_drm(shape, r, True, rng)
    left = tsa.TensorTrainDRM(l, shape, False, seed=1, cores=[np.array(c) for c in ld.cores])
    right = tsa.TensorTrainDRM(r, shape, True, seed=2, cores=[np.array(c) for c in rd.cores])
    return left, right


SMALL = {3: ((9, 11, 13), 13, 7, 11), 4: ((13, 9, 11, 15), 13, 7, 11), 6: ((13, 15, 14, 13, 17, 15), 13, 7, 11)}


@pytest.mark.parametrize("d", [3, 4, 6])
@pytest.mark.parametrize("batch", [1, 2, 32, 33])
def test_small_batches_vs_oracle(tsa, d, batch):
    """Both directions and "auto" (to_tt_batch) on stream_sketch_batch outputs, every tensor against the oracle."""
    from tt_sketch_amd.sketch import assemble_sketched_tt_batch
    shape, s, l, r = SMALL[d]
    rng = np.random.default_rng(100 * d + batch)
    left, right = drms(tsa, shape, l, r, rng)
    tts = [tsa.TensorTrain(orc.random_tt(shape, s, rng)) for _ in range(batch)]
    sks = tsa.stream_sketch_batch(tts, (l,) * (d - 1), (r,) * (d - 1), left_drm=left, right_drm=right)
    hosts = [host_sketch(sk) for sk in sks]
    for direction in ("right", "left"):
        got = assemble_sketched_tt_batch([sk.sketch_ for sk in sks], direction=direction)
        assert len(got) == batch
        for cores, (P, O) in zip(got, hosts):
            want = orc.assemble(P, O, direction)
            assert [c.shape for c in cores] == [c.shape for c in want]
            assert tt_rel_diff(cores, want) < TENSOR_TOL, direction
    out = tsa.to_tt_batch(sks)
    assert len(out) == batch
    from tt_sketch_amd.device import DevArray
    for tt, (P, O) in zip(out, hosts):
        assert all(isinstance(c, DevArray) for c in tt.cores)             # device-resident, like to_tt
        assert tt_rel_diff([np.asarray(c) for c in tt.cores], orc.assemble(P, O, "auto")) < TENSOR_TOL


def test_mixed_signatures_keep_order_and_fallback(tsa, monkeypatch):
    """Two signatures interleaved and a host-array sketch: outputs in input order, the host sketch through s.to_tt()."""
    from tt_sketch_amd import sketch as sk_mod
    rng = np.random.default_rng(7)
    shape = (13, 15, 14, 13)
    la, ra, lb, rb = 7, 11, 5, 9
    A = drms(tsa, shape, la, ra, rng)
    B = drms(tsa, shape, lb, rb, rng)
    ska = tsa.stream_sketch_batch([tsa.TensorTrain(orc.random_tt(shape, 13, rng)) for _ in range(3)], (la,) * 3, (ra,) * 3,
                                  left_drm=A[0], right_drm=A[1])
    skb = tsa.stream_sketch_batch([tsa.TensorTrain(orc.random_tt(shape, 13, rng)) for _ in range(3)], (lb,) * 3, (rb,) * 3,
                                  left_drm=B[0], right_drm=B[1])
    host_one = tsa.stream_sketch(tsa.TensorTrain(orc.random_tt(shape, 13, rng)), (la,) * 3, (ra,) * 3, left_drm=A[0], right_drm=A[1])
    host_one.sketch_._to_host()                          # host arrays: not for the batched call
    sks = [ska[0], skb[0], ska[1], host_one, skb[1], ska[2], skb[2]]
    hosts = [host_sketch(s) if s is not host_one else (host_one.Psi_cores, host_one.Omega_mats) for s in sks]
    calls = []
    real = sk_mod._assemble_batch_call
    monkeypatch.setattr(sk_mod, "_assemble_batch_call", lambda g, dr: calls.append(len(g)) or real(g, dr))
    to_tt_calls = []
    real_to_tt = sk_mod.SketchedTensorTrain.to_tt
    monkeypatch.setattr(sk_mod.SketchedTensorTrain, "to_tt", lambda self: to_tt_calls.append(self) or real_to_tt(self))
    out = tsa.to_tt_batch(sks)
    assert sorted(calls) == [3, 3]
    assert to_tt_calls == [host_one]
    for tt, (P, O) in zip(out, hosts):
        assert tt_rel_diff([np.asarray(c) for c in tt.cores], orc.assemble(P, O, "auto")) < TENSOR_TOL
    assert tsa.to_tt_batch([]) == []


# ---------------------------------------------------------------- C3

SHAPE, S_IN, L, R, NB = (200,) * 6, 100, 50, 100, 32


def device_tt(tsa, shape, rank, seed):
    """bench.py's inputs: cores N(0, 1) / sqrt(r1 n) generated in HBM."""
    from tt_sketch_amd.utils import random_normal_dev
    S = (1,) + (rank,) * (len(shape) - 1) + (1,)
    return tsa.TensorTrain([random_normal_dev((S[k], shape[k], S[k + 1]), seed=(seed << 8) + k, scale=1.0 / np.sqrt(S[k] * shape[k]))
                            for k in range(len(shape))])


@pytest.fixture(scope="module")
def c3_drms(tsa):
    return drms(tsa, SHAPE, L, R, np.random.default_rng(33))


def test_c3_batch_every_tensor(tsa, c3_drms):
    """The bench's batch of 32: every tensor against the oracle (1e-10) and against its own to_tt() (1e-12)."""
    left, right = c3_drms
    tts = [device_tt(tsa, SHAPE, S_IN, 1000 + b) for b in range(NB)]
    sks = tsa.stream_sketch_batch(tts, (L,) * 5, (R,) * 5, left_drm=left, right_drm=right)
    got = tsa.to_tt_batch(sks)
    for b, (tt, sk) in enumerate(zip(got, sks)):
        cores = [np.asarray(c) for c in tt.cores]
        P, O = host_sketch(sk)
        assert tt_rel_diff(cores, orc.assemble(P, O, "right")) < TENSOR_TOL, b
        one = [np.asarray(c) for c in sk.to_tt().cores]
        assert tt_rel_diff(cores, one) <= 1e-12, b


def test_c3_robust_path_inside_batch(tsa, c3_drms):
    """Tensor 3 has TT rank 30 (every Omega rank 30 of 50), tensor 5 gets Omega with singular values down to 1e-7: both
    take the Jacobi path on the device, alone; the rest of the batch is unaffected."""
    from tt_sketch_amd import _native as nat
    left, right = c3_drms
    rng = np.random.default_rng(35)
    tts = [device_tt(tsa, SHAPE, S_IN, 2000 + b) for b in range(8)]
    low = orc.random_tt(SHAPE, 30, rng)
    padded = []
    for k, c in enumerate(low):                          # the rank-30 TT in rank-100 cores (zero blocks)
        r1 = 1 if k == 0 else S_IN
        r2 = 1 if k == len(SHAPE) - 1 else S_IN
        z = np.zeros((r1, SHAPE[k], r2))
        z[:c.shape[0], :, :c.shape[2]] = c
        padded.append(z)
    tts[3] = tsa.TensorTrain(padded)
    sks = tsa.stream_sketch_batch(tts, (L,) * 5, (R,) * 5, left_drm=left, right_drm=right)
    _, Om = sks[5].sketch_.device_arrays()
    for k, o in enumerate(Om):                           # Omega_k of tensor 5 <- U diag(logspace(0, -7)) V^T, same norm
        U, _ = np.linalg.qr(rng.standard_normal((L, L)))
        V, _ = np.linalg.qr(rng.standard_normal((R, L)))
        ill = (U * np.logspace(0, -7, L)) @ V.T
        ill *= np.linalg.norm(o.get()) / np.linalg.norm(ill)
        ill = np.ascontiguousarray(ill)
        nat.call("ttsk_h2d", ctypes.c_void_p(o.contiguous().ptr), ill.ctypes.data_as(ctypes.c_void_p), ill.nbytes, 0)
        assert o.contiguous().ptr == o.ptr
    got = tsa.to_tt_batch(sks)
    for b, (tt, sk) in enumerate(zip(got, sks)):
        cores = [np.asarray(c) for c in tt.cores]
        P, O = host_sketch(sk)
        tol = ROBUST_TOL if b in (3, 5) else TENSOR_TOL
        assert tt_rel_diff(cores, orc.assemble(P, O, "right")) < tol, b
    assert tt_rel_diff([np.asarray(c) for c in got[3].cores], low) < ROBUST_TOL


# ---------------------------------------------------------------- the fused apply at its edges, element by element

def _call_batch(count, d, n, lr, rr, psi, om, cores, work, direction):
    from tt_sketch_amd import _native as nat
    I64, P = ctypes.c_int64, ctypes.c_void_p
    arr = lambda T, v: (T * max(len(v), 1))(*v)
    return nat.lib().ttsk_tt_assemble_batch(count, d, arr(I64, n), arr(I64, lr), arr(I64, rr), arr(P, psi), arr(P, om),
                                            arr(P, cores), arr(P, work), direction, 0)


EDGE = [(50, 100, 1), (50, 100, TILE - 1), (50, 100, TILE + 1), (55, 110, 2 * TILE + 1),
        (COVER_MIN, COVER_MAX, TILE + 1), (COVER_MAX, COVER_MIN, TILE - 1), (COVER_MIN + 1, COVER_MAX, TILE + 1)]


@pytest.mark.parametrize("l,r,m", EDGE)
@pytest.mark.parametrize("direction", [0, 1])
def test_fused_apply_edges(tsa, l, r, m, direction):
    """d = 2, three tensors in one allocation: C = Psi P, R = Psi - C Omega, C += R P restated in NumPy with P read back
    from `work`; the last shape is just outside the cover and takes the fallback."""
    from tt_sketch_amd.device import DevArray, sync
    rng = np.random.default_rng(l * 1000 + r + m + direction)
    count = 3
    n = [m, 7] if direction == 0 else [5, m]
    psis, oms = [], []
    for _ in range(count):
        psis.append([rng.standard_normal((1, n[0], r)), rng.standard_normal((l, n[1], 1))])
        oms.append(rng.standard_normal((l, r)))
    cshape = (1, n[0], l) if direction == 0 else (r, n[1], 1)
    per = 2 * l * r + n[0] * r + l * n[1] + int(np.prod(cshape)) + r * l
    buf = DevArray.from_host(np.full(count * per, np.nan))
    views, off = [], 0

    def take(shape):
        nonlocal off
        sz = int(np.prod(shape))
        v = DevArray(buf.buf, buf.offset + off, shape, tuple(int(np.prod(shape[i + 1:])) for i in range(len(shape))))
        off += sz
        return v
    psi_p, om_p, core_p, work_p, outs, works = [], [], [], [], [], []
    from tt_sketch_amd import _native as nat
    for b in range(count):
        p0, p1, o = take(psis[b][0].shape), take(psis[b][1].shape), take(oms[b].shape)
        c, w = take(cshape), take((r, l))
        for dst, src in ((p0, psis[b][0]), (p1, psis[b][1]), (o, oms[b])):
            src = np.ascontiguousarray(src)
            nat.call("ttsk_h2d", ctypes.c_void_p(dst.ptr), src.ctypes.data_as(ctypes.c_void_p), src.nbytes, 0)
        psi_p += [p0.ptr, p1.ptr]
        om_p.append(o.ptr)
        core_p += [c.ptr, p1.ptr] if direction == 0 else [p0.ptr, c.ptr]    # the copied core aliases its Psi
        work_p.append(w.ptr)
        outs.append(c)
        works.append(w)
    assert off <= count * per
    rc = _call_batch(count, 2, n, [l], [r], psi_p, om_p, core_p, work_p, direction)
    assert rc == 0
    sync()
    for b in range(count):
        Pm = works[b].get()
        Om = oms[b]
        assert np.linalg.norm(Pm - np.linalg.pinv(Om)) <= 1e-8 * np.linalg.norm(Pm)
        if direction == 0:
            X = psis[b][0].reshape(n[0], r)
            C = X @ Pm
            C = C + (X - C @ Om) @ Pm
        else:
            X = psis[b][1].reshape(l, n[1])
            C = Pm @ X
            C = C + Pm @ (X - Om @ C)
        got = outs[b].get().reshape(C.shape)
        assert np.all(np.isfinite(got))
        assert np.max(np.abs(got - C)) <= 1e-12 * max(1.0, np.max(np.abs(C))), (b, np.max(np.abs(got - C)))


def test_c_abi_errors_run_nothing(tsa):
    """count = 0, a NULL Psi or Omega and direction = 2 are TTSK_ERR_ARG, and nothing is written."""
    from tt_sketch_amd.device import DevArray, sync
    l, r, n = 5, 7, [6, 4]
    rng = np.random.default_rng(1)
    psi0, psi1 = DevArray.from_host(rng.standard_normal((1, n[0], r))), DevArray.from_host(rng.standard_normal((l, n[1], 1)))
    om = DevArray.from_host(rng.standard_normal((l, r)))
    core, work = DevArray.from_host(np.full((1, n[0], l), 7.0)), DevArray.from_host(np.full((r, l), 7.0))
    good = dict(psi=[psi0.ptr, psi1.ptr], om=[om.ptr], cores=[core.ptr, psi1.ptr], work=[work.ptr])
    bad = [dict(count=0), dict(psi=[0, psi1.ptr]), dict(om=[0]), dict(direction=2)]
    for change in bad:
        a = dict(count=1, direction=0, **good)
        a.update(change)
        rc = _call_batch(a["count"], 2, n, [l], [r], a["psi"], a["om"], a["cores"], a["work"], a["direction"])
        assert rc == -2, change                       # TTSK_ERR_ARG
    sync()
    assert np.all(core.get() == 7.0) and np.all(work.get() == 7.0)
    assert _call_batch(1, 2, n, [l], [r], good["psi"], good["om"], good["cores"], good["work"], 0) == 0
    sync()
    assert not np.all(core.get() == 7.0)
