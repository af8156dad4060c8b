"""ttsk_shutdown + ttsk_init on the same device, then the same calls again: every family that launches with more than
64 KiB of dynamic LDS must raise its limit anew in the new init generation (csrc/runtime.hip raise_lds_limit) and
compute bit-identical results.  The calls run in a child process under a time limit, so the library state of the
test session is left alone."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, %(root)r)
import tt_sketch_amd as tsa
from tt_sketch_amd import _native as nat, sparse_fused
from tt_sketch_amd.device import DevArray, as_dev, contract, sync
from tt_sketch_amd.drm import fast_lazy_gaussian as flg
from tt_sketch_amd.utils import right_mul_pinv

V = ctypes.c_void_p


def host(x):
    x = x.to_tt() if hasattr(x, "to_tt") else x
    return [np.array(c) for c in x.cores]


def chain(entry, case):
    # ttsk_chain_step / ttsk_chain_step_wide, as tests/test_gpu_parity.py drives them
    nb, n, K1, A, A2, J, right, wt = case
    rng = np.random.default_rng(7)
    W = [rng.standard_normal((K1, A)) for _ in range(nb)]
    E = rng.standard_normal((A, n, A2))
    shp, strides = ((J, n, K1), (n * K1, K1, 1)) if right else ((K1, n, J), (1, J, n * J))
    X = [rng.standard_normal(shp) for _ in range(nb)]
    dW, dX, dE = [as_dev(w) for w in W], [as_dev(x) for x in X], as_dev(E)
    dO = [DevArray.zeros((J, A2)) for _ in range(nb)]
    dT = [DevArray.zeros((A, n, J)) for _ in range(nb)] if wt else None
    arr = lambda xs: (V * nb)(*[x.ptr for x in xs])
    nat.call(entry, nb, n, K1, A, A2, J, arr(dW), A, arr(dX), strides[0], strides[1], strides[2], X[0].size, V(dE.ptr),
             arr(dT) if wt else None, arr(dO), 0)
    sync()
    return [o.get() for o in dO] + ([t.get() for t in dT] if wt else [])


def dense_first():
    rng = np.random.default_rng(3)
    n0, Q, T, ll, r = 64, 264, 64, 20, 41
    Xd, Cd, Pd = as_dev(rng.standard_normal((n0, Q, T))), as_dev(rng.standard_normal((n0, ll))), as_dev(rng.standard_normal((Q, r)))
    Z, U = DevArray.empty((ll, Q, T)), DevArray.empty((n0, r, T))
    nat.call("ttsk_dense_first_pass", V(Xd.ptr), n0, Q, T, V(Cd.ptr), ll, V(Pd.ptr), r, V(Z.ptr), V(U.ptr), 0)
    sync()
    return [Z.get(), U.get()]


def dense_left():
    rng = np.random.default_rng(4)
    n0, n1, n2, n3, n4, l = 64, 2, 8, 8, 64, 20
    X = rng.standard_normal((n0, n1, n2, n3, n4))
    A = [rng.standard_normal((l, int(np.prod(X.shape[:mu + 1])))) for mu in range(4)]
    C = n3 * n4
    Xd, A0 = as_dev(X), as_dev(A[0])
    A3 = as_dev(np.ascontiguousarray(A[3].reshape(l, n0, n1, n2, n3).transpose(0, 3, 2, 4, 1)))
    A1t = as_dev(np.ascontiguousarray(A[1].reshape(l, n0, n1).transpose(0, 2, 1)))
    A2t = as_dev(np.ascontiguousarray(A[2].reshape(l, n0, n1, n2).transpose(0, 3, 2, 1)))
    Z = [DevArray.empty(s) for s in ((l, n1 * n2 * C), (l, n2 * C), (l, C), (l, C))]
    nat.call("ttsk_dense_left_pass", V(Xd.ptr), n0, n1, n2, C, n4, l, V(A0.ptr), V(A1t.ptr), V(A2t.ptr), V(A3.ptr),
             *[V(z.ptr) for z in Z], 0)
    sync()
    return [z.get() for z in Z]


def gemm(spec, a_shape, b_shape, seed):
    rng = np.random.default_rng(seed)
    return [contract(spec, as_dev(rng.standard_normal(a_shape)), as_dev(rng.standard_normal(b_shape))).get()]


def sparse_pass():
    shape, nnz, l, r = (40, 30, 20, 25, 35), 20000, 24, 32
    rng = np.random.default_rng(nnz)
    idx = np.stack([rng.integers(0, n, nnz) for n in shape]).astype(np.int64)
    T = tsa.SparseTensor(shape, idx, rng.standard_normal(nnz))
    kw = lambda h: dict(rank_min=(0,) * 4, rank_max=(h,) * 4, true_rank=(h,) * 4)
    ld = tsa.SparseGaussianDRM((l,) * 4, shape, False, seed=3, **kw(l))
    rd = tsa.SparseGaussianDRM((r,) * 4, shape, True, seed=4, **kw(r))
    assert sparse_fused.try_sparse_gauss_sketch(T, ld, rd, tsa.SketchMethod.streaming) is not None
    sk = tsa.general_sketch(T, ld, rd, tsa.SketchMethod.streaming)
    return list(sk.Psi_cores) + list(sk.Omega_mats)


def sampler():
    rng = np.random.default_rng(5)
    shape = (50, 60, 70)
    idx = np.stack([rng.integers(0, n, 1003) for n in shape])
    return [flg.inds_to_normal(idx, shape, 3, 3 + w, 99) for w in (26, 32)]


def solves():
    rng = np.random.default_rng(3)
    out = []
    for m, n in [(1000, 50), (64, 64), (400, 12)]:
        M = rng.standard_normal((m, n)) if m != 400 else rng.standard_normal((m, 3)) @ rng.standard_normal((3, n))
        d = DevArray.from_host(M)
        nat.call("ttsk_qr_thin", V(d.ptr), m, n, 0)
        out.append(d.get())
    Om = (np.linalg.qr(rng.standard_normal((20, 20)))[0] * np.logspace(0, -4, 20)) @ rng.standard_normal((20, 35))
    out.append(np.array(right_mul_pinv(rng.standard_normal((15, 35)), Om)))          # Jacobi
    out.append(np.array(right_mul_pinv(rng.standard_normal((40, 100)), rng.standard_normal((50, 100)))))   # Cholesky
    return out


def sketches():
    out = []
    tt = tsa.TensorTrain.random((64, 64, 64, 64), 20, seed=1)
    out += host(tsa.stream_sketch(tt, 50, 100, seed=2))                                # chain_fused + to_tt
    terms = [tsa.TensorTrain.random((128,) * 4, 20, seed=10 + i) for i in range(6)]
    out += host(tsa.stream_sketch(tsa.TensorSum(terms), 50, 100, seed=5))              # chain_sum
    terms = [tsa.TensorTrain.random((70, 66, 68, 40), (52, 57, 49), seed=20 + i) for i in range(3)]
    out += host(tsa.stream_sketch(tsa.TensorSum(terms), (26, 28, 30), (54, 58, 70), seed=6))   # stream_small_sum
    out += host(tsa.orthogonal_sketch(tt, 50, 100, seed=7))                            # qr_signs
    sks = tsa.stream_sketch_batch([tsa.TensorTrain.random((13, 9, 11, 15), 13, seed=30 + i) for i in range(3)], 7, 11, seed=8)
    for t in tsa.to_tt_batch(sks):                                                     # assemble_batch
        out += host(t)
    return out


def run():
    out = chain("ttsk_chain_step", (2, 20, 64, 22, 22, 30, True, True))
    out += chain("ttsk_chain_step_wide", (2, 50, 100, 160, 160, 100, True, False))
    out += dense_first() + dense_left()
    out += gemm("mk,kn->mn", (5, 128), (128, 3000), 1)                               # skinny_s
    out += gemm("bq,mq->bm", (64, 8192), (40, 8192), 2)                              # rows_longk
    out += sparse_pass() + sampler() + solves() + sketches()
    return [np.array(x) for x in out]


nat.call("ttsk_init", 0)
first = run()
nat.call("ttsk_sync", -1)
nat.call("ttsk_shutdown")
nat.call("ttsk_init", 0)
again = run()
assert len(first) == len(again)
for i, (a, b) in enumerate(zip(first, again)):
    assert a.shape == b.shape and np.array_equal(a, b), i
print("REINIT-OK", len(first))
"""


def test_every_large_lds_family_after_shutdown_and_init():
    res = subprocess.run([sys.executable, "-c", CHILD % dict(root=ROOT)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "REINIT-OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
