"""The levelled fused chain step (csrc/chain_deal.h, csrc/chain_fused.h) through ttsk_chain_step: TT ranks J beyond four
row tiles, where row tiles are cut by DRM-rank range over two waves and a last row tile of at most 4 rows runs as a
4x4x4 piece, against the two einsums of TensorTrainDRM.sketch_tt (tensor_train_drm.py:81-87) as
test_gpu_parity.test_fused_chain_step_against_einsum forms them, at that file's TOL.  Results differ from the uncut
kernel in summation order only."""
import ctypes
import itertools

import numpy as np
import pytest

from tests.golden_io import rel
from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = 1e-12      # test_gpu_parity.TOL

JS = (65, 80, 96, 97, 100, 112)
RANKS = ((100, 100), (50, 50), (52, 50), (112, 112))
# (nb, n, K1): a batch of 32 has 8 workgroups per tensor on 256 CUs, a single tensor one workgroup per CU: neither
# divides n (unequal slice ranges of 2 or 3 slices: a levelled workgroup needs two); K1 = 100 runs phase A as one run of 25 k-blocks, K1 = 52 as runs of 5
BATCHES = ((32, 19, 100), (1, 600, 52))
# (rank 112 with K1 = 100 is beyond the kernel's LDS: its two images fit up to K1 = 60, the K1 of the rank-112 case of
# test_fused_chain_step_against_einsum)
CASES = [(seed, J, A, A2, wt, right, nb, n, min(K1, 60) if A == 112 else K1) for seed, (J, (A, A2), wt, right, (nb, n, K1)) in
         enumerate(itertools.product(JS, RANKS, (False, True), (False, True), BATCHES))]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "s%d-J%d-A%d-%d-%s-%s-nb%d" % (c[0], c[1], c[2], c[3], "T" if c[4] else "noT",
                                                                                     "right" if c[5] else "left", c[6]))
def test_levelled_chain_step_against_einsum(tsa, case):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray, sync
    seed, J, A, A2, wt, right, nb, n, K1 = case
    rng = np.random.default_rng(seed)
    W = [rng.standard_normal((K1, A)) for _ in range(nb)]
    E = rng.standard_normal((A, n, A2))
    if right:      # X[j][k][c]
        X = [rng.standard_normal((J, n, K1)) for _ in range(nb)]
        strides = (n * K1, K1, 1)
        want_T = [np.einsum("ca,jkc->akj", w, x) for w, x in zip(W, X)]
    else:          # X[c][k][j]
        X = [rng.standard_normal((K1, n, J)) for _ in range(nb)]
        strides = (1, J, n * J)
        want_T = [np.einsum("ca,ckj->akj", w, x) for w, x in zip(W, X)]
    want = [np.einsum("akj,akb->jb", t, E) for t in want_T]
    dW, dX = [DevArray.from_host(w) for w in W], [DevArray.from_host(x) for x in X]
    dE = DevArray.from_host(E)
    dO = [DevArray.from_host(np.full((J, A2), np.nan)) for _ in range(nb)]
    dT = [DevArray.from_host(np.full((A, n, J), np.nan)) for _ in range(nb)] if wt else None
    P = ctypes.c_void_p
    arr = lambda xs: (P * nb)(*[x.ptr for x in xs])
    nat.call("ttsk_chain_step", nb, n, K1, A, A2, J, arr(dW), A, arr(dX), strides[0], strides[1], strides[2],
             X[0].size, P(dE.ptr), arr(dT) if wt else None, arr(dO), 0)
    sync()
    for b in range(nb):
        got = dO[b].get()
        err = rel(got, want[b])
        print("tensor", b, "Out", err)
        assert not np.isnan(got).any(), (b, "output element never written")
        assert err < TOL, (b, err)
        if wt:
            got_T = dT[b].get()
            # a row of a that the deal skipped would still hold its fill value
            assert not np.isnan(got_T).any(), (b, "T element never written", np.argwhere(np.isnan(got_T))[:4])
            err = rel(got_T, want_T[b])
            print("tensor", b, "T", err)
            assert err < TOL, (b, err)
