"""Times the Gaussian sketch of the C2 tensor of bench.py (dense, d = 5, n = 64, 8.59 GB, l = 20, r = 40) with stored
matrices (DenseGaussianDRM) against matrices that are never stored (LazyGaussianDRM: ttsk_gauss_lazy_left / _right), and
each of the two kernels alone against the `contract` on the stored matrix it replaces, at the shapes the C2 sketch calls them with.

One process, the tensor resident, device events on the library stream (ttsk_timer_start / ttsk_timer_stop), the variants
alternated, medians with min and max.  A sketch is timed twice per variant: with the DRMs built beforehand, and with their
construction inside the timed region (for the stored class: the fill of 8.2 GB of matrices; for the lazy one: nothing).
Peak device bytes: the largest sum of live DevArray buffers (device._Buffer, pool classes) during a sketch, the tensor included;
the library's own scratch arenas are not in it.

    python profiles/scripts/gauss_lazy_bench.py [--json profiles/gauss_lazy_bench.json] [--n 64] [--reps 7]
"""
import argparse
import ctypes
import gc
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

import tt_sketch_amd as tsa
import tt_sketch_amd.device as dev
from tt_sketch_amd import _native as nat
from tt_sketch_amd.device import DevArray, contract
from tt_sketch_amd.sketching_methods import dense_sketch
from tt_sketch_amd.utils import random_normal_dev

L_RANK, R_RANK, D = 20, 40, 5
live = dict(now=0, peak=0)


class TrackedBuffer(dev._Buffer):
    __slots__ = ()

    def __init__(self, nbytes, stream=0):
        super().__init__(nbytes, stream)
        live["now"] += self._pooled
        live["peak"] = max(live["peak"], live["now"])

    def __del__(self):
        if self.ptr:
            live["now"] -= self._pooled
        super().__del__()


def timed(fn):
    nat.call("ttsk_timer_start", 0)
    keep = fn()
    ms = ctypes.c_float()
    nat.call("ttsk_timer_stop", 0, ctypes.byref(ms))
    del keep
    return float(ms.value)


def stats(t):
    t = np.array(t)
    return dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), reps=len(t))


def alternate(legs, reps, warm=2):
    times = {k: [] for k in legs}
    for _ in range(warm):
        for fn in legs.values():
            timed(fn)
    for _ in range(reps):
        for k, fn in legs.items():
            times[k].append(timed(fn))
    return {k: stats(v) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    nat.call("ttsk_init", 0)
    dev._Buffer = TrackedBuffer
    n, shape = args.n, (args.n,) * D
    X = random_normal_dev(shape, seed=2)
    T = tsa.DenseTensor(X)
    rec = dict(shape=list(shape), l=L_RANK, r=R_RANK, tensor_bytes=8 * n ** D)
    streaming = tsa.SketchMethod.streaming
    classes = dict(stored=tsa.DenseGaussianDRM, lazy=tsa.LazyGaussianDRM)

    # ---- whole sketches, DRMs pre-built
    drms = {k: (cls(L_RANK, shape, False, seed=1), cls(R_RANK, shape, True, seed=2)) for k, cls in classes.items()}
    rec["sketch_prebuilt"] = alternate({k: (lambda p=p: tsa.general_sketch(T, p[0], p[1], streaming)) for k, p in drms.items()}, args.reps)
    peaks = {}
    for k, p in drms.items():
        gc.collect()
        live["peak"] = live["now"]
        tsa.general_sketch(T, p[0], p[1], streaming)
        dev.sync()
        peaks[k] = dict(peak_bytes=live["peak"], resident_before_bytes=live["now"])
    rec["peak_device_bytes"] = peaks
    print("sketch, DRMs pre-built:", rec["sketch_prebuilt"], flush=True)
    print("peak bytes:", peaks, flush=True)

    # ---- the kernels alone, on the stored matrices of the pre-built DRMs
    (sl, sr), (ll, lr) = drms["stored"], drms["lazy"]
    kernels = {}
    for mu in range(D - 1):
        A, G = sl._mat(mu), ll.sketching_mats[mu]
        Xu = X.reshape(n ** (mu + 1), n ** (D - 1 - mu))
        res = alternate({"contract": lambda: contract("ip,pq->iq", A, Xu), "lazy": lambda: dense_sketch._lazy_left(G, Xu)}, args.reps)
        kernels["left level %d: (%d x %d) (%d x %d)" % (mu, L_RANK, Xu.shape[0], Xu.shape[0], Xu.shape[1])] = res
        print("left", mu, res, flush=True)
    # right: Psi_0 multiplies the tensor's first unfolding; the later levels multiply a left product (l n, n^(d - mu - 1))
    mats_r, recipes_r = list(sr.sketch_dense(T)), list(lr.sketch_dense(T))
    for mu in range(D - 1):
        rows = n if mu == 0 else L_RANK * n
        cols = n ** (D - 1 - mu)
        S = X.reshape(n, -1) if mu == 0 else random_normal_dev((rows, cols), seed=50 + mu)
        B, G = mats_r[mu], recipes_r[mu]
        assert tuple(B.shape) == tuple(G.shape) == (R_RANK, cols)
        res = alternate({"contract": lambda: contract("bq,mq->bm", S, B), "lazy": lambda: dense_sketch._lazy_right(S, G)}, args.reps)
        kernels["right level %d: (%d x %d) (%d x %d)^T" % (mu, rows, cols, R_RANK, cols)] = res
        print("right", mu, res, flush=True)
        del S
    rec["kernels_alone"] = kernels
    del drms, sl, sr, ll, lr, mats_r, recipes_r, A, B, G
    gc.collect()
    dev.release_cached()

    # ---- whole sketches, the construction of the DRMs inside the timed region
    def with_construction(cls):
        def run():
            left, right = cls(L_RANK, shape, False, seed=1), cls(R_RANK, shape, True, seed=2)
            return tsa.general_sketch(T, left, right, streaming)
        return run
    rec["sketch_with_construction"] = alternate({k: with_construction(cls) for k, cls in classes.items()}, args.reps)
    print("sketch with DRM construction:", rec["sketch_with_construction"], flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
