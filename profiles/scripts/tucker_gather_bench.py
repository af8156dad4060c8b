"""Times the evaluation of a resident Tucker tensor at an index list, ttsk_tucker_gather against its composition (column
gathers and batched ``contract`` calls, tensor_gather._tucker_gather_composed), in one process with device events on
library stream 0.

  gather     tucker.gather_dev(sparse): the (N,) values
  dot        sparse.dot(tucker): the three sums only, one read-back

each under route="kernel" and route="composed".  The kernel's figures are set against the fp64 matrix pipe: 2 |C| N flops
over 78.6 TF/s.  The variants are alternated, REPS timed repetitions after WARM warm-up rounds; median
and spread (min .. max).

    python profiles/scripts/tucker_gather_bench.py [--json profiles/tucker_gather_bench.json] [--reps 7]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from tt_sketch_amd import SparseTensor, TuckerTensor, _native as nat
from tt_sketch_amd.device import DevArray

WARM = 1
PIPE_TFLOPS = 78.6          # v_mfma_f64_16x16x4 over 256 CUs

# d, n, rank, N
SHAPES = [(3, 200, 16, 10 ** 6), (3, 200, 16, 10 ** 7), (5, 200, 4, 10 ** 7), (3, 200, 32, 10 ** 6)]


def timed(fn):
    nat.call("ttsk_timer_start", 0)
    fn()
    ms = ctypes.c_float()
    nat.call("ttsk_timer_stop", 0, ctypes.byref(ms))
    return float(ms.value)


def measure(variants, reps):
    times = {k: [] for k, _ in variants}
    for rep in range(WARM + reps):
        for k, fn in variants:
            ms = timed(fn)
            if rep >= WARM:
                times[k].append(ms)
    out = {}
    for k, _ in variants:
        t = np.array(times[k])
        out[k] = [float(np.median(t)), float(t.min()), float(t.max())]
        print(f"  {k:16s} median {np.median(t):10.4f} ms  (min {t.min():.4f} .. max {t.max():.4f}, {len(t)} reps)")
    return out


def case(d, n, r, N, reps):
    rng = np.random.default_rng(N + r)
    factors = [DevArray.from_host(rng.standard_normal((r, n)) / np.sqrt(n)) for _ in range(d)]
    a = TuckerTensor(factors, DevArray.from_host(rng.standard_normal((r,) * d)))
    idx = np.stack([rng.integers(0, n, N) for _ in range(d)]).astype(np.int64)
    sp = SparseTensor((n,) * d, idx, rng.standard_normal(N))
    sp.prepare_device()
    got = {}

    def gather(route):
        def run():
            got["gather " + route] = a.gather_dev(sp, route=route)
        return run

    def dot(route):
        def run():
            got["dot " + route] = sp.dot(a, route=route)
        return run

    flops = 2.0 * float(r) ** d * N
    print(f"\nd = {d}, n = {n}, ranks {r}, N = {N}: {flops / 1e9:.2f} GF, roof {flops / (PIPE_TFLOPS * 1e9):.4f} ms")
    ms = measure([(f"{what} {route}", fn(route)) for what, fn in (("gather", gather), ("dot", dot)) for route in ("kernel", "composed")], reps)
    gap = abs(got["dot kernel"] - got["dot composed"]) / abs(got["dot composed"])
    rec = dict(d=d, n=n, rank=r, N=N, reps=reps, flops=flops, ms=ms, rel_gap_routes=gap,
               of_matrix_peak={k: flops / (PIPE_TFLOPS * 1e9) / ms[k][0] for k in ("gather kernel", "dot kernel")},
               kernel_over_composed={w: ms[w + " kernel"][0] / ms[w + " composed"][0] for w in ("gather", "dot")})
    print(f"  kernel at {100 * rec['of_matrix_peak']['gather kernel']:.1f} % (gather), {100 * rec['of_matrix_peak']['dot kernel']:.1f} % (dot) of the matrix peak; "
          f"kernel / composed {rec['kernel_over_composed']}; routes differ by {gap:.1e}")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    nat.call("ttsk_init", 0)
    recs = [case(d, n, r, N, args.reps) for d, n, r, N in SHAPES]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(cases=recs, pipe_tflops=PIPE_TFLOPS, warm=WARM), f, indent=1)


if __name__ == "__main__":
    main()
