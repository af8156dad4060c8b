"""Times the inner products with a CP tensor (ttsk_cp_gram, the <tt, cp> chain on ttsk_cp_chain_step, and
error(fast=True) built on them) in one process, with device events on library stream 0.

cp_gram alone, d = 8, n = 12, at N = 100 (plot_cp_tensor.py) and N = 25 000 (plot_cp_forest.py):

  sym        cp_gram(a): the tiles on and above the diagonal
  unsym      cp_gram(a, b) with a second CP tensor of the same rank
  host       the same sum by NumPy on the host: np.prod over the modes of A_k^T B_k, in column slabs so that it fits, at the
             BLAS thread count bench.py uses for its CPU leg; wall clock, ONE run (seconds at N = 25 000)

Each device figure is set against the kernel's matrix-pipe roof, flops / 77.7 TF/s, with the flops of
the plan: 2 N M sum n_k, and N (N + 1) sum n_k for sym.

<tt, cp> at train ranks 30 and 50 at those shapes: the routing rule, ttsk_cp_chain_step at every step, the composition at
every step.  tt.error(cp, fast=True, relative=True) end to end (the QR sweep of tt.norm(), cp.norm(), the chain, three
read-backs).

The variants are alternated, REPS timed repetitions after WARM warm-up rounds; median and spread (min .. max).

    python profiles/scripts/cp_gram_bench.py [--json profiles/cp_gram_bench.json] [--reps 15] [--no-host]
"""
import argparse
import contextlib
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from tt_sketch_amd import CPTensor, TensorTrain, cp_gram, _native as nat
from tt_sketch_amd.device import DevArray

WARM = 2
PIPE_TFLOPS = 77.7          # v_mfma_f64_16x16x4 at 2.4 GHz over 256 CUs
CPU_THREADS = 16            # bench.py: CPU_THREADS
SLAB_BYTES = 256 << 20      # host leg: one (N x slab) block of A_k^T B_k and the running product stay below this each


def blas_threads(n=CPU_THREADS):
    try:
        from threadpoolctl import threadpool_limits
        return threadpool_limits(limits=n)
    except Exception:
        return contextlib.nullcontext()


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
        print(f"  {k:9s} median {np.median(t):9.4f} ms  (min {t.min():.4f} .. max {t.max():.4f}, {len(t)} reps)")
    return out


def host_gram(A, B):
    """sum of np.prod_k (A_k^T B_k) in column slabs"""
    N, M = A[0].shape[1], B[0].shape[1]
    slab = max(1, min(M, SLAB_BYTES // (8 * N)))
    total = 0.0
    for lo in range(0, M, slab):
        P = None
        for a, b in zip(A, B):
            g = a.T @ b[:, lo:lo + slab]
            P = g if P is None else np.multiply(P, g, out=P)
        total += float(P.sum())
    return total


def gram_case(N, d, n, reps, host):
    rng = np.random.default_rng(N)
    A = [rng.standard_normal((n, N)) / np.sqrt(n) for _ in range(d)]
    B = [rng.standard_normal((n, N)) / np.sqrt(n) for _ in range(d)]
    a, b = CPTensor([DevArray.from_host(f) for f in A]), CPTensor([DevArray.from_host(f) for f in B])
    got = {}

    def sym():
        got["sym"] = cp_gram(a)

    def unsym():
        got["unsym"] = cp_gram(a, b)

    fl = dict(sym=float(N) * (N + 1) * d * n, unsym=2.0 * N * N * d * n)
    print(f"\ncp_gram: d = {d}, n = {n}, N = {N}: {fl['unsym'] / 1e9:.3f} GF unsymmetric; a dense operand would be {float(n) ** d * 8 / 1e9:.2f} GB")
    ms = measure([("sym", sym), ("unsym", unsym)], reps)
    rec = dict(N=N, d=d, n=n, reps=reps, flops=fl, ms=ms, roof_ms={k: v / (PIPE_TFLOPS * 1e9) for k, v in fl.items()},
               tflops={k: fl[k] / ms[k][0] / 1e9 for k in fl}, of_roof={k: fl[k] / (PIPE_TFLOPS * 1e9) / ms[k][0] for k in fl})
    for k in fl:
        print(f"  {k}: {rec['tflops'][k]:.2f} TF/s, {100 * rec['of_roof'][k]:.1f} % of the matrix pipe's {rec['roof_ms'][k]:.4f} ms")
    if host:
        with blas_threads():
            t0 = time.perf_counter()
            ref = host_gram(A, B)
            rec["host_unsym_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            ref_sym = host_gram(A, A)
            rec["host_sym_s"] = time.perf_counter() - t0
        rec["host_threads"] = CPU_THREADS
        rec["rel_gap_to_host"] = dict(unsym=abs(got["unsym"] - ref) / abs(ref), sym=abs(got["sym"] - ref_sym) / abs(ref_sym))
        print(f"  host NumPy ({CPU_THREADS} BLAS threads, one run): unsym {rec['host_unsym_s']:.3f} s, sym (the full sum) {rec['host_sym_s']:.3f} s; "
              f"device against host: {rec['rel_gap_to_host']}")
    else:
        rec["host"] = "not recorded yet"
    return rec


def dot_case(N, d, n, r, reps):
    rng = np.random.default_rng(N + r)
    rk = (1,) + (r,) * (d - 1) + (1,)
    tt = TensorTrain([DevArray.from_host(rng.standard_normal((rk[k], n, rk[k + 1])) / np.sqrt(rk[k] * n)) for k in range(d)])
    cp = CPTensor([DevArray.from_host(rng.standard_normal((n, N)) / np.sqrt(n)) for _ in range(d)])
    got = {}

    def routed(route):
        def run():
            got[route] = tt.dot(cp, route=route)
        return run

    def error():
        got["error"] = tt.error(cp, fast=True, relative=True)

    print(f"\n<tt, cp>: d = {d}, n = {n}, train rank {r}, N = {N}")
    ms = measure([("rule", routed(None)), ("kernel", routed("kernel")), ("composed", routed("composed")), ("error", error)], reps)
    gap = abs(got["kernel"] - got["composed"]) / abs(got["composed"])
    print(f"  kernel against composed: {gap:.1e}; error(fast=True, relative=True) = {got['error']:.6f}")
    return dict(N=N, d=d, n=n, rank=r, reps=reps, ms=ms, rel_gap_routes=gap, error=got["error"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    nat.call("ttsk_init", 0)
    d, n = 8, 12
    grams = [gram_case(N, d, n, args.reps, not args.no_host) for N in (100, 25_000)]
    dots = [dot_case(N, d, n, r, args.reps) for N in (100, 25_000) for r in (30, 50)]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(cp_gram=grams, tt_dot_cp=dots, pipe_tflops=PIPE_TFLOPS, warm=WARM), f, indent=1)


if __name__ == "__main__":
    main()
