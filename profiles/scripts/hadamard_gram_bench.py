"""Times the inner products of entrywise products of two tensor trains that are never formed (hadamard_gram.py,
ttsk_hadamard_close) in one process, with device events on library stream 0.

Step B alone, G' (P, S' s') from Wl (S s, n, P) of one interior mode with P = R' r' (B1 .. B4, the shapes H1 .. H4 of
hadamard_sketch_bench.py with u = x and v = y; B4 at the 42 values of i that W_BUDGET_BYTES makes of n = 200):

  kernel     hadamard_close(..., route="kernel"): one ttsk_hadamard_close call (T1 stays on the chip, nothing indexed by i
             is written) and the ttsk_sum_slices behind it
  composed   hadamard_close(..., route="composed"): a transposed copy of Wl, two `contract` calls with T1 (n, S, P, s')
             through HBM, and a strided copy that puts p first

End to end, ||x o y||^2 = h.dot(h) and z.error(h, fast=True) for a train z (E1 .. E3):

  rule       half B as the routing rule of hadamard_gram.close_route_ms has it
  kernel     the same with ttsk_hadamard_close at every mode (paths.forced("kernel"), which forces half A too)
  composed   the same with the compositions at every mode
  explicit   as a user of the parent commit would write it: the Kronecker cores formed on resident cores
             (HadamardProduct.to_tt), then the existing chain on that train (tt.dot(tt), z.error(tt, fast=True)); the
             formation is inside the timed region

The variants are alternated, REPS timed repetitions after WARM warm-up rounds; median and spread (min .. max).  A timed
region of step B alone holds INNER calls, so that it is not the clock that is measured; the figure is per call.  After
the timing the routes are compared on the same operands, and lazy against explicit.

    python profiles/scripts/hadamard_gram_bench.py [--json out.json] [--cases B1,B2,B3,B4,E1,E2,E3] [--reps 9]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from tt_sketch_amd import HadamardProduct, TensorTrain, paths, _native as nat
from tt_sketch_amd import hadamard_gram as hg
from tt_sketch_amd.device import DevArray

WARM = 2


def timed(fn, inner=1):
    nat.call("ttsk_timer_start", 0)
    for _ in range(inner):
        fn()
    ms = ctypes.c_float()
    nat.call("ttsk_timer_stop", 0, ctypes.byref(ms))
    return float(ms.value) / inner


def measure(variants, reps, inner=1):
    times = {k: [] for k, _ in variants}
    for rep in range(WARM + reps):
        for k, fn in variants:
            ms = timed(fn, inner)
            if rep >= WARM:
                times[k].append(ms)
    out = {}
    for k, _ in variants:
        t = np.array(times[k])
        out[k] = [float(np.median(t)), float(t.min()), float(t.max())]
        print(f"  {k:9s} median {np.median(t):9.4f} ms  (min {t.min():.4f} .. max {t.max():.4f}, {len(t)} reps)", flush=True)
    return out


def apart(a, b):
    return bool(a[2] < b[1] or b[2] < a[1])


def normal(shape, seed, scale=1.0):
    """standard normals made on the device: the largest operand here is 2 GB"""
    a = DevArray.empty(shape)
    nat.call("ttsk_fill_normal", a, a.size, seed, float(scale), 0)
    return a


def close_case(name, S, s, n, reps, inner):
    P = S * s
    Wl = normal((S * s, n, P), 1, 1.0 / np.sqrt(S * s))
    U, V = normal((S, n, S), 2), normal((s, n, s), 3)
    got = {}

    def kernel():
        got["kernel"] = hg.hadamard_close(Wl, U, V, route="kernel")

    def composed():
        got["composed"] = hg.hadamard_close(Wl, U, V, route="composed")

    fl = 2.0 * n * P * (S * s * s + S * S * s)
    ichunks, slab = hg.close_layout(S, S, s, s, n, P)
    print(f"\n({name}) step B alone: S = {S}, s = {s}, n = {n}, P = {P}: {fl / 1e9:.3f} GF, Wl of {S * s * n * P * 8 / 1e6:.1f} MB, "
          f"{ichunks} chunks of i, a slab of {slab * 8 / 1e6:.1f} MB", flush=True)
    ms = measure([("kernel", kernel), ("composed", composed)], reps, inner)
    a, b = got["kernel"].get().ravel(), got["composed"].get().ravel()
    model = hg.close_route_ms(S, S, s, s, n, P)
    k, c = ms["kernel"], ms["composed"]
    rec = dict(case=name, S=S, S1=S, s=s, s1=s, n=n, P=P, flops=fl, ichunks=ichunks, kernel_ms=k, composed_ms=c, apart=apart(k, c),
               faster="kernel" if k[0] < c[0] else "composed", kernel_tflops=fl / k[0] / 1e9, composed_tflops=fl / c[0] / 1e9,
               max_rel_gap=float(np.max(np.abs(a - b)) / np.max(np.abs(b))), model_ms=dict(kernel=model[0], composed=model[1]),
               route="composed" if model[1] < model[0] else "kernel", reps=reps, inner=inner)
    print(f"  kernel {rec['kernel_tflops']:.2f} TF/s, composed {rec['composed_tflops']:.2f} TF/s; composed / kernel = {c[0] / k[0]:.2f}, "
          f"ranges apart: {rec['apart']}; largest gap {rec['max_rel_gap']:.1e}; rule: kernel {model[0]:.3f} ms, composed {model[1]:.3f} ms -> {rec['route']}",
          flush=True)
    return rec


def random_tt(seed, shape, r):
    rk = (1,) + (r,) * (len(shape) - 1) + (1,)
    return TensorTrain([normal((rk[k], n, rk[k + 1]), seed + k, 1.0 / np.sqrt(rk[k])) for k, n in enumerate(shape)])


def gram_case(name, shape, R, r, z_rank, reps):
    x, y, z = random_tt(10, shape, R), random_tt(30, shape, r), random_tt(50, shape, z_rank)
    h = HadamardProduct(x, y)
    core_gb = (R * r) ** 2 * max(shape) * 8 / 1e9
    print(f"\n({name}) shape {shape}, ranks {R} x {r}: product rank {R * r}, an explicit core {core_gb:.2f} GB; z of rank {z_rank}", flush=True)
    rec = dict(case=name, shape=list(shape), R=R, r=r, z_rank=z_rank, explicit_core_gb=core_gb, reps=reps)
    for what, lazy, explicit in (("norm2", lambda: h.dot(h), lambda: (lambda tt: tt.dot(tt))(h.to_tt())),
                                 ("error", lambda: z.error(h, fast=True), lambda: z.error(h.to_tt(), fast=True))):
        def routed(route, fn=lazy):
            def run():
                with paths.forced(route):
                    return fn()
            return run
        print(f" {what}:", flush=True)
        ms = measure([("rule", routed(None)), ("kernel", routed("kernel")), ("composed", routed("composed")), ("explicit", explicit)], reps)
        with paths.forced("kernel"):
            a = lazy()
        with paths.forced("composed"):
            b = lazy()
        c = explicit()
        rec[what] = dict(ms=ms, value=a, rel_diff_routes=abs(a - b) / abs(a), rel_diff_explicit=abs(a - c) / abs(c),
                         speedup_rule_over_explicit=ms["explicit"][0] / ms["rule"][0], apart_rule_explicit=apart(ms["rule"], ms["explicit"]))
        print(f"  explicit / rule = {rec[what]['speedup_rule_over_explicit']:.2f}, ranges apart: {rec[what]['apart_rule_explicit']}; kernel against "
              f"composed {rec[what]['rel_diff_routes']:.1e}, lazy against explicit {rec[what]['rel_diff_explicit']:.1e}", flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--cases", default="B1,B2,B3,B4,E1,E2,E3")
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    nat.call("ttsk_init", 0)
    cases = args.cases.split(",")
    alone, whole = [], []
    b4_n = hg._slices(200, 2500 * 2500)[0][1]
    for name, S, s, n, inner in (("B1", 20, 20, 20, 10), ("B2", 8, 64, 100, 5), ("B3", 32, 32, 200, 1), ("B4", 50, 50, b4_n, 1)):
        if name in cases:
            alone.append(close_case(name, S, s, n, args.reps, inner))
    for name, shape, R, r, zr in (("E1", (20,) * 8, 20, 20, 20), ("E2", (100,) * 6, 8, 64, 50), ("E3", (200,) * 6, 32, 32, 50)):
        if name in cases:
            whole.append(gram_case(name, shape, R, r, zr, args.reps))
    if args.json:
        rule = dict(floor_ms=hg._CLOSE_FLOOR_MS, kernel_tflops=hg._CLOSE_TFLOPS, launch_ms=hg._CLOSE_LAUNCH_MS,
                    composed_launches=hg._CLOSE_COMPOSED_LAUNCHES, gemm_tflops=hg._CLOSE_GEMM_TFLOPS,
                    w_budget_bytes=hg.W_BUDGET_BYTES)
        with open(args.json, "w") as f:
            json.dump(dict(close_alone=alone, end_to_end=whole, rule_when_run=rule), f, indent=1)


if __name__ == "__main__":
    main()
