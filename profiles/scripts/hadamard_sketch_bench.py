"""Times the sketch of entrywise products of two tensor trains that are never formed (HadamardProduct,
ttsk_hadamard_apply) in one process, with device events on library stream 0.

hadamard_apply alone, W (l, n, R' r') of one interior mode (H1 .. H4):

  kernel     hadamard_apply(..., route="kernel"): one ttsk_hadamard_apply call (T1 stays on the chip)
  composed   hadamard_apply(..., route="composed"): a transposed copy of L, two `contract` calls with T1 (n, R, l, r')
             through HBM, and a strided copy that puts l first

End to end, stream_sketch(HadamardProduct(x, y), ...).to_tt() (E1 .. E4):

  rule       hadamard_fused with W as the routing rule of hadamard_product.route_ms has it
  kernel     the same with ttsk_hadamard_apply at every step (paths.forced("kernel"))
  composed   the same with the composition at every step
  explicit   as a user of the parent commit would write it: the Kronecker cores formed on resident cores
             (HadamardProduct.to_tt), then the same sketch of that train; the formation is inside the timed region.
             Not run where the explicit cores do not fit (E4: 2500 x 200 x 2500 doubles are 10 GB each).

The variants are alternated, REPS timed repetitions after WARM warm-up rounds; median and spread (min .. max).  A timed
region of hadamard_apply alone holds INNER calls, so that it is not the clock that is measured; the figure is per call.
After the timing the routes are compared on the same operands, and lazy and explicit with the same seeded DRMs.

    python profiles/scripts/hadamard_sketch_bench.py [--json out.json] [--cases H1,H2,H3,H4,E1,E2,E3,E4] [--reps 15]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from tt_sketch_amd import HadamardProduct, TensorTrain, paths, stream_sketch, _native as nat
from tt_sketch_amd import hadamard_product as hp
from tt_sketch_amd.device import DevArray
from tt_sketch_amd.utils import process_tt_rank

WARM = 2
INNER = 10


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
        print(f"  {k:9s} median {np.median(t):9.4f} ms  (min {t.min():.4f} .. max {t.max():.4f}, {len(t)} reps)")
    return out


def apart(a, b):
    return bool(a[2] < b[1] or b[2] < a[1])


def kernel_case(name, R, r, n, l, reps):
    rng = np.random.default_rng(l + R)
    L = DevArray.from_host(rng.standard_normal((R, r, l)))
    X = DevArray.from_host(rng.standard_normal((R, n, R)))
    Y = DevArray.from_host(rng.standard_normal((r, n, r)))
    got = {}

    def kernel():
        got["kernel"] = hp.hadamard_apply(L, X, Y, route="kernel")

    def composed():
        got["composed"] = hp.hadamard_apply(L, X, Y, route="composed")

    fl = 2.0 * l * n * (R * r * r + R * R * r)
    print(f"\n({name}) hadamard_apply alone: R = {R}, r = {r}, n = {n}, l = {l}: {fl / 1e9:.4f} GF, W of {l * n * R * r * 8 / 1e6:.1f} MB")
    ms = measure([("kernel", kernel), ("composed", composed)], reps, INNER)
    a, b = got["kernel"].get().ravel(), got["composed"].get().ravel()
    model = hp.route_ms(R, R, r, r, n, l)
    k, c = ms["kernel"], ms["composed"]
    rec = dict(case=name, R=R, R1=R, r=r, r1=r, n=n, l=l, flops=fl, kernel_ms=k, composed_ms=c, apart=apart(k, c),
               faster="kernel" if k[0] < c[0] else "composed", kernel_tflops=fl / k[0] / 1e9, composed_tflops=fl / c[0] / 1e9,
               max_rel_gap=float(np.max(np.abs(a - b)) / np.max(np.abs(b))), model_ms=dict(kernel=model[0], composed=model[1]),
               route="composed" if model[1] < model[0] else "kernel", reps=reps, inner=INNER)
    print(f"  kernel {rec['kernel_tflops']:.2f} TF/s, composed {rec['composed_tflops']:.2f} TF/s; composed / kernel = {c[0] / k[0]:.2f}, "
          f"ranges apart: {rec['apart']}; largest gap {rec['max_rel_gap']:.1e}; rule: kernel {model[0]:.3f} ms, composed {model[1]:.3f} ms -> {rec['route']}")
    return rec


def random_tt(rng, shape, r):
    rk = (1,) + (r,) * (len(shape) - 1) + (1,)
    return TensorTrain([DevArray.from_host(rng.standard_normal((rk[k], n, rk[k + 1])) / np.sqrt(rk[k] * n)) for k, n in enumerate(shape)])


def sketch_case(name, shape, R, r, left_rank, right_rank, reps, with_explicit=True):
    rng = np.random.default_rng(len(shape) + R)
    x, y = random_tt(rng, shape, R), random_tt(rng, shape, r)
    h = HadamardProduct(x, y)
    lr = process_tt_rank(left_rank, shape, trim=True)
    rr = process_tt_rank(right_rank, shape, trim=False)

    def routed(route):
        def run():
            with paths.forced(route):
                return stream_sketch(h, left_rank=lr, right_rank=rr).to_tt()
        return run

    def explicit():
        return stream_sketch(h.to_tt(), left_rank=lr, right_rank=rr).to_tt()

    core_gb = (R * r) ** 2 * max(shape) * 8 / 1e9
    print(f"\n({name}) shape {shape}, ranks {R} x {r}: product rank {R * r}, an explicit core {core_gb:.2f} GB; sketch ranks {left_rank} / {right_rank}")
    variants = [("rule", routed(None)), ("kernel", routed("kernel")), ("composed", routed("composed"))]
    if with_explicit:
        variants.append(("explicit", explicit))
    ms = measure(variants, reps)
    rec = dict(case=name, shape=list(shape), R=R, r=r, left_rank=left_rank, right_rank=right_rank, ms=ms, reps=reps,
               explicit_core_gb=core_gb, explicit="timed" if with_explicit else f"not run: the explicit cores are {core_gb:.0f} GB each")
    with paths.forced("kernel"):
        a = stream_sketch(h, left_rank=lr, right_rank=rr, seed=7).to_tt()
    with paths.forced("composed"):
        b = stream_sketch(h, left_rank=lr, right_rank=rr, seed=7).to_tt()
    rec["rel_diff_routes_same_drms"] = float(a.error(b, relative=True))
    if with_explicit:
        c = stream_sketch(h.to_tt(), left_rank=lr, right_rank=rr, seed=7).to_tt()
        rec["rel_diff_explicit_same_drms"] = float(a.error(c, relative=True))
        rec["speedup_rule_over_explicit"] = ms["explicit"][0] / ms["rule"][0]
        rec["apart_rule_explicit"] = apart(ms["rule"], ms["explicit"])
        print(f"  explicit / rule = {rec['speedup_rule_over_explicit']:.2f}, ranges apart: {rec['apart_rule_explicit']}; same DRMs: lazy against "
              f"explicit {rec['rel_diff_explicit_same_drms']:.1e}")
    print(f"  same DRMs: kernel against composed {rec['rel_diff_routes_same_drms']:.1e} of the norm")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--cases", default="H1,H2,H3,H4,E1,E2,E3,E4")
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    nat.call("ttsk_init", 0)
    cases = args.cases.split(",")
    alone, whole = [], []
    for name, R, r, n, l in (("H1", 20, 20, 20, 20), ("H2", 8, 64, 100, 50), ("H3", 32, 32, 200, 50), ("H4", 50, 50, 200, 50)):
        if name in cases:
            alone.append(kernel_case(name, R, r, n, l, args.reps))
    for name, shape, R, r, lk, rk, explicit in (("E1", (20,) * 8, 20, 20, 20, 40, True), ("E2", (100,) * 6, 8, 64, 50, 100, True),
                                                ("E3", (200,) * 6, 32, 32, 50, 100, True), ("E4", (200,) * 6, 50, 50, 50, 100, False)):
        if name in cases:
            whole.append(sketch_case(name, shape, R, r, lk, rk, args.reps, explicit))
    if args.json:
        rule = dict(kernel_floor_ms=hp._KERNEL_FLOOR_MS, kernel_tflops=hp._KERNEL_TFLOPS, launch_ms=hp._LAUNCH_MS,
                    composed_launches=hp._COMPOSED_LAUNCHES, gemm_tflops=hp._GEMM_TFLOPS)
        with open(args.json, "w") as f:
            json.dump(dict(kernel_alone=alone, end_to_end=whole, rule_when_run=rule), f, indent=1)


if __name__ == "__main__":
    main()
