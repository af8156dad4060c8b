"""Times the sketched rounding of operator-times-train products that are never formed (OperatorProduct, ttsk_op_apply)
against the explicit path it replaces, in one process and with device events on library stream 0:

  lazy       TTLinearMapSum(maps, lazy=True)(x) rounded by the streaming sketch: operator_fused, no product core anywhere;
             W from ttsk_op_apply or composed, as the routing rule of operator_product.op_apply has it
  lazy_k     the same sketch with ttsk_op_apply at every step (operator_fused.try_operator_sketch(..., route="kernel"))
  explicit   the same call as the parent commit makes it: MPO.__call__ forms every product, then the batched TT sketch;
             the product formation is inside the timed region

at two shapes:

  G1  a Krylov step of TT-GMRES: d = 8, n = 20, train ranks 20, three MPOs of rank 4, the sketch of round_tt_sum(max_rank=20,
      oversample_factor=2, method="sketch"): stream_sketch with ranks 20 / 40 (the smaller side trimmed), to_tt()
  G2  one wide product: d = 6, n = 100, ranks 64, one MPO of rank 8, stream_sketch with ranks 50 / 100, to_tt()

The MPOs hold host (NumPy) cores, as MPO.random and MPO.eye make them: they become resident at the first call, inside the
warm-up rounds, as in a GMRES run.  After the timing, lazy and explicit are sketched once more with the SAME seeded DRMs
and the relative difference of the two results is recorded.

And op_apply alone at an interior mode of both shapes, and for three terms of the larger one:

  kernel     op_apply(..., route="kernel"): one ttsk_op_apply call (T1 stays on the chip)
  composed   op_apply(..., route="composed"): W from two `contract` calls per term, T1 (R, l, n_in, r') through HBM, and
             with several terms one strided copy per term into its column block

The variants are alternated, REPS timed repetitions after WARM warm-up rounds; median and spread (min .. max).

    python profiles/scripts/operator_sketch_bench.py [--json out.json] [--cases G1,G2,K1,K2,K3] [--reps 15]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from tt_sketch_amd import SketchedTensorTrain, SketchContainer, SketchMethod, TensorTrain, TensorTrainDRM, stream_sketch, _native as nat
from tt_sketch_amd.device import DevArray
from tt_sketch_amd.operator_fused import try_operator_sketch
from tt_sketch_amd.operator_product import op_apply, route_ms
from tt_sketch_amd.tt_gmres import MPO, TTLinearMapSum
from tt_sketch_amd.utils import process_tt_rank

WARM = 2


def timed(fn):
    nat.call("ttsk_timer_start", 0)
    fn()
    ms = ctypes.c_float()
    nat.call("ttsk_timer_stop", 0, ctypes.byref(ms))
    return float(ms.value)


def measure(name, variants, reps):
    usable, failed = [], {}
    for k, fn in variants:                  # a variant the library refuses at this shape is reported, not timed
        try:
            fn()
            usable.append((k, fn))
        except Exception as e:              # noqa: BLE001
            failed[k] = f"{type(e).__name__}: {e}"
            print(f"  {k:9s} not available: {failed[k]}")
    variants = usable
    times = {k: [] for k, _ in variants}
    for rep in range(WARM + reps):
        for k, fn in variants:
            ms = timed(fn)
            if rep >= WARM:
                times[k].append(ms)
    rec = dict(case=name, ms={}, failed=failed)
    for k, _ in variants:
        t = np.array(times[k])
        rec["ms"][k] = dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()), reps=len(t))
        print(f"  {k:9s} median {np.median(t):9.3f} ms  (min {t.min():.3f} .. max {t.max():.3f}, {len(t)} reps)")
    return rec


def random_tt(rng, shape, r):
    rk = (1,) + (r,) * (len(shape) - 1) + (1,)
    return TensorTrain([DevArray.from_host(rng.standard_normal((rk[k], n, rk[k + 1])) / np.sqrt(rk[k] * n)) for k, n in enumerate(shape)])


def random_mpo(rng, shape, R):
    rk = (1,) + (R,) * (len(shape) - 1) + (1,)
    return MPO([rng.standard_normal((rk[k], n, n, rk[k + 1])) / np.sqrt(rk[k] * n) for k, n in enumerate(shape)])


def sketch_case(name, shape, r, R, n_maps, left_rank, right_rank, reps):
    rng = np.random.default_rng(len(shape))
    x = random_tt(rng, shape, r)
    maps = [random_mpo(rng, shape, R) for _ in range(n_maps)]
    A_lazy, A_explicit = TTLinearMapSum(maps, lazy=True), TTLinearMapSum(maps)
    lr = process_tt_rank(left_rank, shape, trim=True)
    rr = process_tt_rank(right_rank, shape, trim=False)

    def lazy():
        return stream_sketch(A_lazy(x), left_rank=lr, right_rank=rr).to_tt()

    def lazy_k():
        seed = int(rng.integers(1 << 30))
        left, right = TensorTrainDRM(lr, shape, transpose=False, seed=seed), TensorTrainDRM(rr, shape, transpose=True, seed=seed + 1)
        Psi, Om = try_operator_sketch(A_lazy(x), left, right, SketchMethod.streaming, route="kernel")
        return SketchedTensorTrain(SketchContainer(Psi, Om), left, right).to_tt()

    def explicit():
        return stream_sketch(A_explicit(x), left_rank=lr, right_rank=rr).to_tt()

    print(f"\n({name}) shape {shape}, train ranks {r}, {n_maps} MPO of rank {R}: product ranks {R * r}; sketch ranks {left_rank} / {right_rank}")
    rec = measure(name, [("lazy", lazy), ("lazy_k", lazy_k), ("explicit", explicit)], reps)
    rec.update(shape=shape, rank=r, op_rank=R, maps=n_maps, left_rank=left_rank, right_rank=right_rank)
    if rec["failed"]:
        return rec
    lo, hi = rec["ms"]["lazy"], rec["ms"]["explicit"]
    rec.update(speedup=hi["median"] / lo["median"], apart=bool(lo["max"] < hi["min"] or hi["max"] < lo["min"]))
    a = stream_sketch(A_lazy(x), left_rank=lr, right_rank=rr, seed=7).to_tt()
    b = stream_sketch(A_explicit(x), left_rank=lr, right_rank=rr, seed=7).to_tt()
    rec["rel_diff_same_drms"] = float(a.error(b, relative=True))
    print(f"  explicit / lazy = {rec['speedup']:.2f}, ranges apart: {rec['apart']}; with the same DRMs the two results differ by "
          f"{rec['rel_diff_same_drms']:.1e} of their norm")
    return rec


def kernel_case(name, R, r, n, l, terms, reps):
    rng = np.random.default_rng(l)
    Ls = [DevArray.from_host(rng.standard_normal((R, r, l))) for _ in range(terms)]
    Ms = [DevArray.from_host(rng.standard_normal((R, n, n, R))) for _ in range(terms)]
    Cs = [DevArray.from_host(rng.standard_normal((r, n, r))) for _ in range(terms)]
    got = {}

    def kernel():
        got["kernel"] = op_apply(Ls, Ms, Cs, route="kernel")[0]

    def composed():
        got["composed"] = op_apply(Ls, Ms, Cs, route="composed")[0]

    fl = terms * 2.0 * l * (R * r * n * r + R * n * n * R * r)
    print(f"\n({name}) op_apply alone: {terms} term(s) of R = {R}, r = {r}, n = {n}, l = {l}: {fl / 1e9:.3f} GF")
    rec = measure(name, [("kernel", kernel), ("composed", composed)], reps)
    rec.update(R=R, r=r, n=n, l=l, terms=terms, flops=fl)
    if rec["failed"]:
        return rec
    a, b = got["kernel"].get().ravel(), got["composed"].get().ravel()
    lo, hi = rec["ms"]["kernel"], rec["ms"]["composed"]
    model = route_ms([(R, R, r, r, n, n, l, False)] * terms)
    rec.update(max_rel_gap=float(np.max(np.abs(a - b)) / np.max(np.abs(b))), kernel_tflops=fl / lo["median"] / 1e9,
               apart=bool(lo["max"] < hi["min"] or hi["max"] < lo["min"]), model_ms=dict(kernel=model[0], composed=model[1]),
               route="composed" if model[1] < model[0] else "kernel")
    print(f"  kernel {rec['kernel_tflops']:.2f} TF/s; composed / kernel = {hi['median'] / lo['median']:.2f}, ranges apart: {rec['apart']}; "
          f"largest gap {rec['max_rel_gap']:.1e}; rule: kernel {model[0]:.3f} ms, composed {model[1]:.3f} ms -> {rec['route']}")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--cases", default="G1,G2,K1,K2,K3")
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    nat.call("ttsk_init", 0)
    cases = args.cases.split(",")
    recs = []
    if "G1" in cases:
        recs.append(sketch_case("G1", (20,) * 8, 20, 4, 3, 20, 40, args.reps))         # round_tt_sum(max_rank=20, oversample_factor=2)
    if "G2" in cases:
        recs.append(sketch_case("G2", (100,) * 6, 64, 8, 1, 50, 100, max(3, args.reps // 3)))
    if "K1" in cases:
        recs.append(kernel_case("K1", 4, 20, 20, 20, 1, args.reps))
    if "K2" in cases:
        recs.append(kernel_case("K2", 8, 64, 100, 50, 1, args.reps))
    if "K3" in cases:
        recs.append(kernel_case("K3", 8, 64, 100, 50, 3, args.reps))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(cases=recs), f, indent=1)


if __name__ == "__main__":
    main()
