"""Times the Gram pass of tensor trains (ttsk_tt_gram) against the composed path it replaces, in one process and with
device events on library stream 0:

  gram       tt_gram: one ttsk_tt_gram call (one launch per mode over all pairs, one closing launch), G read back
  composed   the same numbers as the parent commit formed them

at two shapes:

  (a) the recompression check: d = 6, n = 200, ranks 50 against 100.  `gram` is the 2 x 2 Gram of error(fast=True), with
      the routing rule of tt_gram switched off (route="kernel"), here and below, so that the pass
      itself is timed;
      `composed` is error(relative=True) as it is without `fast`: add + QR sweep (norm) of the rank-150 direct sum and
      the QR sweep of the reference norm.  `chain` is the `contract` chain of dot() for the three products the formula
      needs.
  (b) an Arnoldi column: d = 8, n = 20, ranks 20, 1 x 16.  `composed` is sixteen `contract` chains, each read back.
  (c) shapes between the two, for the routing rule of tt_gram: K x M trains of one rank, pass against chain
      (d = 6: ranks 32, n = 100, 2 x 2; ranks 64, n = 50, 1 x 1; ranks 50, n = 100, 1 x 16; ranks 100, n = 50, 1 x 4;
      single pairs at ranks 30, d = 8, n = 20 and ranks 32, n = 100; ranks 64, n = 50, 4 x 4).
Every case also prints what the routing rule expects of the pass and of the chain, and which of the two it picks.

The variants are alternated, REPS timed repetitions after WARM warm-up rounds; median and spread (min .. max).

    python profiles/scripts/tt_gram_bench.py [--json out.json] [--cases a,b,c] [--reps 21]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from tt_sketch_amd import TensorTrain, tt_gram, _native as nat
from tt_sketch_amd import tensor_gram as tmod
from tt_sketch_amd.device import DevArray
from tt_sketch_amd.paths import forced
from tt_sketch_amd.tensor_gram import _tt_dot_composed

WARM = 2


def timed(fn):
    nat.call("ttsk_timer_start", 0)
    fn()
    ms = ctypes.c_float()
    nat.call("ttsk_timer_stop", 0, ctypes.byref(ms))
    return float(ms.value)


def random_tt(rng, shape, r):
    rk = (1,) + (r,) * (len(shape) - 1) + (1,)
    return TensorTrain([DevArray.from_host(rng.standard_normal((rk[k], n, rk[k + 1])) / np.sqrt(rk[k] * n)) for k, n in enumerate(shape)])


def flops(shape, ra, rb, pairs):
    d = len(shape)
    a, b = (1,) + (ra,) * (d - 1) + (1,), (1,) + (rb,) * (d - 1) + (1,)
    return pairs * sum(2.0 * n * (a[k] * b[k] * a[k + 1] + a[k + 1] * b[k] * b[k + 1]) for k, n in enumerate(shape))


def routed(rec, As, Bs, sym=False):
    """What the routing rule of tt_gram expects for the call, next to what was measured."""
    rk = [np.array([[c.shape[0] for c in t.dev_cores()] + [1] for t in ts]) for ts in (As, Bs)]
    work, chain = tmod._gram_route_ms(rk[0], rk[1], As[0].shape)
    if sym:
        chain *= (len(As) + 1) / (2 * len(Bs))
    rec["model_ms"] = dict(pass_work=float(work), chain=float(chain))
    rec["route"] = "chain" if work > chain else "pass"
    print(f"  routing rule: pass work {work:.3f} ms, chain {chain:.3f} ms -> {rec['route']}")


def measure(name, variants, reps):
    times = {k: [] for k, _ in variants}
    for rep in range(WARM + reps):
        for k, fn in variants:
            ms = timed(fn)
            if rep >= WARM:
                times[k].append(ms)
    rec = dict(case=name, ms={})
    for k, _ in variants:
        t = np.array(times[k])
        rec["ms"][k] = dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()), reps=len(t))
        print(f"  {k:9s} median {np.median(t):9.3f} ms  (min {t.min():.3f} .. max {t.max():.3f}, {len(t)} reps)")
    return rec


def case_a(reps):
    rng = np.random.default_rng(1)
    shape = (200,) * 6
    a, b = random_tt(rng, shape, 50), random_tt(rng, shape, 100)
    got = {}

    def gram():
        with forced("kernel"):                  # error() calls tt_gram without a keyword
            got["gram"] = a.error(b, fast=True, relative=True)

    def composed():
        got["composed"] = a.error(b, relative=True)

    def chain():
        aa, bb, ab = _tt_dot_composed(a, a), _tt_dot_composed(b, b), _tt_dot_composed(a, b)
        got["chain"] = np.sqrt(abs(aa + bb - 2 * ab)) / np.sqrt(bb)

    print(f"\n(a) recompression check: shape {shape}, ranks 50 against 100, 2 x 2 Gram")
    rec = measure("a", [("gram", gram), ("composed", composed), ("chain", chain)], reps)
    rec["values"] = {k: float(v) for k, v in got.items()}
    routed(rec, [a, b], [a, b], sym=True)
    rec["flops"] = flops(shape, 50, 100, 1) + flops(shape, 50, 50, 1) + flops(shape, 100, 50, 1) + flops(shape, 100, 100, 1)
    print(f"  relative error: gram {got['gram']:.12e}, composed {got['composed']:.12e}, chain {got['chain']:.12e}")
    print(f"  gram: {rec['flops'] / rec['ms']['gram']['median'] / 1e9:.2f} TF/s of the model's {rec['flops'] / 1e9:.2f} GF")
    return rec


def case_b(reps):
    rng = np.random.default_rng(2)
    shape = (20,) * 8
    w = random_tt(rng, shape, 20)
    basis = [random_tt(rng, shape, 20) for _ in range(16)]
    got = {}

    def gram():
        got["gram"] = tt_gram([w], basis, route="kernel")[0]

    def composed():
        got["composed"] = np.array([_tt_dot_composed(w, v) for v in basis])

    print(f"\n(b) Arnoldi column: shape {shape}, ranks 20, 1 x 16")
    rec = measure("b", [("gram", gram), ("composed", composed)], reps)
    rec["flops"] = flops(shape, 20, 20, 16)
    routed(rec, [w], basis)
    gap = float(np.max(np.abs(got["gram"] - got["composed"]) / np.abs(got["composed"])))
    rec["max_rel_gap"] = gap
    print(f"  largest relative gap between the two columns {gap:.2e}")
    return rec


def case_mid(name, shape, r, K, M, reps):
    rng = np.random.default_rng(3)
    As, Bs = [random_tt(rng, shape, r) for _ in range(K)], [random_tt(rng, shape, r) for _ in range(M)]
    got = {}

    def gram():
        got["gram"] = tt_gram(As, Bs, route="kernel")

    def composed():
        got["composed"] = np.array([[_tt_dot_composed(a, b) for b in Bs] for a in As])

    fl = flops(shape, r, r, K * M)
    print(f"\n({name}) shape {shape}, ranks {r}, {K} x {M}: {fl / (K * M) / 1e6:.0f} MF per pair")
    rec = measure(name, [("gram", gram), ("composed", composed)], reps)
    rec.update(shape=shape, rank=r, K=K, M=M, flops=fl, flops_per_pair=fl / (K * M))
    routed(rec, As, Bs)
    rec["max_rel_gap"] = float(np.max(np.abs(got["gram"] - got["composed"]) / np.abs(got["composed"])))
    print(f"  largest relative gap {rec['max_rel_gap']:.2e}; chain {rec['ms']['composed']['median'] / (K * M):.3f} ms per pair, "
          f"pass {fl / rec['ms']['gram']['median'] / 1e9:.2f} TF/s")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    nat.call("ttsk_init", 0)
    recs = []
    if "a" in args.cases:
        recs.append(case_a(args.reps))
    if "b" in args.cases:
        recs.append(case_b(args.reps))
    if "c" in args.cases:
        for name, shape, r, K, M in (("c1", (100,) * 6, 32, 2, 2), ("c2", (50,) * 6, 64, 1, 1), ("c3", (100,) * 6, 50, 1, 16),
                                     ("c4", (50,) * 6, 100, 1, 4), ("c5", (20,) * 8, 30, 1, 1), ("c6", (100,) * 6, 32, 1, 1),
                                     ("c7", (50,) * 6, 64, 4, 4)):
            recs.append(case_mid(name, shape, r, K, M, args.reps))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(cases=recs), f, indent=1)


if __name__ == "__main__":
    main()
