"""Times Gram-SVD rounding (TensorTrain.round_gram: two Gram chains, ttsk_gram_round_bonds, one read-back, core update)
against the sweeps it stands beside (TensorTrain.round_dev), in one process, with device events on library stream 0 and the
host clock next to them:

  (a) the north-star shape: d = 6, n = 200, rank 100 -> 50
  (b) the GMRES shape: d = 8, n = 20, the direct sum of three rank-20 terms (rank 60) -> 20
  (c) d = 6, n = 200, rank 200 -> 100

`round_gram` is also timed in its three parts (each with a stream sync at its end, so their sum exceeds the whole, which
syncs once): the Gram chains, the bond solve with the read-back of the ranks, the core update.

The variants are alternated, REPS timed repetitions after WARM warm-up rounds; median and spread (min .. max).  Both
roundings start from the same resident train; the error of each result against the input is the Gram-chain error
(error(fast=True)), good to about 1e-8.

    python profiles/scripts/gram_round_bench.py [--json out.json] [--cases a,b,c] [--reps 11]
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from tt_sketch_amd import TensorTrain, _native as nat
from tt_sketch_amd import tensor_round as tr
from tt_sketch_amd.device import DevArray, contract
from tt_sketch_amd.utils import process_tt_rank

WARM = 2


def timed(fn):
    """(device ms between two events on stream 0, host ms) of fn, which ends with the stream drained"""
    nat.call("ttsk_sync", -1)
    t0 = time.perf_counter()
    nat.call("ttsk_timer_start", 0)
    fn()
    ms = ctypes.c_float()
    nat.call("ttsk_timer_stop", 0, ctypes.byref(ms))
    return float(ms.value), (time.perf_counter() - t0) * 1e3


def random_tt(rng, shape, r):
    rk = (1,) + (r,) * (len(shape) - 1) + (1,)
    return TensorTrain([DevArray.from_host(rng.standard_normal((rk[k], n, rk[k + 1])) / np.sqrt(rk[k] * n)) for k, n in enumerate(shape)])


def stats(t):
    t = np.array(t)
    return dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()), reps=len(t))


def measure(name, x, max_rank, reps):
    caps = process_tt_rank(max_rank, x.shape, trim=True)
    cores = [c.contiguous() for c in x.dev_cores()]
    got, state = {}, {}

    def gram():
        got["round_gram"] = x.round_gram(max_rank=max_rank)

    def dev():
        got["round_dev"] = x.round_dev(max_rank=max_rank)

    def chains():
        state["G"] = tr._grams(cores)
        nat.call("ttsk_sync", 0)

    def solve():
        state["sol"] = tr._bond_solve(state["G"][0], state["G"][1], list(x.rank), list(caps), 0.0)
        state["rho"] = [int(r) for r in state["sol"][3].get()]
        nat.call("ttsk_sync", tr._HELPER)

    def update():
        Pt, Q, _, _ = state["sol"]
        rho, out = state["rho"], []
        for k, C in enumerate(cores):
            if k > 0:
                C = contract("ca,aib->cib", Q[k - 1][:rho[k - 1]], C)
            if k < x.ndim - 1:
                C = contract("cib,eb->cie", C, Pt[k][:rho[k]])
            out.append(C)
        nat.call("ttsk_sync", 0)

    variants = [("round_gram", gram), ("round_dev", dev), ("gram_chains", chains), ("bond_solve", solve), ("core_update", update)]
    dev_ms, host_ms = {k: [] for k, _ in variants}, {k: [] for k, _ in variants}
    for rep in range(WARM + reps):
        for k, fn in variants:
            d, h = timed(fn)
            if rep >= WARM:
                dev_ms[k].append(d)
                host_ms[k].append(h)
    rec = dict(case=name, shape=list(x.shape), rank=list(x.rank), max_rank=max_rank, ms={}, host_ms={})
    for k, _ in variants:
        rec["ms"][k], rec["host_ms"][k] = stats(dev_ms[k]), stats(host_ms[k])
        s = rec["ms"][k]
        print(f"  {k:12s} median {s['median']:9.3f} ms  (min {s['min']:.3f} .. max {s['max']:.3f}, {s['reps']} reps; host {rec['host_ms'][k]['median']:.3f} ms)")
    rec["ranks"] = {k: list(v.rank) for k, v in got.items()}
    rec["rel_error"] = {k: float(v.error(x, relative=True, fast=True)) for k, v in got.items()}
    rec["speedup"] = rec["ms"]["round_dev"]["median"] / rec["ms"]["round_gram"]["median"]
    print(f"  ranks equal: {rec['ranks']['round_gram'] == rec['ranks']['round_dev']}; relative error round_gram {rec['rel_error']['round_gram']:.6e}, "
          f"round_dev {rec['rel_error']['round_dev']:.6e}; round_dev / round_gram = {rec['speedup']:.2f}")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--reps", type=int, default=11)
    args = ap.parse_args()
    nat.call("ttsk_init", 0)
    rng = np.random.default_rng(1)
    recs = []
    if "a" in args.cases:
        print("\n(a) north-star: d = 6, n = 200, rank 100 -> 50")
        recs.append(measure("a", random_tt(rng, (200,) * 6, 100), 50, args.reps))
    if "b" in args.cases:
        print("\n(b) GMRES: d = 8, n = 20, three rank-20 terms (rank 60) -> 20")
        terms = [random_tt(rng, (20,) * 8, 20) for _ in range(3)]
        recs.append(measure("b", terms[0].add(terms[1]).add(terms[2]), 20, args.reps))
    if "c" in args.cases:
        print("\n(c) d = 6, n = 200, rank 200 -> 100")
        recs.append(measure("c", random_tt(rng, (200,) * 6, 200), 100, max(3, args.reps // 2)))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(cases=recs), f, indent=1)


if __name__ == "__main__":
    main()
