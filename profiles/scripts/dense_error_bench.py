"""Times the error of a resident tensor train against a dense device tensor, in one process and with device events:

  fused      TensorTrain.dense_stats: the panels L, R by the contraction kernel, one pass of ttsk_tt_dense_stats, the
             four sums read back
  composed   what the device primitives gave before: full(tt) by `contract` into a second array the size of X,
             x.t and t.t by `contract`, `axpby` to t - x in place, |t - x|^2 by `contract`

at C2 (d = 5, n = 64, 8.59 GB) with all bonds at rho in {3, 20, 40, 64}, and (fused only unless --composed-big) at
d = 3, n = 2048 (68.7 GB) with rho = 100, where the pass runs in slabs.  The variants are alternated, REPS timed
repetitions after WARM warm-up rounds; median and spread (min .. max) are reported beside the two roofs of the pass:
8 |X| bytes at the streaming rate --hbm (TB/s, as bench.py measures it) and 2 rho |X| flops at ttsk_mfma_f64_peak_probe.

    python profiles/scripts/dense_error_bench.py [--json out.json] [--only-fused] [--cases c2] [--hbm 5.0]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from tt_sketch_amd import TensorTrain, _native as nat
from tt_sketch_amd import device as dev
from tt_sketch_amd.device import DevArray, axpby, contract
from tt_sketch_amd.tensor_dense import _dense_split, _tt_dense_pass

WARM, REPS = 3, 21


def timed(fn):
    nat.call("ttsk_timer_start", 0)
    fn()
    ms = ctypes.c_float()
    nat.call("ttsk_timer_stop", 0, ctypes.byref(ms))
    return float(ms.value)


def run(name, shape, rho, peak_tf, hbm_tbs, composed=True):
    rng = np.random.default_rng(4)
    d = len(shape)
    rk = (1,) + (rho,) * (d - 1) + (1,)
    cores = [DevArray.from_host(rng.standard_normal((rk[k], n, rk[k + 1])) / np.sqrt(rk[k])) for k, n in enumerate(shape)]
    tt = TensorTrain(cores)
    X = tt.to_dense_dev().data                      # error 0: the time does not depend on the values
    size = X.size
    plan = _dense_split(shape, tt.rank)
    big_before = dev._pool_bytes[True]
    got = {}

    def fused():
        got["fused"] = _tt_dense_pass(tt, X, False, True)[1]

    def comp():
        P = cores[0].reshape(shape[0], -1)
        for c in cores[1:]:
            P = contract("ia,ajb->ijb", P, c)
            P = P.reshape(-1, P.shape[-1])
        T, x = P.reshape(size, 1), X.reshape(size, 1)
        xt = contract("ka,kb->ab", x, T)
        tt_ = contract("ka,kb->ab", T, T)
        axpby(T, x, -1.0, 1.0)
        rr = contract("ka,kb->ab", T, T)
        got["composed"] = np.array([xt.get()[0, 0], tt_.get()[0, 0], rr.get()[0, 0]])

    variants = [("fused", fused)] + ([("composed", comp)] if composed else [])
    times = {k: [] for k, _ in variants}
    for rep in range(WARM + REPS):
        for k, fn in variants:
            ms = timed(fn)
            if rep >= WARM:
                times[k].append(ms)
        if rep == 0:
            # allocation check: what the fused variant left in the large pool after its first run (panels only)
            got["fused_pool_growth"] = None if composed else dev._pool_bytes[True] - big_before
    flops, nbytes = 2.0 * plan["rho"] * size, 8.0 * size
    rec = dict(case=name, shape=shape, rho=rho, plan={k: plan[k] for k in ("k", "M", "N", "rho")}, slabs=len(plan["slabs"]),
               bytes=nbytes, flops=flops, ms={}, sums={k: [float(v) for v in got[k]] for k, _ in variants})
    print(f"\n{name}: shape {shape}, rho {rho}, cut at bond {plan['k']} (M {plan['M']}, N {plan['N']}), {len(plan['slabs'])} slab(s); "
          f"panels {8 * (plan['M'] + plan['N']) * plan['rho'] / 1e6:.1f} MB beside X = {nbytes / 1e9:.2f} GB")
    for k, _ in variants:
        t = np.array(times[k])
        med = float(np.median(t))
        rec["ms"][k] = dict(median=med, min=float(t.min()), max=float(t.max()))
        line = f"  {k:9s} median {med:9.3f} ms  (min {t.min():.3f} .. max {t.max():.3f}, {len(t)} reps)"
        if k == "fused":
            rec["roof"] = dict(hbm_fraction=nbytes / (hbm_tbs * 1e12) / (med * 1e-3), mfma_fraction=flops / (peak_tf * 1e12) / (med * 1e-3),
                               hbm_ms=nbytes / (hbm_tbs * 1e9), mfma_ms=flops / (peak_tf * 1e9))
            line += (f"   X at {nbytes / med / 1e9:6.2f} TB/s = {rec['roof']['hbm_fraction']:.2f} of {hbm_tbs} TB/s;  "
                     f"{flops / med / 1e9:6.2f} TF/s = {rec['roof']['mfma_fraction']:.2f} of the probe's {peak_tf:.1f}")
        print(line)
    if composed:
        f, c = rec["ms"]["fused"], rec["ms"]["composed"]
        rec["ratio"] = c["median"] / f["median"]
        print(f"  composed / fused = {rec['ratio']:.2f}; gap {c['median'] - f['median']:.3f} ms against spreads fused "
              f"{f['max'] - f['min']:.3f} + composed {c['max'] - c['min']:.3f} ms")
        a, b = got["fused"], got["composed"]
        assert abs(a[0] - b[0]) <= 1e-10 * abs(b[0]) and abs(a[1] - b[1]) <= 1e-10 * b[1], "fused and composed sums differ"
    del X
    dev.release_cached()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--only-fused", action="store_true", help="the fused variant alone (for a kernel trace)")
    ap.add_argument("--composed-big", action="store_true", help="the composition at 2048^3 too (137 GB of arrays)")
    ap.add_argument("--cases", default="c2,big")
    ap.add_argument("--hbm", type=float, default=5.0, help="streaming read rate in TB/s the byte roof is stated against")
    args = ap.parse_args()
    nat.call("ttsk_init", 0)
    probe = ctypes.c_double()
    nat.call("ttsk_mfma_f64_peak_probe", ctypes.byref(probe))
    print(f"fp64 MFMA probe {probe.value:.1f} TF/s, HBM roof stated against {args.hbm} TB/s")
    recs = []
    if "c2" in args.cases:
        for rho in (3, 20, 40, 64):
            recs.append(run(f"C2 rho {rho}", (64,) * 5, rho, probe.value, args.hbm, not args.only_fused))
    if "big" in args.cases:
        recs.append(run("d3 2048^3 rho 100", (2048,) * 3, 100, probe.value, args.hbm, args.composed_big and not args.only_fused))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(probe_tflops=probe.value, hbm_tbs=args.hbm, cases=recs), f, indent=1)


if __name__ == "__main__":
    main()
