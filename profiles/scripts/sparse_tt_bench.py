"""Times the streaming sketch of a sparse tensor with tensor-train DRMs on the one-pass sparse kernel (chain factors of
csrc/sparse_pass.h; paths.forced("kernel")) against the panel path it replaces (TensorTrainDRM.sketch_sparse with its
(nnz x rank) panels and the fp64 atomics of ttsk_sparse_psi; paths.forced("composed")), and beside them the same tensor with
hashed DRMs (SparseGaussianDRM on both sides, the pass without chain factors).

`general_sketch` with the DRMs pre-built, the tensor resident, its streams and the DRMs' tables made by the warm-up rounds;
wall-clock time of a call, read-back of the sketch included, closed by a synchronisation of the device.  The legs are
alternated in one process; each is repeated until it has filled a second (at least MIN_REPS, at most MAX_REPS times);
medians.  The record also holds what sparse_fused.chain_route_ms is asked with, and the fit of its constants is made from it.

    python profiles/scripts/sparse_tt_bench.py [--json profiles/sparse_tt_bench.json] [--cases c4_1e7,c4_1e6,...]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from tt_sketch_amd import SparseGaussianDRM, SparseTensor, TensorTrainDRM, paths, sparse_fused, _native as nat
from tt_sketch_amd.device import sync
from tt_sketch_amd.sketch_dispatch import SketchMethod, general_sketch

WARM, MIN_REPS, MAX_REPS, FILL_S = 2, 5, 400, 1.0
C4 = (200, 150, 100, 120, 300)
CASES = {
    # name: (shape, nnz, l, r)
    "c4_1e7": (C4, 10 ** 7, 10, 15),
    "c4_1e6": (C4, 10 ** 6, 10, 15),
    "c4_2e5": (C4, 2 * 10 ** 5, 10, 15),
    "d3_1e6": ((10 ** 4, 10 ** 4, 10 ** 3), 10 ** 6, 10, 15),
    "c4_1e7_r32": (C4, 10 ** 7, 32, 32),
}


def timed(fn):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def measure(legs):
    times = {k: [] for k, _ in legs}
    for _ in range(WARM):
        for _, fn in legs:
            fn()
    rep = 0
    while rep < MAX_REPS and (rep < MIN_REPS or min(sum(t) for t in times.values()) < FILL_S * 1e3):
        for k, fn in legs:
            times[k].append(timed(fn))
        rep += 1
    out = {}
    for k, _ in legs:
        t = np.array(times[k])
        out[k] = dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()), reps=len(t))
        print(f"  {k:12s} median {np.median(t):9.3f} ms  (min {t.min():.3f} .. max {t.max():.3f}, {len(t)} reps)", flush=True)
    return out


def case(name, shape, nnz, l, r):
    print(f"\n({name}) shape {shape}, nnz = {nnz}, l = {l}, r = {r}", flush=True)
    d = len(shape)
    rng = np.random.default_rng(nnz % 1000 + d)
    idx = np.stack([rng.integers(0, n, nnz) for n in shape]).astype(np.int64)
    T = SparseTensor(shape, idx, rng.standard_normal(nnz))
    T.prepare_device()
    lt, rt = TensorTrainDRM(l, shape, transpose=False, seed=1), TensorTrainDRM(r, shape, transpose=True, seed=2)
    lh, rh = SparseGaussianDRM(l, shape, transpose=False, seed=1), SparseGaussianDRM(r, shape, transpose=True, seed=2)
    got = {}

    def leg(route, left, right):
        def run():
            with paths.forced(route):
                got[route] = general_sketch(T, left, right, SketchMethod.streaming)
        return run

    L, R = sparse_fused._Side(lt, shape, nnz), sparse_fused._Side(rt, shape[::-1], nnz)
    work, panels, panel_fma = sparse_fused._route_inputs(L, R, sparse_fused._riders(L, R, d), d)
    ms = measure([("tt_kernel", leg("kernel", lt, rt)), ("tt_composed", leg("composed", lt, rt)), ("hashed", leg(None, lh, rh))])
    a, b = got["kernel"], got["composed"]
    gap = max(float(np.linalg.norm(x - y) / np.linalg.norm(y)) for x, y in zip(a.Psi_cores + a.Omega_mats, b.Psi_cores + b.Omega_mats))
    k_ms, c_ms = ms["tt_kernel"]["median"], ms["tt_composed"]["median"]
    rule = sparse_fused.chain_route_ms(nnz, d, work, panels, panel_fma)
    print(f"  start levels left {[L.start_level(k) for k in range(d - 1)]}, right {[R.start_level(k) for k in range(d - 1)]}; "
          f"{work} (weighted) chain multiply-adds, {panels} panel columns and {panel_fma} panel multiply-adds per nonzero")
    print(f"  pass / panels = {k_ms / c_ms:.3f}; the rule expects {rule[0]:.3f} / {rule[1]:.3f} ms; largest relative gap {gap:.2e}", flush=True)
    return dict(name=name, shape=list(shape), nnz=nnz, l=l, r=r, chain_fma=work, panel_cols=panels, panel_fma=panel_fma, tt_kernel_ms=k_ms, tt_composed_ms=c_ms,
                hashed_ms=ms["hashed"]["median"], winner="kernel" if k_ms <= c_ms else "composed", max_rel_gap=gap, legs=ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    nat.call("ttsk_init", 0)
    recs = []
    for name in args.cases.split(","):
        recs.append(case(name, *CASES[name]))
        if args.json:                          # after every case: a run cut short keeps what it has measured
            with open(args.json, "w") as f:
                json.dump(dict(cases=recs), f, indent=1)


if __name__ == "__main__":
    main()
