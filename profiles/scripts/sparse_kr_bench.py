"""Times the streaming sketch of the C4 tensor of bench.py (d = 5, shape (200, 150, 100, 120, 300), 10^7 nonzeros, rng seed 4)
at l = 10, r = 15 on the one-pass sparse kernel with three pairs of DRMs: Khatri-Rao / Khatri-Rao (tables and the diagonal
chain factors, kind 5 of ttsk_sg_factor), Gaussian / Gaussian (SparseGaussianDRM: tables and columns sampled in the pass)
and train / train (TensorTrainDRM: tables and rank x rank chain steps, paths.forced("kernel")).

`general_sketch` with the DRMs pre-built, the tensor resident, its streams and the DRMs' tables made by the warm-up rounds;
wall-clock time of a call, closed by a synchronisation of the device.  The three legs are alternated in one process; each is
repeated until it has filled a second (at least MIN_REPS, at most MAX_REPS times); medians.  Beside the times the record
holds what each pair's passes did (sparse_fused.last_plan) and where its chains start.

    python profiles/scripts/sparse_kr_bench.py [--json profiles/sparse_kr_bench.json] [--nnz 10000000]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from tt_sketch_amd import KhatriRaoDRM, SparseGaussianDRM, SparseTensor, TensorTrainDRM, paths, sparse_fused, _native as nat
from tt_sketch_amd.device import sync
from tt_sketch_amd.sketch_dispatch import SketchMethod, general_sketch

WARM, MIN_REPS, MAX_REPS, FILL_S = 2, 5, 200, 1.0
SHAPE, L_RANK, R_RANK = (200, 150, 100, 120, 300), 10, 15


def timed(fn):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--nnz", type=int, default=10_000_000)
    args = ap.parse_args()
    nat.call("ttsk_init", 0)
    shape, nnz, d = SHAPE, args.nnz, len(SHAPE)
    rng = np.random.default_rng(4)
    idx = np.stack([rng.integers(0, n, nnz) for n in shape]).astype(np.int64)
    T = SparseTensor(shape, idx, rng.standard_normal(nnz))
    T.prepare_device()
    pairs = {
        "khatri_rao": (KhatriRaoDRM(L_RANK, shape, False, seed=3), KhatriRaoDRM(R_RANK, shape, True, seed=4)),
        "gaussian": (SparseGaussianDRM(L_RANK, shape, False, seed=3), SparseGaussianDRM(R_RANK, shape, True, seed=4)),
        "train": (TensorTrainDRM(L_RANK, shape, False, seed=3), TensorTrainDRM(R_RANK, shape, True, seed=4)),
    }
    plans = {}

    def leg(name):
        left, right = pairs[name]

        def run():
            with paths.forced("kernel" if name == "train" else None):
                general_sketch(T, left, right, SketchMethod.streaming)
            plans[name] = dict(sparse_fused.last_plan)
        return run

    legs = [(name, leg(name)) for name in pairs]
    times = {k: [] for k, _ in legs}
    for _ in range(WARM):
        for _, fn in legs:
            fn()
    rep = 0
    while rep < MAX_REPS and (rep < MIN_REPS or min(sum(t) for t in times.values()) < FILL_S * 1e3):
        for k, fn in legs:
            times[k].append(timed(fn))
        rep += 1
    rec = dict(shape=list(shape), nnz=nnz, l=L_RANK, r=R_RANK, legs={})
    for k, _ in legs:
        t = np.array(times[k])
        left, right = pairs[k]
        Ls, Rs = sparse_fused._Side(left, shape, nnz), sparse_fused._Side(right, shape[::-1], nnz)
        start = lambda S: [S._kr_start(j) if S.kr else (S.start_level(j) if S.tt else (j if S.use_table(j) else None)) for j in range(d - 1)]
        rec["legs"][k] = dict(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), reps=len(t), plan=plans[k],
                              table_levels_left=start(Ls), table_levels_right=start(Rs))
        print(f"  {k:12s} median {np.median(t):9.3f} ms  (min {t.min():.3f} .. max {t.max():.3f}, {len(t)} reps)  {plans[k]}", flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
