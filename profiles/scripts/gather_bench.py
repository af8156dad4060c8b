"""Times the evaluation of a resident tensor train at an index list, in one process and with device events:

  fused+out    ttsk_tt_gather writing the (N,) values
  fused+stats  ttsk_tt_gather forming the three sums only
  composed     the same values from ttsk_sparse_ttdrm_step, one launch per mode, (N x rank) panels in HBM, no chunking
               (what could be assembled before the fused kernel existed)

at the full C4 shape (d = 5, shape (200, 150, 100, 120, 300), N = 10^7, ranks 10) and at the C3 ranks with the sample
size of the reference's scripts/frostt.py (d = 6, n = 200, ranks 100, N = 10^4).  The three are alternated, REPS timed
repetitions after WARM warm-up rounds; median and spread (min .. max) are reported beside the byte model.

    python profiles/scripts/gather_bench.py [--json out.json] [--only-fused]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from tt_sketch_amd import _native as nat
from tt_sketch_amd.device import DevArray

WARM, REPS = 3, 21


def byte_model(shape, ranks, N):
    """Bytes per pass.  hbm: what any algorithm must move (indices, entries, cores once); l2: the slice rows
    G_k[a, i_k, :] every tuple reads through the cache, 8 N sum r_k r_{k+1}; panels: what the composition adds, one
    write and one read of an (N x r) panel between consecutive modes, 8 N (r_k + r_{k+1}) per mode."""
    d = len(shape)
    rk = (1,) + tuple(ranks) + (1,)
    cores = 8 * sum(rk[k] * shape[k] * rk[k + 1] for k in range(d))
    return dict(hbm=8 * N * (d + 1) + cores, cores=cores,
                l2=8 * N * sum(rk[k] * rk[k + 1] for k in range(d)),
                panels=8 * N * sum(rk[k] + rk[k + 1] for k in range(d)))


def timed(fn):
    nat.call("ttsk_timer_start", 0)
    fn()
    ms = ctypes.c_float()
    nat.call("ttsk_timer_stop", 0, ctypes.byref(ms))
    return float(ms.value)


def run(name, shape, ranks, N, only_fused=False):
    rng = np.random.default_rng(4)
    d = len(shape)
    rk = (1,) + tuple(ranks) + (1,)
    idx = DevArray.from_host(np.stack([rng.integers(0, n, N) for n in shape]).astype(np.int64), dtype=np.int64)
    val = DevArray.from_host(rng.standard_normal(N))
    cores = [DevArray.from_host(rng.standard_normal((rk[k], n, rk[k + 1])) / np.sqrt(rk[k])) for k, n in enumerate(shape)]
    out, out2, stats = DevArray.empty((N,)), DevArray.empty((N,)), DevArray.empty((3,))
    widest = max(rk)
    panels = [DevArray.empty((N, widest)), DevArray.empty((N, widest))]
    P = lambda a: ctypes.c_void_p(a.ptr)
    cptr = (ctypes.c_void_p * d)(*[c.ptr for c in cores])
    crk, cshape = (ctypes.c_int64 * (d + 1))(*rk), (ctypes.c_int64 * d)(*shape)

    def fused_out():
        nat.call("ttsk_tt_gather", cptr, crk, cshape, d, P(idx), N, None, ctypes.c_size_t(N), None, P(out), None, 0)

    def fused_stats():
        nat.call("ttsk_tt_gather", cptr, crk, cshape, d, P(idx), N, None, ctypes.c_size_t(N), P(val), None, P(stats), 0)

    def composed():
        v = None
        for k in range(d):
            dst = out2 if k == d - 1 else panels[k & 1]
            nat.call("ttsk_sparse_ttdrm_step", None if v is None else P(v), rk[k], P(cores[k]), shape[k], rk[k + 1],
                     ctypes.c_void_p(idx.ptr + k * N * 8), ctypes.c_size_t(N), P(dst), 0)
            v = dst

    variants = [("fused+out", fused_out), ("fused+stats", fused_stats)] + ([] if only_fused else [("composed", composed)])
    times = {k: [] for k, _ in variants}
    for rep in range(WARM + REPS):
        for k, fn in variants:
            ms = timed(fn)
            if rep >= WARM:
                times[k].append(ms)
    if not only_fused:
        a, b = out.get(), out2.get()
        assert np.linalg.norm(a - b) <= 1e-12 * np.linalg.norm(b), "fused and composed values differ"
    bm = byte_model(shape, ranks, N)
    rec = dict(case=name, shape=shape, ranks=ranks, N=N, bytes=bm, ms={})
    print(f"\n{name}: shape {shape}, ranks {ranks}, N = {N}")
    print(f"  byte model: HBM {bm['hbm'] / 1e6:.1f} MB (cores {bm['cores'] / 1e6:.2f} MB), slice rows through L2 "
          f"{bm['l2'] / 1e9:.3f} GB, panels of the composition {bm['panels'] / 1e9:.3f} GB")
    for k, _ in variants:
        t = np.array(times[k])
        med = float(np.median(t))
        rec["ms"][k] = dict(median=med, min=float(t.min()), max=float(t.max()))
        extra = bm["panels"] if k == "composed" else 0
        print(f"  {k:12s} median {med:9.4f} ms  (min {t.min():.4f} .. max {t.max():.4f}, {len(t)} reps)   "
              f"HBM model {(bm['hbm'] + extra) / med / 1e6:8.1f} GB/s   L2 rows {bm['l2'] / med / 1e6:8.1f} GB/s")
    if not only_fused:
        f, c = rec["ms"]["fused+out"], rec["ms"]["composed"]
        rec["ratio"] = c["median"] / f["median"]
        print(f"  composed / fused+out = {rec['ratio']:.2f}   (spreads: fused {f['max'] - f['min']:.4f} ms, composed "
              f"{c['max'] - c['min']:.4f} ms)")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--only-fused", action="store_true", help="the two fused variants alone (for a kernel trace)")
    args = ap.parse_args()
    nat.call("ttsk_init", 0)
    recs = [run("C4", (200, 150, 100, 120, 300), (10,) * 4, 10_000_000, args.only_fused),
            run("C3 ranks, frostt sample", (200,) * 6, (100,) * 5, 10_000, args.only_fused)]
    if args.json:
        with open(args.json, "w") as f:
            json.dump(recs, f, indent=1)


if __name__ == "__main__":
    main()
