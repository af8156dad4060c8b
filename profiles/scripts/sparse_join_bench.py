"""Times the sorted-key join of sparse tensors (csrc/sparse_join.hip), in one process and with device events:

  index        ttsk_sparse_key_index: keys, radix sort, permuted entries, splitters
  join         ttsk_sparse_join forming the dot only, with 8192 and with 16384 splitters (the two candidates of
               SJ_MAX_SPLIT), the queries in their original (random) order and sorted by key; and writing out as well
  dense        ttsk_dense_join against a C2-shaped dense tensor (d = 5, n = 64: 8.6 GB)
  end to end   sp.dot(sp2) of two uploaded tensors: the first call (builds the index of sp2) and the later ones
  host         the same dot on two host tensors -- the dict of every nonzero and the Python loop over the queries
               that an uploaded pair took before this pass existed -- at 10^6 nonzeros only

at the C4 shape (d = 5, n = 200) with 10^6 and 10^7 nonzeros per tensor, half of the queries present in the table.  The
variants are alternated, REPS timed repetitions after WARM warm-up rounds; median and spread (min .. max) are reported
beside the HBM roof: the algorithmic bytes (the query's index rows and entries, one key and one value per hit) over the
copy bandwidth DESIGN section 4 records (4.6 TB/s, the low end of the measured range).

    python profiles/scripts/sparse_join_bench.py [--json out.json] [--small]
"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

import tt_sketch_amd as tsa
from tt_sketch_amd import _native as nat
from tt_sketch_amd.device import DevArray

WARM, REPS = 3, 11
COPY_BW = 4.6e12            # bytes / s: DESIGN section 4, copy, low end
SPLITS = (8192, 16384)
P = lambda a: None if a is None else ctypes.c_void_p(a.ptr)


def timed(fn):
    nat.call("ttsk_timer_start", 0)
    fn()
    ms = ctypes.c_float()
    nat.call("ttsk_timer_stop", 0, ctypes.byref(ms))
    return float(ms.value)


def alternate(variants):
    times = {k: [] for k, _ in variants}
    for rep in range(WARM + REPS):
        for k, fn in variants:
            ms = timed(fn)
            if rep >= WARM:
                times[k].append(ms)
    return {k: dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t))) for k, t in times.items()}


def layout(N, max_split):
    out = (ctypes.c_int64 * 8)()
    nat.call("ttsk_sparse_join_layout", N, N, max_split, out)
    return dict(zip(("max_split", "stride", "n_split", "lds_steps", "seg_steps", "grid", "run", "depth"), (int(v) for v in out)))


def unravel(keys, shape):
    return np.stack(np.unravel_index(keys, shape)).astype(np.int64)


def report(name, rec, roof_ms):
    for k, t in rec.items():
        print(f"  {name:8s} {k:28s} median {t['median']:9.4f} ms  (min {t['min']:.4f} .. max {t['max']:.4f})"
              + (f"   roof {roof_ms:.4f} ms = {roof_ms / t['median']:.3f} of the time" if roof_ms else ""))


def run_sparse(shape, N, host: bool):
    rng = np.random.default_rng(N % 1000 + 5)
    d, total = len(shape), int(np.prod(shape))
    kb = rng.integers(0, total, N, dtype=np.int64)
    ka = rng.integers(0, total, N, dtype=np.int64)
    ka[:N // 2] = kb[rng.integers(0, N, N // 2)]
    ka = ka[rng.permutation(N)]
    va, vb = rng.standard_normal(N), rng.standard_normal(N)
    hits = int(np.isin(ka, kb).sum())
    order = np.argsort(ka, kind="stable")
    ia, ib = unravel(ka, shape), unravel(kb, shape)
    cshape, rows = (ctypes.c_int64 * d)(*shape), (ctypes.c_int * d)(*range(d))
    dev = dict(a=DevArray.from_host(ia, dtype=np.int64), a_sorted=DevArray.from_host(ia[:, order], dtype=np.int64),
               b=DevArray.from_host(ib, dtype=np.int64), va=DevArray.from_host(va), va_sorted=DevArray.from_host(va[order]),
               vb=DevArray.from_host(vb))
    rec = dict(shape=shape, N=N, hits=hits, reps=REPS)
    # ---- the index
    index = {}
    for ms in SPLITS:
        lay = layout(N, ms)
        index[ms] = (DevArray.empty((N,), dtype=np.int64), DevArray.empty((N,)), DevArray.empty((lay["n_split"],), dtype=np.int64))
        rec[f"layout_{ms}"] = lay

    def build(ms):
        k, v, s = index[ms]
        return lambda: nat.call("ttsk_sparse_key_index", cshape, d, P(dev["b"]), N, rows, ctypes.c_size_t(N), P(dev["vb"]), ms, P(k), P(v), P(s), 0)
    rec["index_ms"] = alternate([(f"index, {ms} splitters", build(ms)) for ms in SPLITS])
    index_bytes = N * (8 * d + 8) + 2 * 16 * N + 16 * N         # read rows and entries; the pairs in and out of one sort pass; the index written
    rec["index_bytes_floor"] = index_bytes
    report("index", rec["index_ms"], index_bytes / COPY_BW * 1e3)
    # ---- the join
    out, dot = DevArray.empty((N,)), DevArray.empty((1,))
    default = layout(N, 0)["max_split"]                         # SJ_MAX_SPLIT

    def join(ms, q, v, o):
        k, vals, s = index[ms]
        return lambda: nat.call("ttsk_sparse_join", P(k), P(vals), P(s), ctypes.c_size_t(N), ms, cshape, d, P(dev[q]), N, rows, ctypes.c_size_t(N),
                                P(dev[v]), P(o), P(dot), 0)
    variants = [(f"dot, {ms} splitters, {name} queries", join(ms, q, v, None))
                for ms in SPLITS for name, q, v in (("original", "a", "va"), ("sorted", "a_sorted", "va_sorted"))]
    variants.append((f"out + dot, {default} splitters, original queries", join(default, "a", "va", out)))
    rec["join_ms"] = alternate(variants)
    rec["join_bytes"] = 8 * N * (d + 1) + 16 * hits
    rec["join_roof_ms"] = rec["join_bytes"] / COPY_BW * 1e3
    report("join", rec["join_ms"], rec["join_roof_ms"])
    want = float(np.dot(va, dict_lookup(kb, vb, ka))) if N <= 10 ** 6 else None
    got = float(dot.get()[0])
    if want is not None:
        assert abs(got - want) <= 1e-10 * np.abs(va).sum() * np.abs(vb).max(), (got, want)
    # ---- end to end through the classes
    sp, sp2 = tsa.SparseTensor(shape, ia, va), tsa.SparseTensor(shape, ib, vb)
    sp.prepare_device()
    sp2.prepare_device()
    nat.call("ttsk_sync", -1)
    t0 = time.perf_counter()
    first = sp.dot(sp2)
    t1 = time.perf_counter()
    later = []
    for _ in range(REPS):
        t = time.perf_counter()
        again = sp.dot(sp2)
        later.append(time.perf_counter() - t)
    assert first == again == got, (first, again, got)
    rec["end_to_end_s"] = dict(first_call_with_index=t1 - t0, later_median=float(np.median(later)), later_min=min(later), later_max=max(later))
    print(f"  sp.dot(sp2): first call {1e3 * (t1 - t0):.3f} ms (builds the index), later {1e3 * np.median(later):.3f} ms "
          f"(min {1e3 * min(later):.3f} .. max {1e3 * max(later):.3f})")
    # ---- the host path two tensors took before (and two host tensors still take)
    if host:
        ha, hb = tsa.SparseTensor(shape, ia, va), tsa.SparseTensor(shape, ib, vb)
        t = time.perf_counter()
        hd = ha.dot(hb)
        rec["host_path_s"] = time.perf_counter() - t
        assert ha._dev is None and hb._dev is None and abs(hd - got) <= 1e-10 * np.abs(va).sum() * np.abs(vb).max()
        print(f"  host path (dict + loop), N = {N}: {rec['host_path_s']:.3f} s = {rec['host_path_s'] / rec['end_to_end_s']['later_median']:.0f} x the "
              f"later device calls, {rec['host_path_s'] / rec['end_to_end_s']['first_call_with_index']:.0f} x the first")
    return rec


def run_routes(shape, sizes):
    """sp.dot(sp2) of two uploaded tensors by either route of tensor_sparse, first call and later calls: the points the
    routing rule is fitted to."""
    from tt_sketch_amd import paths
    recs = []
    for N in sizes:
        rng = np.random.default_rng(N % 1000 + 3)
        total = int(np.prod(shape))
        kb = rng.integers(0, total, N, dtype=np.int64)
        ka = kb[rng.permutation(N)]
        va, vb = rng.standard_normal(N), rng.standard_normal(N)
        rec = dict(N=N)
        for route in ("kernel", "composed"):
            sp, sp2 = tsa.SparseTensor(shape, unravel(ka, shape), va), tsa.SparseTensor(shape, unravel(kb, shape), vb)
            sp.prepare_device()
            sp2.prepare_device()
            nat.call("ttsk_sync", -1)
            with paths.forced(route):
                t0 = time.perf_counter()
                first = sp.dot(sp2)
                t1 = time.perf_counter()
                later = []
                for _ in range(5):
                    t = time.perf_counter()
                    sp.dot(sp2)
                    later.append(time.perf_counter() - t)
            rec[route] = dict(first_ms=1e3 * (t1 - t0), later_ms=1e3 * float(np.median(later)), value=first)
        assert abs(rec["kernel"]["value"] - rec["composed"]["value"]) <= 1e-10 * np.abs(va).sum() * np.abs(vb).max()
        print(f"  N = {N:8d}: device first {rec['kernel']['first_ms']:9.3f} ms, later {rec['kernel']['later_ms']:8.3f} ms;   "
              f"host first {rec['composed']['first_ms']:9.3f} ms, later {rec['composed']['later_ms']:9.3f} ms")
        recs.append(rec)
    return recs


def dict_lookup(kb, vb, ka):
    table = dict(zip(kb.tolist(), vb.tolist()))
    return np.array([table.get(k, 0.0) for k in ka.tolist()])


def run_dense(shape, sizes):
    d, total = len(shape), int(np.prod(shape))
    X = DevArray.empty(shape)
    nat.call("ttsk_fill_normal", P(X), ctypes.c_size_t(total), 7, 1.0, 0)
    cshape, rows = (ctypes.c_int64 * d)(*shape), (ctypes.c_int * d)(*range(d))
    recs = []
    for N in sizes:
        rng = np.random.default_rng(N % 1000 + 9)
        keys = rng.integers(0, total, N, dtype=np.int64)
        val = DevArray.from_host(rng.standard_normal(N))
        q = {"original": DevArray.from_host(unravel(keys, shape), dtype=np.int64), "sorted": DevArray.from_host(unravel(np.sort(keys), shape), dtype=np.int64)}
        out, dot = DevArray.empty((N,)), DevArray.empty((1,))
        call = lambda name, o: (lambda: nat.call("ttsk_dense_join", P(X), cshape, d, P(q[name]), N, rows, ctypes.c_size_t(N), P(val), P(o), P(dot), 0))
        ms = alternate([("dot, original queries", call("original", None)), ("dot, sorted queries", call("sorted", None)),
                        ("out + dot, original queries", call("original", out))])
        nbytes = 8 * N * (d + 1) + 8 * N
        rec = dict(shape=shape, N=N, dense_ms=ms, bytes=nbytes, roof_ms=nbytes / COPY_BW * 1e3, sector_bytes=8 * N * (d + 1) + 64 * N)
        report("dense", ms, rec["roof_ms"])
        recs.append(rec)
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--small", action="store_true", help="a rehearsal at small sizes")
    args = ap.parse_args()
    nat.call("ttsk_init", 0)
    shape = (200,) * 5
    sizes = (10 ** 4, 10 ** 5) if args.small else (10 ** 6, 10 ** 7)
    rec = dict(copy_bandwidth=COPY_BW, sparse=[], dense=[])
    for N in sizes:
        print(f"\nC4 shape {shape}, {N} nonzeros per tensor")
        rec["sparse"].append(run_sparse(shape, N, host=N <= 10 ** 6))
    print("\nsp.dot(sp2) by route (wall clock, with the read-back)")
    rec["routes"] = run_routes(shape, (100, 1000, 10 ** 4) if args.small else (100, 1000, 10 ** 4, 10 ** 5, 10 ** 6))
    dshape = (16,) * 5 if args.small else (64,) * 5
    print(f"\ndense tensor of shape {dshape}")
    rec["dense"] = run_dense(dshape, sizes)
    h = [r for r in rec["sparse"] if "host_path_s" in r]
    if h and not args.small:
        r = h[-1]
        rec["host_path_extrapolated_s"] = {"N": 10 ** 7, "s": r["host_path_s"] * 10 ** 7 / r["N"], "note": "linear in N from the run at 10^6; not run"}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
