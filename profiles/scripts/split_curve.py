"""Kernel times and step times of ttsk_tt_sketch_batch at bench.py's C3 (32 tensors) under CU budgets forced with
ttsk_tt_sketch_split: the raw series behind profiles/split_curve.json (DESIGN.md "CU budgets").
usage: python profiles/scripts/split_curve.py OUT.json"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tt_sketch_amd import TensorTrainDRM, _native as nat  # noqa: E402
from tt_sketch_amd.device import DevArray  # noqa: E402
from tt_sketch_amd.tt_fused import TTSketchPlan  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else "split_curve_raw.json"
nat.call("ttsk_init", 0)
D, N, S, L, R, B = bench.D, bench.N_MODE, bench.S_IN, bench.L_RANK, bench.R_RANK, 32
shape = (N,) * D
tts = [bench.device_tt(shape, S, 1000 + b) for b in range(B)]
left = TensorTrainDRM(L, shape, False, seed=1)
right = TensorTrainDRM(R, shape, True, seed=2)
plan = TTSketchPlan(shape, (S,) * (D - 1), left, right)
stride = plan.size + (plan.size & 1)
outs = [DevArray.empty((B * stride,)) for _ in range(2)]
keep, flat = [], []
for t in tts:
    p1, k1 = plan.core_pointers(t)
    keep.append(k1)
    flat += [p1[i] for i in range(plan.d)]
ptrs = (ctypes.c_void_p * len(flat))(*flat)
CLS = {1: "right", 3: "left", 4: "psi"}


def split(r, l, p):
    nat.call("ttsk_tt_sketch_split", r, l, p)


def prof_once():
    """one batched sketch with the brackets on -> {class: avg us per launch}"""
    nat.call("ttsk_sync", -1)
    nat.call("ttsk_prof_enable", 1)
    plan.run_batch(ptrs, B, outs[0], stride, stream=0)
    nat.call("ttsk_sync", -1)
    res = {}
    for c, name in CLS.items():
        n_l, ms, fl = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        nat.call("ttsk_prof_read", c, ctypes.byref(n_l), ctypes.byref(ms), ctypes.byref(fl))
        res[name] = 1e3 * ms.value / max(1, n_l.value)
        res[name + "_launches"] = n_l.value
    nat.call("ttsk_prof_enable", 0)
    return res


def wall(inflight, steps=12):
    for i in range(4):
        plan.run_batch(ptrs, B, outs[i % inflight], stride, stream=2 * (i % inflight))
    nat.call("ttsk_sync", -1)
    t0 = time.perf_counter()
    for i in range(steps):
        plan.run_batch(ptrs, B, outs[i % inflight], stride, stream=2 * (i % inflight))
    nat.call("ttsk_sync", -1)
    return 1e3 * (time.perf_counter() - t0) / steps


result = {"shape": dict(d=D, n=N, s=S, l=L, r=R, nb=B), "alone": {}, "beside": {}, "wall_ms": {}}
split(0, 0, 0)
for _ in range(3):
    plan.run_batch(ptrs, B, outs[0], stride, stream=0)
nat.call("ttsk_sync", -1)

# 1 + 3: each kernel alone on the chip (one stream), planned for X CUs
os.environ["TTSK_SINGLE_STREAM"] = "1"
for X in (64, 96, 128, 160, 192, 224, 256):
    split(X, X, X)
    prof_once()
    result["alone"][str(X)] = [prof_once() for _ in range(5)]
    print("alone", X, result["alone"][str(X)][0], flush=True)
os.environ.pop("TTSK_SINGLE_STREAM", None)

# 2: two streams, brackets on (kernel time as its own stream sees it, the other chain's kernels beside it), then the
# step time with one and two steps in flight (brackets off)
CONFIGS = [(0, 0, 0), (192, 64, 0), (192, 64, 64), (192, 64, 128), (160, 96, 0), (160, 96, 96), (160, 96, 160), (128, 128, 128),
           (224, 32, 0), (224, 32, 64), (0, 64, 64), (0, 96, 96), (192, 0, 0), (0, 0, 128), (0, 0, 0)]
for k, cfg in enumerate(CONFIGS):
    split(*cfg)
    key = "%d_%d_%d%s" % (cfg + ("_again" if k == len(CONFIGS) - 1 else "",))
    prof_once()
    result["beside"][key] = [prof_once() for _ in range(5)]
    result["wall_ms"][key] = {"inflight1": [wall(1) for _ in range(5)], "inflight2": [wall(2) for _ in range(5)]}
    print("beside", key, result["beside"][key][0], result["wall_ms"][key], flush=True)
    with open(OUT, "w") as f:
        json.dump(result, f, indent=1)
split(-1, -1, -1)
result["wall_ms"]["auto"] = {"inflight1": [wall(1) for _ in range(5)], "inflight2": [wall(2) for _ in range(5)]}
print("auto", result["wall_ms"]["auto"], flush=True)
with open(OUT, "w") as f:
    json.dump(result, f, indent=1)
