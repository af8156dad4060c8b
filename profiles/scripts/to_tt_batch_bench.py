"""to_tt_batch at C3 (d = 6, n = 200, TT rank 100 -> l = 50, r = 100), batch 32: ms per tensor of
  to_tt_batch(sks)                      the batched assembly (ttsk_tt_assemble_batch)
  [s.to_tt() for s in sks]              one ttsk_tt_assemble per tensor
  stream_sketch_batch + to_tt_batch     the whole recompression
and the work of the fused apply per tensor (FLOP and HBM bytes computed from the shapes), to set against the kernel time
that `rocprofv3 --kernel-trace --stats` reports for assemble_apply_kernel.
  --profile B   one warm-up and one timed to_tt_batch of a batch of B only (for a kernel trace: launches per call)
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))   # the repository root
import numpy as np  # noqa: E402
from tt_sketch_amd import _native as nat  # noqa: E402
from tt_sketch_amd import TensorTrain, TensorTrainDRM, stream_sketch_batch, to_tt_batch  # noqa: E402
from tt_sketch_amd.utils import random_normal_dev  # noqa: E402

PEAK_TFS, HBM_TBS = 78.6, 6.3          # fp64 matrix peak; measured HBM read rate (DESIGN)

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--profile", type=int, default=0)
args = ap.parse_args()

nat.call("ttsk_init", 0)
d, n, s, l, r = 6, 200, 100, 50, 100
shape = (n,) * d
B = args.profile or args.batch


def device_tt(seed):
    S = (1,) + (s,) * (d - 1) + (1,)
    return TensorTrain([random_normal_dev((S[k], n, S[k + 1]), seed=(seed << 8) + k, scale=1.0 / np.sqrt(S[k] * n)) for k in range(d)])


tts = [device_tt(1000 + b) for b in range(B)]
left = TensorTrainDRM(l, shape, False, seed=1)
right = TensorTrainDRM(r, shape, True, seed=2)
sk = lambda: stream_sketch_batch(tts, (l,) * (d - 1), (r,) * (d - 1), left_drm=left, right_drm=right)
sks = sk()
nat.call("ttsk_sync", -1)
if args.profile:
    to_tt_batch(sks)
    nat.call("ttsk_sync", -1)
    to_tt_batch(sks)
    nat.call("ttsk_sync", -1)
    print(f"profile: batch {B}: two to_tt_batch calls")
    sys.exit(0)


def T(f, reps=args.reps):
    f()
    nat.call("ttsk_sync", -1)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        nat.call("ttsk_sync", -1)
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3, float(np.min(ts)) * 1e3


rows = n + (d - 2) * l * n                          # right direction: unfolding rows of the d - 1 pairs
flops = 3 * 2.0 * rows * r * l                      # C = Psi P, R = Psi - C Omega, C += R P
nbytes = 8.0 * rows * (r + l)                       # Psi read once, C written once (P, Omega: L2-resident)
res = {}
res["to_tt_batch"] = T(lambda: to_tt_batch(sks))
res["per-tensor to_tt"] = T(lambda: [x.to_tt() for x in sks])
res["stream_sketch_batch + to_tt_batch"] = T(lambda: to_tt_batch(sk()))
res["stream_sketch_batch"] = T(sk)
print(f"C3, batch {B}: d {d}, n {n}, TT rank {s}, l {l}, r {r}")
for k, (med, mn) in res.items():
    print(f"  {k:38s} {med / B:8.4f} ms per tensor (median of {args.reps}; min {mn / B:.4f})")
print(f"  fused apply per tensor: {flops / 1e9:.3f} GF, {nbytes / 1e6:.1f} MB; at the {PEAK_TFS} TF/s fp64 matrix peak "
      f"{flops / PEAK_TFS / 1e6:.1f} us, at {HBM_TBS} TB/s {nbytes / HBM_TBS / 1e6:.1f} us")
