"""Times the sketch of a CP tensor with tensor-train DRMs on the one-pass kernels of csrc/cp_pass.hip against the
compositions of `contract` calls they replace, in one process and with device events on library stream 0:

  sketch     stream_sketch with the DRMs pre-built: `composed` (cp_fused.forced("composed"): the generic path, two or three
             `contract` calls per product with their N x n x rank panels) against `kernel` (cp_fused.try_cp_sketch: the
             chains on two streams, one ttsk_cp_psi_omega per mode); both with the read-back of the sketch, and the device
             part alone (`*_device`)
  chain      one ttsk_cp_chain_step at a middle mode of the left and of the right chain against its two `contract` calls
  psi        one ttsk_cp_psi_omega at a middle mode, Psi with Omega riding along, against the three `contract` calls; and
             Psi alone against its two

at two shapes of the reference's scripts:

  forest     plot_cp_forest.py: d = 8, n = 12, N = 25 000, l = 50, r = 100
  cp_tensor  plot_cp_tensor.py: d = 5, n = 10, N = 100, l = 30, r = 60

For each kernel the flops and algorithmic bytes of cp_pass_plan.h are set against the fp64 MFMA probe and the time.
The variants are alternated, REPS timed repetitions after WARM warm-up rounds; median and spread (min .. max).

    python profiles/scripts/cp_sketch_bench.py [--json out.json] [--cases forest,cp_tensor] [--reps 21]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from tt_sketch_amd import CPTensor, TensorTrainDRM, cp_fused, stream_sketch, _native as nat
from tt_sketch_amd.device import DevArray, contract
from tt_sketch_amd.sketch_dispatch import SketchMethod, general_sketch_device

WARM = 3
N_CHUNK = 512          # CP_N_CHUNK of csrc/cp_pass_plan.h


def timed(fn):
    nat.call("ttsk_timer_start", 0)
    fn()
    ms = ctypes.c_float()
    nat.call("ttsk_timer_stop", 0, ctypes.byref(ms))
    return float(ms.value)


def measure(variants, reps):
    times = {k: [] for k, _ in variants}
    for rep in range(WARM + reps):
        for k, fn in variants:
            ms = timed(fn)
            if rep >= WARM:
                times[k].append(ms)
    out = {}
    for k, _ in variants:
        t = np.array(times[k])
        out[k] = dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()), reps=len(t))
        print(f"  {k:18s} median {np.median(t):9.3f} ms  (min {t.min():.3f} .. max {t.max():.3f}, {len(t)} reps)")
    return out


def dev(rng, shape, scale=1.0):
    return DevArray.from_host(rng.standard_normal(shape) * scale)


def kernel_line(name, ms, flops, nbytes, peak):
    tf = flops / ms / 1e9
    print(f"  {name}: {flops / 1e9:.3f} GF, {nbytes / 1e6:.1f} MB -> {tf:.2f} TF/s = {100 * tf / peak:.1f} % of the fp64 MFMA probe, "
          f"{nbytes / ms / 1e9:.3f} TB/s of algorithmic bytes")
    return dict(flops=flops, bytes=nbytes, tflops=tf, share_of_peak=tf / peak, tb_per_s=nbytes / ms / 1e9)


def case(name, d, n, N, l, r, reps, peak):
    rng = np.random.default_rng(25)
    shape = (n,) * d
    print(f"\n({name}) d = {d}, n = {n}, N = {N}, l = {l}, r = {r}")
    tensor = CPTensor([dev(rng, (n, N), 1.0 / np.sqrt(n)) for _ in range(d)])
    left = TensorTrainDRM(l, shape, transpose=False, seed=1)
    right = TensorTrainDRM(r, shape, transpose=True, seed=2)
    rec = dict(case=name, d=d, n=n, N=N, l=l, r=r)

    # ---- the whole sketch
    got = {}

    def sk_composed():
        with cp_fused.forced("composed"):
            got["composed"] = stream_sketch(tensor, left.rank, right.rank[::-1], left_drm=left, right_drm=right)

    def sk_kernel():
        with cp_fused.forced("kernel"):
            got["kernel"] = stream_sketch(tensor, left.rank, right.rank[::-1], left_drm=left, right_drm=right)

    def dev_composed():
        with cp_fused.forced("composed"):
            general_sketch_device(tensor, left, right, SketchMethod.streaming)

    def dev_kernel():
        assert cp_fused.try_cp_sketch(tensor, left, right, SketchMethod.streaming, route="kernel") is not None

    rec["sketch_ms"] = measure([("composed", sk_composed), ("kernel", sk_kernel), ("composed_device", dev_composed),
                                ("kernel_device", dev_kernel)], reps)
    a, b = got["kernel"], got["composed"]
    gap = max(float(np.linalg.norm(x - y) / np.linalg.norm(y)) for x, y in zip(a.Psi_cores + a.Omega_mats, b.Psi_cores + b.Omega_mats))
    rec["max_rel_gap"] = gap
    print(f"  largest relative gap between the two sketches {gap:.2e}")

    # ---- the entries alone, at a middle mode
    V = tensor.dev_cores()[d // 2]
    rec["chain"] = {}
    for side, rho in (("left", l), ("right", r)):
        L, D = dev(rng, (N, rho), 1.0 / np.sqrt(rho)), dev(rng, (rho, n, rho), 1.0 / np.sqrt(rho * n))

        def kern():
            assert cp_fused.chain_step(L, V, D, route="kernel") is not None

        def comp():
            W = contract("ij,jkl->ikl", L, D)
            contract("ki,ikl->il", V, W)

        print(f" chain step, {side}: rho = rho' = {rho}")
        ms = measure([("kernel", kern), ("composed", comp)], reps)
        flops = 2.0 * N * rho * n * rho
        nbytes = 8.0 * (N * rho + N * n + rho * n * rho + N * rho)
        rec["chain"][side] = dict(ms=ms, kernel=kernel_line("cp_chain_kernel", ms["kernel"]["median"], flops, nbytes, peak))
    L, R, Ro = dev(rng, (N, l), 1.0 / np.sqrt(l)), dev(rng, (N, r), 1.0 / np.sqrt(r)), dev(rng, (N, r), 1.0 / np.sqrt(r))

    def psi_om_kernel():
        assert cp_fused.psi_omega(L, R, V, R_om=Ro, psi=True, omega=True, route="kernel") is not None

    def psi_om_composed():
        W = contract("kj,jm->jkm", V, R)
        contract("ji,jkm->ikm", L, W)
        contract("ji,jk->ik", L, Ro)

    def psi_kernel():
        assert cp_fused.psi_omega(L, R, V, route="kernel") is not None

    def psi_composed():
        W = contract("kj,jm->jkm", V, R)
        contract("ji,jkm->ikm", L, W)

    print(f" Psi and Omega: l = {l}, r = {r}")
    ms = measure([("kernel", psi_om_kernel), ("composed", psi_om_composed), ("kernel_psi_alone", psi_kernel),
                  ("composed_psi_alone", psi_composed)], reps)
    cols, chunks = n * r + r, -(-N // N_CHUNK)
    flops = 2.0 * l * N * cols
    ws = 8.0 * chunks * l * cols if chunks > 1 else 0.0
    nbytes = 8.0 * (N * l + 2 * N * r + N * n + l * cols) + 2 * ws
    rec["psi_omega"] = dict(ms=ms, chunks=chunks, workspace_bytes=ws,
                            kernel=kernel_line("cp_psi_kernel (+ closing sum)", ms["kernel"]["median"], flops, nbytes, peak))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--cases", default="forest,cp_tensor")
    ap.add_argument("--reps", type=int, default=21)
    args = ap.parse_args()
    nat.call("ttsk_init", 0)
    probe = ctypes.c_double()
    nat.call("ttsk_mfma_f64_peak_probe", ctypes.byref(probe))
    print(f"fp64 MFMA probe {probe.value:.1f} TF/s")
    recs = []
    if "forest" in args.cases:
        recs.append(case("forest", 8, 12, 25000, 50, 100, args.reps, probe.value))
    if "cp_tensor" in args.cases:
        recs.append(case("cp_tensor", 5, 10, 100, 30, 60, args.reps, probe.value))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(mfma_f64_probe_tflops=probe.value, cases=recs), f, indent=1)


if __name__ == "__main__":
    main()
