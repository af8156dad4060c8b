"""Times the inner products of operator-times-train products that are never formed (operator_gram.py, ttsk_op_close), with
device events on library stream 0.  Every case is a child process of its own under its own time limit; the first one that
fails ends the run.

Step B alone, G' (P, s' S') from Wl (s S, n, P) of one interior mode with P = R' r' (B1 the TT-GMRES shape, B2 the wide
shape of operator_sketch_bench.py; the second product has the ranks of the first):

  kernel     op_close(..., route="kernel"): one ttsk_op_close call (T1 stays on the chip, nothing indexed by j is written)
             and the ttsk_sum_slices behind it
  composed   op_close(..., route="composed"): two `contract` calls with T1 (s, P, n, S') through HBM, a copy of T1 that puts
             j next to c, and a strided copy that puts c' first

End to end, ||A_0 x|| = OperatorProduct(A_0, x).norm() and the true residual A.residual(x, b) of a sum of three operators
(E1, E2 at the same two shapes):

  rule       half B as the routing rule of operator_gram.close_route_ms has it
  kernel     the same with ttsk_op_close at every mode (paths.forced("kernel"), which forces half A too)
  composed   the same with the compositions at every mode
  explicit   the only path of the parent commit: the products formed with mpo(tt) on resident cores, then tt_gram on those
             trains (and b); the formation is inside the timed region

The variants are alternated, REPS timed repetitions after WARM warm-up rounds; median and spread (min .. max).  A timed
region of step B alone holds INNER calls, so that it is not the clock that is measured; the figure is per call.

    python profiles/scripts/operator_gram_bench.py [--json out.json] [--cases B1,B2,E1,E2] [--reps 9]
"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np

from hadamard_gram_bench import apart, measure, normal, random_tt

CASES = {          # name: (kind, d, n, train rank, operator rank, maps, seconds allowed)
    "B1": ("close", 8, 20, 20, 4, 3, 120),
    "B2": ("close", 6, 100, 64, 8, 3, 180),
    "E1": ("whole", 8, 20, 20, 4, 3, 240),
    "E2": ("whole", 6, 100, 64, 8, 3, 420),
}


def close_case(name, n, s, S, reps, inner):
    from tt_sketch_amd import operator_gram as og
    P = S * s
    Wl = normal((s * S, n, P), 1, 1.0 / np.sqrt(s * S * n))
    N = normal((S, n, n, S), 2).transpose(0, 2, 1, 3)             # packed: (gamma, i) one run
    Y = normal((s, n, s), 3)
    got = {}

    def kernel():
        got["kernel"] = og.op_close(Wl, N, Y, route="kernel")

    def composed():
        got["composed"] = og.op_close(Wl, N, Y, route="composed")

    fl = 2.0 * n * P * S * (s * S * n + s * s)
    jchunks, slab = og.close_layout(S, S, s, s, n, n, P)
    print(f"\n({name}) step B alone: S = {S}, s = {s}, n = {n}, P = {P}: {fl / 1e9:.3f} GF, Wl of {s * S * n * P * 8 / 1e6:.1f} MB, "
          f"{jchunks} chunks of j, a slab of {slab * 8 / 1e6:.1f} MB", flush=True)
    ms = measure([("kernel", kernel), ("composed", composed)], reps, inner)
    a, b = got["kernel"].get().ravel(), got["composed"].get().ravel()
    model = og.close_route_ms(S, S, s, s, n, n, P)
    k, c = ms["kernel"], ms["composed"]
    rec = dict(case=name, S=S, S1=S, s=s, s1=s, n_in=n, n_out=n, P=P, flops=fl, jchunks=jchunks, kernel_ms=k, composed_ms=c, apart=apart(k, c),
               faster="kernel" if k[0] < c[0] else "composed", kernel_tflops=fl / k[0] / 1e9, composed_tflops=fl / c[0] / 1e9,
               max_rel_gap=float(np.max(np.abs(a - b)) / np.max(np.abs(b))), model_ms=dict(kernel=model[0], composed=model[1]),
               route="composed" if model[1] < model[0] else "kernel", reps=reps, inner=inner)
    print(f"  kernel {rec['kernel_tflops']:.2f} TF/s, composed {rec['composed_tflops']:.2f} TF/s; composed / kernel = {c[0] / k[0]:.2f}, "
          f"ranges apart: {rec['apart']}; largest gap {rec['max_rel_gap']:.1e}; rule: kernel {model[0]:.3f} ms, composed {model[1]:.3f} ms -> {rec['route']}",
          flush=True)
    return rec


def whole_case(name, d, n, r, R, maps, reps):
    from tt_sketch_amd import OperatorProduct, paths
    from tt_sketch_amd.tensor_gram import tt_gram
    from tt_sketch_amd.tt_gmres import MPO, TTLinearMapSum
    shape = (n,) * d
    rk = (1,) + (R,) * (d - 1) + (1,)
    ops = [MPO([normal((rk[k], n, n, rk[k + 1]), 100 * p + k, 1.0 / np.sqrt(rk[k] * n)) for k in range(d)]) for p in range(maps)]
    x, b = random_tt(10, shape, r), random_tt(30, shape, r)
    A = TTLinearMapSum(ops)
    core_gb = (R * r) ** 2 * n * 8 / 1e9
    print(f"\n({name}) shape {shape}, train rank {r}, {maps} operators of rank {R}: product rank {R * r}, an explicit core {core_gb:.3f} GB", flush=True)
    rec = dict(case=name, shape=list(shape), r=r, R=R, maps=maps, explicit_core_gb=core_gb, reps=reps)

    def explicit_norm():
        t = ops[0](x)
        return float(np.sqrt(abs(tt_gram([t])[0, 0])))

    def explicit_residual():
        G = tt_gram([m(x) for m in ops] + [b])
        c = np.array([-1.0] * maps + [1.0])
        return float(np.sqrt(max(c @ G @ c, 0.0)))

    for what, lazy, explicit in (("norm", lambda: OperatorProduct(ops[0], x).norm(), explicit_norm),
                                 ("residual", lambda: A.residual(x, b), explicit_residual)):
        def routed(route, fn=lazy):
            def run():
                with paths.forced(route):
                    return fn()
            return run
        print(f" {what}:", flush=True)
        ms = measure([("rule", routed(None)), ("kernel", routed("kernel")), ("composed", routed("composed")), ("explicit", explicit)], reps)
        with paths.forced("kernel"):
            a = lazy()
        with paths.forced("composed"):
            c2 = lazy()
        c = explicit()
        rec[what] = dict(ms=ms, value=a, rel_diff_routes=abs(a - c2) / abs(a), rel_diff_explicit=abs(a - c) / abs(c),
                         speedup_rule_over_explicit=ms["explicit"][0] / ms["rule"][0], apart_rule_explicit=apart(ms["rule"], ms["explicit"]))
        print(f"  explicit / rule = {rec[what]['speedup_rule_over_explicit']:.2f}, ranges apart: {rec[what]['apart_rule_explicit']}; kernel against "
              f"composed {rec[what]['rel_diff_routes']:.1e}, lazy against explicit {rec[what]['rel_diff_explicit']:.1e}", flush=True)
    return rec


def one_case(name, reps):
    from tt_sketch_amd import _native as nat
    nat.call("ttsk_init", 0)
    kind, d, n, r, R, maps, _ = CASES[name]
    if kind == "close":
        return close_case(name, n, r, R, reps, 10 if name == "B1" else 3)
    return whole_case(name, d, n, r, R, maps, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--cases", default="B1,B2,E1,E2")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--child", help="run this one case here and write its record to --json")
    args = ap.parse_args()
    if args.child:
        rec = one_case(args.child, args.reps)
        with open(args.json, "w") as f:
            json.dump(rec, f)
        return 0
    alone, whole, unmeasured = [], [], []
    names = args.cases.split(",")
    part = (args.json or "operator_gram_bench.json") + ".part"
    for k, name in enumerate(names):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(args.reps), "--json", part]
        try:
            status = subprocess.run(cmd, timeout=CASES[name][6]).returncode       # the child prints as it goes
        except subprocess.TimeoutExpired:
            status = f"past its {CASES[name][6]} s"
        if status != 0:
            print(f"({name}) ended with status {status}: the run ends here", flush=True)
            unmeasured += names[k:]
            break
        with open(part) as f:
            (alone if CASES[name][0] == "close" else whole).append(json.load(f))
        os.remove(part)
    if args.json:
        from tt_sketch_amd import hadamard_gram as hg, operator_gram as og
        rule = dict(floor_ms=og._CLOSE_FLOOR_MS, kernel_tflops=og._CLOSE_TFLOPS, launch_ms=og._CLOSE_LAUNCH_MS,
                    composed_launches=og._CLOSE_COMPOSED_LAUNCHES, gemm_tflops=og._CLOSE_GEMM_TFLOPS, w_budget_bytes=hg.W_BUDGET_BYTES)
        with open(args.json, "w") as f:
            json.dump(dict(close_alone=alone, end_to_end=whole, unmeasured=unmeasured, rule_when_run=rule), f, indent=1)
    return 1 if unmeasured else 0


if __name__ == "__main__":
    sys.exit(main())
