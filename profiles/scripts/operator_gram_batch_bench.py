"""Times the Gram matrix of operator-times-train products in which every pair advances through a mode together
(operator_gram.op_gram, ttsk_op_close_batch), with device events on library stream 0.  Every case is a
child process of its own under its own time limit; the first one that fails ends the run.

Half B alone (C1: the nine pairs of the residual of three operators at the TT-GMRES shape, six product pairs and three
products against the train b as degenerate pairs), every Wl a column slice of one W:

  batched    close_batch: ONE ttsk_op_close_batch call
  single     nine op_close(..., route="kernel") calls on contiguous copies of the same Wl

Closing against a train alone (T1, T2: the three pairs <A_p x, b> of that residual at the two shapes), every Wl a column
slice of one W (s, n, 3 P):

  batched    close_batch of the three degenerate pairs (N = the core of b viewed as an operator core, Y = 1): one call
  contract   three `contract` calls on the same slices, as op_tt_dot closes a mode

End to end, the true residual of a sum of three operators (R1 the TT-GMRES shape, R2 the wide shape):

  batched    A.residual(x, b): one symmetric op_gram of the A_p x and b, half B as the routing rule has it
  kernel     the same with every pair in the batch (paths.forced("kernel")); R1 only
  per_pair   the parent commit's path: ten dot calls, one chain and one read-back each (tt_gmres._residual_squares)
  explicit   the products formed with mpo(tt) on resident cores, then one tt_gram; the formation is inside the timed region
  gram       op_gram of the four members alone, without the arithmetic of the residual

The variants are alternated, REPS timed repetitions after WARM warm-up rounds; median and spread (min .. max).

    python profiles/scripts/operator_gram_batch_bench.py [--json out.json] [--cases C1,T1,T2,R1,R2] [--reps 9]
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
    "C1": ("close", 8, 20, 20, 4, 3, 120),
    "T1": ("close_train", 8, 20, 20, 4, 3, 120),
    "T2": ("close_train", 6, 100, 64, 8, 3, 180),
    "R1": ("whole", 8, 20, 20, 4, 3, 240),
    "R2": ("whole", 6, 100, 64, 8, 3, 420),
}


def close_case(name, n, s, S, maps, reps, inner):
    from tt_sketch_amd import operator_gram as og
    from tt_sketch_amd.operator_product import chain_start
    P = S * s
    shapes = [(S, s, n)] * (maps * (maps + 1) // 2) + [(s, 1, 1)] * maps           # (S, s, n_in) of the right side of every pair
    W = normal((max(a * b for a, b, _ in shapes), n, len(shapes) * P), 1, 1.0 / np.sqrt(s * S * n))
    Wls = [W[:a * b, :, k * P:(k + 1) * P] for k, (a, b, _) in enumerate(shapes)]
    copies = [w.contiguous() for w in Wls]
    Ns = [normal((a, n, n_in, a), 2 + k).transpose(0, 2, 1, 3) for k, (a, _, n_in) in enumerate(shapes)]
    Ys = [normal((b, n_in, b), 40 + k) if b > 1 else chain_start() for k, (_, b, n_in) in enumerate(shapes)]
    outs = [og.DevArray.empty((P, a * b)) for a, b, _ in shapes]
    alone = [og.DevArray.empty((P, a * b)) for a, b, _ in shapes]

    def batched():
        og.close_batch(Wls, Ns, Ys, outs)

    def single():
        for w, N, Y, o in zip(copies, Ns, Ys, alone):
            og.op_close(w, N, Y, out=o, route="kernel")

    print(f"\n({name}) half B alone: {len(shapes)} pairs at S = {S}, s = {s}, n = {n}, P = {P}", flush=True)
    ms = measure([("batched", batched), ("single", single)], reps, inner)
    same = all(np.array_equal(a.get(), b.get()) for a, b in zip(outs, alone))
    k, c = ms["batched"], ms["single"]
    rec = dict(case=name, pairs=len(shapes), S=S, s=s, n=n, P=P, batched_ms=k, single_ms=c, apart=apart(k, c), same_bits=bool(same), reps=reps, inner=inner)
    print(f"  single / batched = {c[0] / k[0]:.2f}, ranges apart: {rec['apart']}; the same bits: {same}", flush=True)
    return rec


def close_train_case(name, n, s, S, maps, reps, inner):
    from tt_sketch_amd import operator_gram as og
    from tt_sketch_amd.device import contract
    from tt_sketch_amd.operator_product import chain_start
    P = S * s
    W = normal((s, n, maps * P), 1, 1.0 / np.sqrt(s * n))
    Wls = [W[:, :, k * P:(k + 1) * P] for k in range(maps)]
    Z = normal((s, n, s), 2)
    Ns, Ys = [Z.reshape(s, 1, n, s)] * maps, [chain_start()] * maps
    outs = [og.DevArray.empty((P, s)) for _ in range(maps)]
    alone = [og.DevArray.empty((P, s)) for _ in range(maps)]

    def batched():
        og.close_batch(Wls, Ns, Ys, outs)

    def contracts():
        for w, o in zip(Wls, alone):
            contract("gip,gih->ph", w, Z, out=o)

    print(f"\n({name}) closing against a train alone: {maps} pairs at s = {s}, n = {n}, P = {P}", flush=True)
    ms = measure([("batched", batched), ("contract", contracts)], reps, inner)
    gap = max(float(np.max(np.abs(a.get() - b.get())) / np.max(np.abs(b.get()))) for a, b in zip(outs, alone))
    model, riding = og.tt_close_route_ms(s, s, n, P, alone=True), og.tt_close_route_ms(s, s, n, P)
    k, c = ms["batched"], ms["contract"]
    rec = dict(case=name, pairs=maps, s=s, n=n, P=P, batched_ms=k, contract_ms=c, apart=apart(k, c), max_rel_gap=gap,
               model_ms_per_pair_alone=dict(batch=model[0], contract=model[1]), model_ms_per_pair_riding=dict(batch=riding[0], contract=riding[1]),
               reps=reps, inner=inner)
    print(f"  contract / batched = {c[0] / k[0]:.2f}, ranges apart: {rec['apart']}; largest gap {gap:.1e}; rule per pair: alone in the batch {model[0]:.4f} ms, "
          f"riding {riding[0]:.4f} ms, contract {model[1]:.4f} ms", flush=True)
    return rec


def whole_case(name, d, n, r, R, maps, reps):
    from tt_sketch_amd import OperatorProduct, operator_gram as og, paths
    from tt_sketch_amd.tensor_gram import tt_gram
    from tt_sketch_amd.tt_gmres import MPO, TTLinearMapSum, _residual_squares
    shape = (n,) * d
    rk = (1,) + (R,) * (d - 1) + (1,)
    ops = [MPO([normal((rk[k], n, n, rk[k + 1]), 100 * p + k, 1.0 / np.sqrt(rk[k] * n)) for k in range(d)]) for p in range(maps)]
    x, b = random_tt(10, shape, r), random_tt(30, shape, r)
    A = TTLinearMapSum(ops)
    print(f"\n({name}) shape {shape}, train rank {r}, {maps} operators of rank {R}: product rank {R * r}", flush=True)

    def per_pair():
        total, _ = _residual_squares([OperatorProduct(m, x) for m in ops], b)
        return float(np.sqrt(max(total, 0.0)))

    def explicit():
        G = tt_gram([m(x) for m in ops] + [b])
        c = np.array([-1.0] * maps + [1.0])
        return float(np.sqrt(max(c @ G @ c, 0.0)))

    def kernel():
        with paths.forced("kernel"):
            return A.residual(x, b)

    variants = [("batched", lambda: A.residual(x, b)), ("per_pair", per_pair), ("explicit", explicit),
                ("gram", lambda: og.op_gram([OperatorProduct(m, x) for m in ops] + [b]))]
    if name == "R1":
        variants.insert(1, ("kernel", kernel))
    ms = measure(variants, reps)
    a, p, e = A.residual(x, b), per_pair(), explicit()
    rec = dict(case=name, shape=list(shape), r=r, R=R, maps=maps, reps=reps, ms=ms, value=a, rel_diff_per_pair=abs(a - p) / abs(p),
               rel_diff_explicit=abs(a - e) / abs(e), per_pair_over_batched=ms["per_pair"][0] / ms["batched"][0],
               apart_batched_per_pair=apart(ms["batched"], ms["per_pair"]), explicit_over_batched=ms["explicit"][0] / ms["batched"][0],
               apart_batched_explicit=apart(ms["batched"], ms["explicit"]))
    print(f"  per pair / batched = {rec['per_pair_over_batched']:.2f}, ranges apart: {rec['apart_batched_per_pair']}; explicit / batched = "
          f"{rec['explicit_over_batched']:.2f}, ranges apart: {rec['apart_batched_explicit']}; batched against per pair {rec['rel_diff_per_pair']:.1e}, "
          f"against explicit {rec['rel_diff_explicit']:.1e}", flush=True)
    return rec


def one_case(name, reps):
    from tt_sketch_amd import _native as nat
    nat.call("ttsk_init", 0)
    kind, d, n, r, R, maps, _ = CASES[name]
    if kind == "close":
        return close_case(name, n, r, R, maps, reps, 10)
    if kind == "close_train":
        return close_train_case(name, n, r, R, maps, reps, 10 if name == "T1" else 3)
    return whole_case(name, d, n, r, R, maps, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--cases", default="C1,T1,T2,R1,R2")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--child", help="run this one case here and write its record to --json")
    args = ap.parse_args()
    if args.child:
        rec = one_case(args.child, args.reps)
        with open(args.json, "w") as f:
            json.dump(rec, f)
        return 0
    alone, train, whole, unmeasured = [], [], [], []
    names = args.cases.split(",")
    part = (args.json or "operator_gram_batch_bench.json") + ".part"
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
            dict(close=alone, close_train=train, whole=whole)[CASES[name][0]].append(json.load(f))
        os.remove(part)
    if args.json:
        from tt_sketch_amd import hadamard_gram as hg, operator_gram as og
        rule = dict(floor_ms=og._CLOSE_FLOOR_MS, kernel_tflops=og._CLOSE_TFLOPS, launch_ms=og._CLOSE_LAUNCH_MS,
                    composed_launches=og._CLOSE_COMPOSED_LAUNCHES, gemm_tflops=og._CLOSE_GEMM_TFLOPS, w_budget_bytes=hg.W_BUDGET_BYTES,
                    max_pairs=og.MAX_PAIRS)
        with open(args.json, "w") as f:
            json.dump(dict(close_alone=alone, close_train=train, residual=whole, unmeasured=unmeasured, rule_when_run=rule), f, indent=1)
    return 1 if unmeasured else 0


if __name__ == "__main__":
    sys.exit(main())
