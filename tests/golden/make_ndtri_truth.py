"""Generate tests/golden/ndtri_truth.npz: the crafted uniforms of tests/test_gpu_ndtri_edges.py and their TRUE
normal quantiles, sqrt(2) erfinv(2 u - 1) with mpmath at 50 digits, rounded to double.

    python tests/golden/make_ndtri_truth.py

Needs mpmath (no test imports it) and the oracle's C library.  Numbers only: the mantissas
k (u = k / 2^52), the quantiles, the quantile at 2^-53 (what the fill kernels put in the place of u == 0) and E_ref,
the largest error in ulp of the oracle's Cephes ndtri against the truth over this same set -- the GPU test asserts
device error <= E_ref + ULP_BAR, tests/test_gpu_ndtri_edges.py::test_oracle_ndtri_against_truth_fixture asserts the
oracle at E_ref, so a stale fixture is noticed without a GPU.

The set: 0; 1, 2, 3; 55..59 (exp(-32) 2^52 = 57.03: the last
far-tail and the first near-tail value); 2^52 - 59 .. 2^52 - 1; two mantissas on each side of exp(-2) and of
1 - exp(-2); 2^51 - 1, 2^51, 2^51 + 1; both sides of every switch of the device's own logarithm (first logarithm:
argument mantissa at sqrt 2, i.e. y = sqrt(2) 2^-j; second logarithm: x = sqrt(-2 log y) at 2 sqrt 2 and 4 sqrt 2,
found by bisection on the oracle's x), each with its mirror 1 - u; a log-spaced ladder of 200 values from 2^-52 to
exp(-2) and its mirror; 1000 random mantissas as control.
"""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import mpmath as mp  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

ge.build_oracle()
from oracle import ttsk_oracle as orc  # noqa: E402

TWO52 = 1 << 52
EXPM2 = 0.13533528323661269189          # the constant of Cephes ndtri (and of every device copy of the split)


def oracle_x(k: int) -> float:
    """x = sqrt(-2 log u) as the oracle's ndtri forms it for the tail sample u = k / 2^52 (u <= exp(-2))"""
    return math.sqrt(-2.0 * math.log(k / TWO52))


def last_k_with_x_at_least(x_switch: float) -> int:
    lo, hi = 1, int(EXPM2 * TWO52)       # x decreases with k: x(lo) >= x_switch > x(hi)
    assert oracle_x(lo) >= x_switch > oracle_x(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if oracle_x(mid) >= x_switch:
            lo = mid
        else:
            hi = mid
    return lo


def input_set():
    lower = {1, 2, 3} | set(range(55, 60))
    k0 = int(math.floor(EXPM2 * TWO52))                   # exp(-2) lies in (k0, k0 + 1) / 2^52
    lower |= {k0 - 1, k0, k0 + 1, k0 + 2}
    k1 = int(math.floor((1.0 - EXPM2) * TWO52))
    upper = {k1 - 1, k1, k1 + 1, k1 + 2} | set(range(TWO52 - 59, TWO52))
    switches = {}
    for j in range(4, 53):                                # first logarithm: y = sqrt(2) 2^-j, j = 4 (0.088) .. 52
        s = math.sqrt(2.0) * 2.0 ** (52 - j)
        ks = {int(math.floor(s)), int(math.floor(s)) + 1}
        switches[f"log(y): y mantissa at sqrt 2, y = sqrt(2) 2^-{j}"] = sorted(ks)
        lower |= ks
    for name, xs in (("2 sqrt 2", 2.0 * math.sqrt(2.0)), ("4 sqrt 2", 4.0 * math.sqrt(2.0))):
        k = last_k_with_x_at_least(xs)                    # device and oracle x may differ in the last bit: two on each side
        ks = {k - 1, k, k + 1, k + 2}
        switches[f"log(x): x at {name}"] = sorted(ks)
        lower |= ks
    ladder = np.unique(np.round(np.exp(np.linspace(math.log(2.0 ** -52), math.log(EXPM2), 200)) * TWO52).astype(np.int64))
    lower |= {int(k) for k in ladder if 1 <= k <= k0}
    upper |= {TWO52 - k for k in lower}
    rng = np.random.default_rng(20240521)
    control = {int(k) for k in rng.integers(1, TWO52, 1000)}
    mants = sorted({0, (1 << 51) - 1, 1 << 51, (1 << 51) + 1} | lower | upper | control)
    return np.array(mants, dtype=np.uint64), switches, k0, k1


def truth(u) -> float:
    return float(mp.sqrt(2) * mp.erfinv(2 * mp.mpf(u) - 1))


def ulp_err(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def main():
    mp.mp.dps = 50
    mants, switches, k0, k1 = input_set()
    u = mants.astype(np.float64) * 2.0 ** -52
    assert np.array_equal((u * 2.0 ** 52).astype(np.uint64), mants)
    val = np.array([-np.inf if k == 0 else truth(mp.mpf(int(k)) / TWO52) for k in mants])
    t53 = truth(mp.mpf(2) ** -53)
    # the same quantile by another route at the ends, where erfinv works hardest: the root of erfc at 80 digits
    mp.mp.dps = 80
    for k in (1, 57, 58, TWO52 - 57, TWO52 - 1):
        i = int(np.searchsorted(mants, k))
        x = mp.findroot(lambda t: mp.erfc(-t / mp.sqrt(2)) / 2 - mp.mpf(k) / TWO52, val[i])
        assert float(x) == val[i], k
    mp.mp.dps = 50
    fin = mants != 0
    ora = orc.ndtri(u)
    assert ora[~fin][0] == -np.inf
    err = ulp_err(ora[fin], val[fin])
    e53 = float(ulp_err(orc.ndtri(np.array([2.0 ** -53])), np.array([t53]))[0])
    e_ref = max(float(err.max()), e53)
    worst = mants[fin][int(err.argmax())]
    print(f"{mants.size} mantissas; E_ref = {e_ref:.3f} ulp (at k = {worst}); oracle at 2^-53: {e53:.3f} ulp")
    far = (mants[fin] <= 57) | (mants[fin] >= TWO52 - 57)
    print(f"  far tail: {err[far].max():.3f}   rest: {err[~far].max():.3f}")

    at = {int(k): i for i, k in enumerate(mants)}

    def signed(k):
        return (ora[at[k]] - val[at[k]]) / np.spacing(abs(val[at[k]]))
    print("signed oracle error (ulp) on either side of each branch point:")
    ylog = {n: ks for n, ks in switches.items() if n.startswith("log(y)")}
    for name, ks in [("x = 8 (far / near tail)", [55, 56, 57, 58, 59]), ("mirror of x = 8", [TWO52 - k for k in (55, 56, 57, 58, 59)]),
                     ("exp(-2)", [k0 - 1, k0, k0 + 1, k0 + 2]), ("1 - exp(-2)", [k1 - 1, k1, k1 + 1, k1 + 2])] + \
            [(n, ks) for n, ks in switches.items() if n not in ylog]:
        print(f"  {name}: " + "  ".join(f"{k}: {signed(k):+.2f}" for k in ks))
    jumps = [abs(signed(ks[1]) - signed(ks[0])) for ks in ylog.values()]
    print(f"  log(y), y mantissa at sqrt 2 ({len(ylog)} switches, y = sqrt(2) 2^-4 .. 2^-52): largest jump {max(jumps):.2f}")
    np.savez(os.path.join(HERE, "ndtri_truth.npz"), mantissa=mants, truth=val, truth_2m53=np.float64(t53),
             e_ref=np.float64(e_ref))


if __name__ == "__main__":
    main()
