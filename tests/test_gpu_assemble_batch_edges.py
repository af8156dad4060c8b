"""ttsk_tt_assemble_batch (csrc/assemble_batch.hip, behind to_tt_batch) at every edge of its host plan, element by element.

The cases, their operands, the truth and the checks are those of tests/assemble_batch_ref.py (read its docstring);
tests/test_assemble_batch_cover.py shows without a GPU that each case reaches the plan fields it is tagged with, that the
tags cover every branch, that the checks reject a result with one seeded defect, and that the poison batch dominates every
case.  Here every case runs through the C entry point, in an integer and a Gaussian pass:

- poison: the same entry point first runs POISON, a larger batch whose operands are scaled by 2^300 -- every staging
  region then holds values hundreds of binary orders off wherever a case may read what it did not write itself;
- integer pass: on the covered path P read back from `work` and C EQUAL the dyadic truth bit for bit;
- Gaussian pass: P by the one rule of tests/test_gpu_solve_edges.py, every element of C within the derived bound of the
  long-double refined product of the P read back; the refine cases also against 8 e_lapack, the robust case's two
  matrices at the stable bar, its neighbours with the bits they have in a batch without the two;
- every guard word around C and `work` still holds the sentinel, the operands (the aliased copied core among them) read
  back bit-identical, a second call on fresh sentinel buffers gives the same bits.

Argument errors must return TTSK_ERR_ARG and write nothing."""
import ctypes

import numpy as np
import pytest

from tests import assemble_batch_ref as ref
from tests.edge_kit import assert_bits_equal, nat, run_entry, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
CASES = ref.cases()
WORST = {}


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratios():
    yield
    print("\n[assemble batch edges] largest err / bar over all cases:")
    for k in sorted(WORST):
        print("  %-10s %.3g  at %s" % (k, WORST[k][0], WORST[k][1]))


def entry_args(c, ptr, **change):
    psi, om, cores, work = ref.pointer_table(c, ptr)
    arr = lambda v: (P * max(len(v), 1))(*v)
    a = dict(count=c.count, d=c.d, n=c.n, lr=c.lr, rr=c.rr, psi=arr(psi), om=arr(om), cores=arr(cores), work=arr(work), direction=c.direction)
    a.update(change)
    i64 = lambda v: (ctypes.c_int64 * max(len(v), 1))(*v)
    return [a["count"], a["d"], i64(a["n"]), i64(a["lr"]), i64(a["rr"]), a["psi"], a["om"], a["cores"], a["work"], a["direction"], 0]


def run(nat, what, args):
    run_entry(nat, "ttsk_tt_assemble_batch", args, what)


class Device:
    """the operands of one (case, pass) on the device; call() runs the entry point on fresh sentinel buffers"""

    def __init__(self, nat, c, vals):
        from tt_sketch_amd.device import DevArray
        self.nat, self.c = nat, c
        self.host = ref.arenas_in(c, vals)
        self.dev = {n: DevArray.from_host(h) for n, h in self.host.items()}

    def call(self):
        """-> host images of the output arenas after the call"""
        from tt_sketch_amd.device import DevArray
        dO = {n: DevArray.from_host(h) for n, h in ref.arenas_out(self.c).items()}
        ptr = {n: d.ptr for n, d in list(self.dev.items()) + list(dO.items())}
        assert all(p % 8 == 0 for p in ptr.values())
        run(self.nat, self.c.id, entry_args(self.c, ptr))
        return {n: d.get() for n, d in dO.items()}

    def operands_untouched(self, what):
        for n, h in self.host.items():
            assert_bits_equal(self.dev[n], h, "%s: %s" % (what, n))


@pytest.fixture(scope="module")
def poison(nat):
    c = ref.POISON
    dev = Device(nat, c, ref.values(c, "gaussian", 99, scale=ref.POISON_SCALE))
    from tt_sketch_amd.device import DevArray
    outs = {n: DevArray.from_host(h) for n, h in ref.arenas_out(c).items()}
    args = entry_args(c, {n: d.ptr for n, d in list(dev.dev.items()) + list(outs.items())})

    def call(_held=(dev, outs)):             # the addresses in `args` are theirs: they live as long as the calls
        run(nat, c.id, args)
    return call


def one_pass(nat, poison, c, mode, seed):
    """poison, call, check, call again, compare; -> (the check's worst ratios, the output arenas)"""
    what = "%s %s" % (c.id, mode)
    vals = ref.values(c, mode, seed)
    dev = Device(nat, c, vals)
    poison()
    out = dev.call()
    worst = ref.check_results(c, vals, out, mode, what)
    again = dev.call()
    same_bits(again, out, what + ", second call")
    dev.operands_untouched(what)
    return worst, out


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_assemble_batch_edge_case(nat, poison, c):
    seed = 11
    one_pass(nat, poison, c, "integer", seed)
    mode = ref.gaussian_mode(c)
    worst, out = one_pass(nat, poison, c, mode, seed)
    for k, v in worst.items():
        if v > WORST.get(k, (-1.0, None))[0]:
            WORST[k] = (v, c.id)
    print("[assemble batch edges] %s: largest err / bar, %s pass: %s" % (c.id, mode, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))
    if mode == "robust":
        # the same batch with benign Omegas in place of the two: tensors 0 and 3 keep their bits
        vals, benign = ref.values(c, "robust", seed), ref.values(c, "benign", seed)
        for name in vals:
            if name.startswith("psi"):
                benign[name] = vals[name]
            elif name.startswith("om"):
                benign[name] = {s: (benign if s in (1, 2) else vals)[name][s] for s in vals[name]}
        dev = Device(nat, c, benign)
        poison()
        other = dev.call()
        ref.check_results(c, benign, other, "gaussian", c.id + " benign")
        for name in out:
            for b in (0, 3):
                o, sz = ref.place(c, name, b)
                same_bits(out[name][o:o + sz], other[name][o:o + sz], "%s: tensor %d of %s changes with its neighbours' route:" % (c.id, b, name))


@pytest.mark.parametrize("what", ref.ARG_ERRORS)
def test_argument_errors_write_nothing(nat, what):
    from tt_sketch_amd.device import DevArray
    c = ref.by_id("pad-3x5-R")
    dev = Device(nat, c, ref.values(c, "gaussian", 5))
    dO = {n: DevArray.from_host(h) for n, h in ref.arenas_out(c).items()}
    ptr = {n: d.ptr for n, d in list(dev.dev.items()) + list(dO.items())}
    psi, om, cores, work = ref.pointer_table(c, ptr)
    arr = lambda v: (P * len(v))(*v)
    change = {"count0": dict(count=0), "null-psi": dict(psi=arr([0] + psi[1:])), "null-omega": dict(om=arr([om[0], 0])),
              "direction2": dict(direction=2), "d1": dict(d=1), "d65": dict(d=65), "zero-rank": dict(lr=(0,)), "null-work": dict(work=None)}[what]
    with pytest.raises(ValueError):
        run(nat, what, entry_args(c, ptr, **change))
    ref.check_untouched({n: d.get() for n, d in dO.items()}, what)
    dev.operands_untouched(what)
    # the same buffers in a good call: they were what a call writes
    run(nat, what, entry_args(c, ptr))
    assert not np.all(dO["c0"].get().view(np.uint64) == ref.SENT) and not np.all(dO["work0"].get().view(np.uint64) == ref.SENT)
