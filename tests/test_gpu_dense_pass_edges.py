"""The two passes over a dense tensor -- dense_pass_kernel (ttsk_dense_first_pass) and dense_left_pass_kernel
(ttsk_dense_left_pass) -- at every edge of their host plans, element by element.

The cases, their operands, the reference and the checks are those of tests/dense_pass_ref.py (read its docstring);
tests/test_dense_pass_cover.py shows without a GPU that each case reaches the plan branch it is tagged with, that the tags
cover every branch, that the checks reject a result with one wrong piece, and that no case needs more scratch than its
poison shape.  Here every accepted case runs through the C entry point:

- poison: the same entry point first runs a fixed larger shape whose X is scaled by 2^500 -- the library's scratch then
  holds huge values wherever the case may read a slab slice, a partial Z or a left slab that it did not write itself;
- integer pass: Z and U (Z_0, Z_1, Z_2, E3) EQUAL the int64 einsum; Gaussian pass: every element within the derived
  bound of the long-double truth, then the Frobenius ratio;
- every guard element around the outputs still holds the sentinel, the operands read back bit-identical, a second call
  on fresh sentinel buffers gives the same bits.

The far side of every cover limit must raise TtskUnsupported and write nothing."""
import ctypes

import pytest

from tests import dense_pass_ref as ref
from tests.edge_kit import assert_bits_equal, nat, run_entry, same_bits, sentinel_buffer  # noqa: F401

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
CASES = ref.all_cases()
REFUSED = ref.refusals()


def entry_args(c, ptr):
    """the arguments of the C entry point: ptr maps an operand's or output's name to its device address"""
    if c.kind == "first":
        return [P(ptr["X"]), c.n0, c.Q, c.T, P(ptr["C"]), c.ll, P(ptr["P"]), c.r, P(ptr["Z"]), P(ptr["U"]), 0]
    return [P(ptr["X"]), c.n0, c.n1, c.n2, c.n3 * c.n4, c.n4, c.l] + [P(ptr[n]) for n in ("A0", "A1t", "A2t", "A3p", "Z0", "Z1", "Z2", "E3")] + [0]


def run(nat, c, args):
    run_entry(nat, ref.ENTRY[c.kind], args, c.id)


class Device:
    """the operands of one (case, pass) on the device; call() runs the entry point on fresh sentinel buffers"""

    def __init__(self, nat, c, vals):
        from tt_sketch_amd.device import DevArray
        self.nat, self.c = nat, c
        self.host = ref.operands(c, vals)
        self.dev = {n: DevArray.from_host(h) for n, h in self.host.items()}
        assert all(d.ptr % 16 == 0 for d in self.dev.values())
        self.ptr = {n: d.ptr + 8 * (ref.PRE + ref.offset(c, n)) for n, d in self.dev.items()}

    def call(self):
        """-> host images of the output buffers after the call (also kept in self.out when the call raises)"""
        from tt_sketch_amd.device import DevArray
        c = self.c
        dO = {n: DevArray.from_host(h) for n, h in ref.sentinels(c).items()}
        assert all(d.ptr % 16 == 0 for d in dO.values())
        ptr = dict(self.ptr, **{n: d.ptr + 8 * (ref.PRE + ref.offset(c, n)) for n, d in dO.items()})
        try:
            run(self.nat, c, entry_args(c, ptr))
        finally:
            self.out = {n: d.get() for n, d in dO.items()}
        return self.out

    def operands_untouched(self, what):
        for n, h in self.host.items():
            assert_bits_equal(self.dev[n], h, "%s: %s" % (what, n))


@pytest.fixture(scope="module")
def poison(nat):
    """kind -> a call of that entry point on its poison shape; the operands go to the device once"""
    held = {}
    for c in (ref.POISON_FIRST, ref.POISON_LEFT):
        from tt_sketch_amd.device import DevArray
        v = ref.values(c, False, 99, scale=2.0 ** 500)
        ins = {n: DevArray.from_host(h) for n, h in ref.operands(c, v).items()}
        outs = {n: DevArray.from_host(h) for n, h in ref.sentinels(c).items()}
        ptr = {n: d.ptr + 8 * ref.PRE for n, d in list(ins.items()) + list(outs.items())}
        held[c.kind] = (c, ins, outs, entry_args(c, ptr))
    return lambda kind: run(nat, held[kind][0], held[kind][3])


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_dense_pass_edge_case(nat, poison, c):
    seed = sum(map(ord, c.id))
    worst = {}
    for integer in (True, False):
        what = "%s %s" % (c.id, "integer" if integer else "Gaussian")
        vals = ref.values(c, integer, seed + (0 if integer else 1))
        tr = ref.truth(c, vals, integer)
        dev = Device(nat, c, vals)
        poison(c.kind)
        out = dev.call()
        worst = ref.check_results(c, out, tr, integer)
        again = dev.call()
        same_bits(again, out, what + ", second call")
        dev.operands_untouched(what)
    print("[dense pass edges] %s: largest |err| / bound, Gaussian pass: %s" % (c.id, ", ".join("%s %.3g" % kv for kv in worst.items())))


@pytest.mark.parametrize("c", REFUSED, ids=[c.id for c in REFUSED])
def test_outside_the_cover_is_refused_and_nothing_written(nat, c):
    from tt_sketch_amd.device import DevArray
    if c.opts.get("dummy"):              # refused before anything is touched: no operand of that size for this
        host = sentinel_buffer(64, ref.PRE, ref.POST)
        d = DevArray.from_host(host)
        ptr = {n: d.ptr + 8 * ref.PRE for n in ref.IN_NAMES[c.kind] + ref.OUT_NAMES[c.kind]}
        with pytest.raises(nat.TtskUnsupported):
            run(nat, c, entry_args(c, ptr))
        ref.check_untouched({"the one buffer": d.get()}, c.id)
        return
    dev = Device(nat, c, ref.values(c, False, 5))
    with pytest.raises(nat.TtskUnsupported):
        dev.call()
    ref.check_untouched(dev.out, c.id)
    dev.operands_untouched(c.id)
