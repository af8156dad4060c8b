"""The three fused chain-step kernels -- chain_step_kernel (ttsk_chain_step), chain_wide_kernel (ttsk_chain_step_wide),
chain_sum_kernel (ttsk_chain_step_sum) -- at every edge of their host plans, element by element.

The cases, their operands, the reference and the checks are those of tests/chain_step_ref.py (read its docstring);
tests/test_chain_edge_cover.py shows without a GPU that each case reaches the plan branch it is tagged with, that the
tags cover every branch, and that the checks reject a result with one wrong piece.  Here every accepted case runs through
the C entry point, in both layouts of X and with every way of storing T:

- integer pass: Out and T EQUAL the int64 einsum; Gaussian pass: every element within the derived bound of the
  long-double truth, then the Frobenius ratio;
- every guard element around Out and T (and the padding inside a stacked-terms T) still holds the sentinel, W, X and E
  read back bit-identical, a second call on fresh sentinel buffers gives the same bits;
- the profiling bracket (class 11: a direct call) names the instantiation the case's tags say -- on a device with 256
  compute units, which the tags assume; on another the numerics run and the name check is left out with a note;
- cases marked `pack` repeat the Gaussian call after ttsk_drm_pack: the same bits as from the unpacked core.

The far side of every cover limit must raise TtskUnsupported and write nothing."""
import ctypes

import pytest

from tests import chain_step_ref as ref
from tests.edge_kit import PROF_OTHER, assert_bits_equal, nat, num_cu, run_entry, same_bits  # noqa: F401
from tests.test_chain_plan import bracket_name

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
CASES = ref.all_cases()
REFUSED = ref.refusals()


def expected_name(c, wt):
    f = dict(x.split("=") for x in ref.TAGS[c.id].split())
    f["wt"] = "1" if wt else "0"
    return bracket_name(c.kind, f, {"cw": [str(x) for x in ref.CW]})


class Device:
    """the operands of one (case, pass, layout) on the device; call() runs the entry point on fresh sentinel buffers"""

    def __init__(self, nat, c, layout, vals):
        from tt_sketch_amd.device import DevArray
        self.nat, self.c, self.layout = nat, c, layout
        self.hW, self.hX, self.hE, self.off = ref.operands(c, layout, vals)
        self.dW, self.dX = [DevArray.from_host(w) for w in self.hW], [DevArray.from_host(x) for x in self.hX]
        self.dE = DevArray.from_host(self.hE)
        assert all(d.ptr % 16 == 0 for d in self.dW + self.dX + [self.dE])
        self.e_ptr = self.dE.ptr + 8 * self.off["E"]

    def call(self, wt, profile=False):
        """-> (host images of the Out buffers, of the T buffers or None, recorded kernel name or None)"""
        from tt_sketch_amd.device import DevArray
        c, nat = self.c, self.nat
        g = ref.geometry(c, self.layout, wt)
        hO, hT = ref.sentinels(c, self.layout, wt)
        dO = [DevArray.from_host(o) for o in hO]
        dT = [DevArray.from_host(t) for t in hT] if hT is not None else None
        arr = lambda ds, offs: (P * c.nb)(*[d.ptr + 8 * o for d, o in zip(ds, offs)])
        args = [c.nb, c.n, c.K1, c.A, c.A2, c.J, arr(self.dW, self.off["W"]), g["w_c"], arr(self.dX, self.off["X"]), g["x_j"], g["x_k"],
                g["x_c"], g["x_extent"], P(self.e_ptr)]
        if c.kind == "sum":
            args += [P(dT[0].ptr + 8 * ref.PRE) if dT else None, g["t_b"], g["t_ld"], g["t_extent"]]
        else:
            args += [arr(dT, [ref.PRE] * c.nb) if dT else None]
        args += [arr(dO, [ref.PRE] * c.nb), 0]
        name = None
        try:
            name = run_entry(nat, ref.KINDS[c.kind], args, c.id, PROF_OTHER if profile else None)
        finally:
            self.out = [d.get() for d in dO]
            self.T = [d.get() for d in dT] if dT else None
        return self.out, self.T, name

    def pack(self):
        self.nat.call("ttsk_drm_pack", P(self.e_ptr), self.c.A, self.c.n, self.c.A2, 0)

    def unpack(self):
        self.nat.call("ttsk_drm_unpack", P(self.e_ptr))

    def operands_untouched(self, what):
        for name, host, dev in (("W", self.hW, self.dW), ("X", self.hX, self.dX), ("E", [self.hE], [self.dE])):
            for b, (h, d) in enumerate(zip(host, dev)):
                assert_bits_equal(d, h, "%s: %s[%d]" % (what, name, b))


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_chain_step_edge_case(nat, num_cu, c):
    seed = sum(map(ord, c.id))
    worst = {"Out": 0.0, "T": 0.0}
    for integer in (True, False):
        vals = ref.values(c, integer, seed + (0 if integer else 1))
        tr = ref.truth(c, vals, integer)
        for layout in ref.layouts(c):
            dev = Device(nat, c, layout, vals)
            for wt in ref.T_MODES[c.kind]:
                what = "%s %s T%d %s" % (c.id, layout, wt, "integer" if integer else "Gaussian")
                out, T, name = dev.call(wt, profile=True)
                w = ref.check_results(c, layout, wt, out, T, tr, integer)
                worst = {k: max(worst[k], w[k]) for k in worst}
                if num_cu == 256:
                    assert name == expected_name(c, wt), "%s: ran %r, the tags say %r" % (what, name, expected_name(c, wt))
                same_bits(dev.call(wt)[:2], (out, T), what + ", second call")
                if c.opts.get("pack") and not integer:
                    dev.pack()
                    try:
                        packed = dev.call(wt)[:2]
                    finally:
                        dev.unpack()
                    same_bits(packed, (out, T), what + ", packed core")
            dev.operands_untouched("%s %s" % (c.id, layout))
    print("[chain edges] %s: largest |err| / bound, Gaussian pass: Out %.3g, T %.3g" % (c.id, worst["Out"], worst["T"]))


@pytest.mark.parametrize("c", REFUSED, ids=[c.id for c in REFUSED])
def test_outside_the_cover_is_refused_and_nothing_written(nat, c):
    vals = ref.values(c, False, 5)
    for layout in ref.layouts(c):
        dev = Device(nat, c, layout, vals)
        for wt in ref.T_MODES[c.kind]:
            with pytest.raises(nat.TtskUnsupported):
                dev.call(wt)
            ref.check_untouched(c, dev.out, dev.T, "%s %s T%d" % (c.id, layout, wt))
        dev.operands_untouched("%s %s" % (c.id, layout))
