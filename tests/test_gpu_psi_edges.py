"""The two Psi product kernels of csrc/stream_small.h -- stream_small_kernel (ttsk_psi_stream) and stream_small_sum_kernel
(ttsk_psi_stream_sum) -- at every edge of their host plans (csrc/psi_plan.h), element by element.

The cases, their operands, the reference and the checks are those of tests/psi_stream_ref.py (read its docstring);
tests/test_psi_plan.py shows without a GPU that each case reaches the plan branch it is tagged with, that the tags cover
both launch tables completely, and that the checks reject a result with one wrong piece.  Here every accepted case runs
through its C entry point:

- integer pass: C (with `accumulate` the prior C plus the product) EQUALS the int64 einsum; Gaussian pass: every element
  within the derived bound of the long-double truth, then the Frobenius ratio;
- every element of the C buffers outside the J x A window (row padding, the guard bands) still holds the sentinel, S and W
  read back bit-identical, a second call on fresh buffers gives the same bits.  W's padding is NaN and S's 1e300, so a
  result that uses either as data cannot pass;
- the profiling bracket (class 11: a direct call) names the instantiation the case's tags say -- on a device with 256
  compute units, which the tags assume; on another the numerics run and the name check is left out with a note;
- the nan_gap cases put NaN into the doubles between two terms of the sum kernel's S, and only there: row J - 1 of C is
  NaN throughout and every other row is right -- the behaviour csrc/stream_small.h documents and the driver excludes.

The far side of every cover limit must raise TtskUnsupported and write nothing.  The end-to-end test at the bottom runs
the driver (tsa.stream_sketch of a TensorSum) on the two routes that hand these kernels their arguments: the sum kernel
with an odd lt n s -- a pad double between the terms' T, poisoned by a call before it -- and the chunked interleaved route."""
import ctypes

import numpy as np
import pytest

from tests import psi_stream_ref as ref
from tests.edge_kit import PROF_OTHER, assert_bits_equal, nat, num_cu, rel_fro, run_entry, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
CASES = ref.all_cases()
REFUSED = ref.refusals()


class Device:
    """the operands of one (case, pass) on the device; call() runs the entry point on fresh sentinel buffers"""

    def __init__(self, nat, c, vals, cb=None):
        """cb: the case the buffers are made for, where the call's own nb makes none (a refused nb of 0 or 33: the pointer tables
        then repeat cb's buffers)"""
        from tt_sketch_amd.device import DevArray
        self.nat, self.c, self.vals, self.cb = nat, c, vals, cb or c
        self.hS, self.hW = ref.operands(self.cb, vals)
        self.dS, self.dW = [DevArray.from_host(s) for s in self.hS], [DevArray.from_host(w) for w in self.hW]
        assert all(d.ptr % 16 == 0 for d in self.dS + self.dW)

    def call(self, profile=False):
        """-> (host images of the C buffers, recorded kernel name or None)"""
        from tt_sketch_amd.device import DevArray
        c, nat, g = self.c, self.nat, ref.geometry(self.c)
        dC = [DevArray.from_host(x) for x in ref.sentinels(self.cb, self.vals)]
        acc = int(bool(c.opts.get("acc")))
        if c.kind == "ss":
            ntab = max(1, min(c.nb, 33))
            arr = lambda ds: (P * ntab)(*[ds[b % len(ds)].ptr + 8 * ref.PRE for b in range(ntab)])
            args = [c.nb, c.J, c.K1, c.A, arr(self.dS), g["s_j"], arr(self.dW), g["w_c"], arr(dC), g["c_j"], acc, 0]
        else:
            args = [c.nb, c.J, c.K1, c.A, P(self.dS[0].ptr + 8 * ref.PRE), g["s_j"], g["s_b"], P(self.dW[0].ptr + 8 * ref.PRE), g["w_c"], g["w_b"],
                    P(dC[0].ptr + 8 * ref.PRE), g["c_j"], acc, 0]
        name = None
        try:
            name = run_entry(nat, ref.KINDS[c.kind], args, c.id, PROF_OTHER if profile else None)
        finally:
            self.out = [d.get() for d in dC]
        return self.out, name

    def operands_untouched(self, what):
        for name, host, dev in (("S", self.hS, self.dS), ("W", self.hW, self.dW)):
            for b, (h, d) in enumerate(zip(host, dev)):
                assert_bits_equal(d, h, "%s: %s[%d]" % (what, name, b))


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_psi_stream_edge_case(nat, num_cu, c):
    seed = sum(map(ord, c.id))
    worst = 0.0
    for integer in (True, False):
        vals = ref.values(c, integer, seed + (0 if integer else 1))
        tr = ref.truth(c, vals, integer)
        dev = Device(nat, c, vals)
        what = "%s %s" % (c.id, "integer" if integer else "Gaussian")
        out, name = dev.call(profile=True)
        worst = max(worst, ref.check_results(c, out, tr, integer))
        if num_cu == 256:
            assert name == ref.expected_name(c), "%s: ran %r, the tags say %r" % (what, name, ref.expected_name(c))
        same_bits(dev.call()[0], out, what + ", second call")
        dev.operands_untouched(what)
    print("[psi edges] %s: largest |err| / bound, Gaussian pass: %.3g" % (c.id, worst))


@pytest.mark.parametrize("c", REFUSED, ids=[c.id for c in REFUSED])
def test_outside_the_cover_is_refused_and_nothing_written(nat, c):
    cb = c._replace(nb=min(max(c.nb, 1), 2)) if c.kind == "ss" else c
    dev = Device(nat, c, ref.values(cb, False, 5), cb)
    with pytest.raises(nat.TtskUnsupported):
        dev.call()
    ref.check_untouched(cb, dev.out, c.id)
    dev.operands_untouched(c.id)


# ------------------------------------------------------------------------------------------------ through the driver
def _sum_sketch(nat, shape, ranks, lr, rr, nb, seed, kernel, poison=None):
    """The sketch of the sum of nb random TTs -- ttsk_tt_sketch_sum through its plan object, then tsa.stream_sketch of the
    TensorSum -- against the sum of the oracle's sketches, at the bar of tests/test_gpu_parity.py; the Psi bracket (class 4)
    must name `kernel`.  poison = a mode: before each of the two, a call of the same ranks with that mode one longer and NaN
    cores runs on the same stream -- its T of that mode, NaN throughout, lies over the pad double that follows term 0 of the
    call under test (the workspace blocks before it depend on the ranks alone, and the scratch slot only ever grows)."""
    import ctypes as ct
    import tt_sketch_amd as tsa
    from oracle import ttsk_oracle as orc
    from tt_sketch_amd import tt_fused
    from tt_sketch_amd.device import DevArray
    from tests.gpu_build import make_drm, make_tensor
    rng = np.random.default_rng(seed)

    def operands(shape, nan):
        ld, rd = orc.random_tt_drm(shape, lr, False, rng), orc.random_tt_drm(shape, rr, True, rng)
        tts = [orc.random_tt(shape, ranks, rng) for _ in range(nb)]
        if nan:
            tts = [[np.full_like(x, np.nan) for x in cores] for cores in tts]
        return ld, rd, tts, make_drm(ld), make_drm(rd), [make_tensor("tt", c) for c in tts]

    def run_plan(L, R, dev):
        plan = tt_fused.TTSketchPlan(dev[0].shape, dev[0].rank, L, R)
        keep, flat = [], []
        for t in dev:
            ptrs, k = plan.core_pointers(t)
            keep.append(k)
            flat += [ptrs[i] for i in range(plan.d)]
        out = DevArray.empty((plan.size,))
        plan.run_sum((ct.c_void_p * len(flat))(*flat), nb, out)
        Psi, Om = plan.views(out)
        return [a.get() for a in Psi + Om]

    def run_api(L, R, dev):
        sk = tsa.stream_sketch(tsa.TensorSum(dev), L.rank, tuple(R.rank[::-1]), left_drm=L, right_drm=R)
        return [np.asarray(a) for a in sk.Psi_cores + sk.Omega_mats]

    def poisoned():
        if poison is None:
            return
        big = tuple(n + 1 if i == poison else n for i, n in enumerate(shape))
        got = run_plan(*operands(big, True)[3:])
        assert np.isnan(got[poison]).all()                    # the poison went through the workspace

    ld, rd, tts, L, R, dev = operands(shape, False)
    want = None
    for cores in tts:
        oP, oO = orc.general_sketch("tt", cores, ld, rd, "streaming")
        want = [a + b for a, b in zip(want, oP + oO)] if want else list(oP + oO)
    for run in (run_plan, run_api):
        poisoned()
        nat.call("ttsk_sync", -1)
        nat.call("ttsk_prof_enable", 1)
        try:
            got = run(L, R, dev)
            nat.call("ttsk_sync", -1)
            buf = ctypes.create_string_buffer(160)
            nat.call("ttsk_prof_kernel_name", 4, buf, ctypes.c_size_t(len(buf)))
        finally:
            nat.call("ttsk_prof_enable", 0)
        assert buf.value.decode().startswith(kernel + "<"), (shape, run.__name__, buf.value.decode())
        for i, (a, w) in enumerate(zip(got, want)):
            assert a.shape == w.shape and np.isfinite(a).all(), (shape, run.__name__, i, "a non-finite element")
            assert rel_fro(a, w) < 1e-12, (shape, run.__name__, i, rel_fro(a, w))


def test_driver_hands_the_kernels_the_same_arguments(nat):
    """(a) The smallest signature on the sum kernel's route (c.sum, T per term, s > 48, l n >= 1024) with an odd lt n s: lt =
    25, n = 41, s = 49, three terms, right rank 17 -- the narrowest the kernel takes; the next left rank 19 is odd, so the chain
    matrices are not packed and T stays per term.  The terms' T lie even(50225) = 50226 doubles apart; the double behind term
    0 is inside the kernel's descriptor, K1 = 49 never fills its k-blocks, and the call before it has left NaN there.  The
    driver zeroes it: the sketch is finite and equals the oracle's.
    (b) The chunked interleaved route (tail_sum: stream_small_chunks cuts K = 16 terms x rank 20 = 320 in two, the chunks of
    both interior modes are the four problems of one launch of stream_small_kernel, row stride 320): l n = 50 x 21 = 1050."""
    _sum_sketch(nat, (12, 41, 10), (12, 49), (25, 19), (17, 17), 3, 41, "stream_small_sum_kernel", poison=1)
    _sum_sketch(nat, (16, 21, 21, 16), (20, 20, 20), (50, 50, 50), (100, 100, 100), 16, 43, "stream_small_kernel")
