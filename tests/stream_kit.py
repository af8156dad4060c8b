"""A one-call driver queued on a library stream s with no host synchronisation around it: what the tests of
tests/test_gpu_streams_in_flight.py share.  Plain module (no fixtures of its own): the device is touched only inside the
functions, through tt_sketch_amd._native handed in as `nat`.

The drivers fork helper streams behind the caller's stream and join them back.  With the host synchronised around a call
neither shows: the helper finds the operands complete whether it was forked or not, and the host reads the results after
every stream has drained.  Here everything is queued on s and the host waits once, at the end, for s alone:

  blocker    k plain ttsk_gemm calls of one square shape on s, queued first.  While they run the host queues everything
             below, so that the call under test stands complete in the queues before its first kernel may start.
             k = ceil(GATE_FACTOR * t_enqueue / t_unit): t_unit, one product, is timed on the device (ttsk_timer_start /
             _stop) in a run of its own; t_enqueue, the host time of queuing what is under test, is taken with perf_counter
             in a synchronous warm-up run of the same calls (which also grows every scratch arena: a growing arena
             synchronises its stream).  GATE_FACTOR = 4 covers a busy host.  The blocker stays under GATE_CAP_MS.  After the
             gated run the time actually taken to queue (the blocker's own calls included) must be below k * t_unit;
             otherwise the step is repeated ONCE with 2 k -- a timing condition, never a repeat after an error -- and then
             fails with both times.  Two calls in flight: one blocker on the first caller's stream and
             ttsk_stream_wait(second, first) behind it.
  producer   the cores (or Psi / Omega) the call reads lie in a buffer prefilled with NaN; behind the blocker a ttsk_d2d on
             s copies the data into place.  A kernel on a helper stream that was not forked behind s starts while the
             blocker runs, reads NaN, and the exact comparison fails.  What this cannot show: the library's 8 streams share
             the hardware queues the runtime opens (4 by default), and a helper that shares a queue with s stands behind the
             blocker whether it was forked or not.  How the runtime maps streams to queues is not stated anywhere; that s
             and s + 1 do not share one is an assumption that only one observation supports (with the fork of run_chains
             removed, the helper of stream 0 did read NaN).  If the mapping is stream mod 4, a missing fork of the pair on
             s + 4 in the concurrent chains of ttsk_tt_orth_sketch_batch is NOT detectable by the producer; the consumer,
             the oracle and the bits of a synchronous call still hold that pair's results.
  consumer   the outputs lie in sentinel buffers (edge_kit); behind the call a ttsk_d2d on s copies the WHOLE buffer, guards
             included, into a second sentinel buffer, then ttsk_sync(s) only, and the copy is what is checked: what a helper
             that was not joined had not written yet is still the sentinel (or the prefill) in the copy.

Every GPU step runs inside gpu_step (sketch_int_ref: a limit of 60 s, a HIP error ends the run); nothing is repeated after an
error.

last_sketch_stream (tt_fused.hip) is process-wide: the stream of the one-call sketch queued last decides whether the next one
counts as pipelined, and so its grids.  A module that called on other streams than 0 ends with restore_sketch_history: one tiny
synchronous sketch on stream 0, so that the first stream-0 call of the next module is planned as it would be alone."""
import ctypes
import math
import time

import numpy as np
import pytest

from tests.edge_kit import PAD, assert_bits_equal, assert_guards, sentinel_buffer
from tests.sketch_int_ref import gpu_step

GATE_N = 1536               # the blocker's unit: one GATE_N^3 product
GATE_FACTOR = 4
GATE_CAP_MS = 250.0
PRE = 6                     # guard elements in front of the first output
POST = 5                    # ... and behind every output (out_stride = plan.size + 5, as in tests/test_gpu_sketch_split.py)
ALIGN = 32                  # elements: every staged operand starts on 256 bytes, as an allocation of its own would


def h2d(nat, dev, host, stream):
    assert host.flags.c_contiguous and host.nbytes <= dev.size * 8
    nat.call("ttsk_h2d", dev, host.ctypes.data, host.nbytes, stream)


class Blocker:
    """k products of one square shape on a stream; one product timed once per stream"""

    def __init__(self, nat):
        from tt_sketch_amd.device import DevArray
        self.nat = nat
        n = GATE_N
        self.A, self.B, self.C = (DevArray.zeros((n * n,)) for _ in range(3))
        self.desc = nat.GemmDesc(batch=1, M=n, N=n, Ko=1, Ki=n, a_m=n, a_ki=1, b_ki=n, b_n=1, c_m=n, c_n=1, alpha=1.0, accumulate=0, split_k=0)
        self._unit = {}

    def queue(self, stream, k):
        for _ in range(k):
            self.nat.call("ttsk_gemm", ctypes.byref(self.desc), self.A, self.B, self.C, None, stream)

    def unit_ms(self, stream):
        if stream not in self._unit:
            nat, ms = self.nat, ctypes.c_float()
            with gpu_step(nat, "blocker unit on stream %d" % stream):
                self.queue(stream, 1)                      # (its split-K slabs, the kernel's first launch)
                nat.call("ttsk_sync", stream)
                nat.call("ttsk_timer_start", stream)
                self.queue(stream, 4)
                nat.call("ttsk_timer_stop", stream, ctypes.byref(ms))
            assert ms.value > 0
            self._unit[stream] = ms.value / 4
        return self._unit[stream]


class Staged:
    """Host arrays as the operands of a call, behind one another in ONE device buffer `work` that is NaN until produce()
    copies them in from `stage`.  The gaps between them hold edge_kit's PAD: finite, and a read that meets a nonzero partner
    shows."""

    def __init__(self, nat, arrays, stream):
        from tt_sketch_amd.device import DevArray
        self.nat = nat
        self.off, tot = [], 0
        for a in arrays:
            self.off.append(tot)
            tot += (a.size + ALIGN - 1) // ALIGN * ALIGN
        self.image = np.full(tot, PAD)
        for a, o in zip(arrays, self.off):
            self.image[o:o + a.size] = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
        self.nan_image = np.full(tot, np.nan)
        self.stage, self.nan, self.work = (DevArray.empty((tot,)) for _ in range(3))
        h2d(nat, self.stage, self.image, stream)
        h2d(nat, self.nan, self.nan_image, stream)
        self.ptrs = (ctypes.c_void_p * len(arrays))(*[self.work.ptr + 8 * o for o in self.off])

    def poison(self, stream):
        self.nat.call("ttsk_d2d", self.work, self.nan, self.image.nbytes, stream)

    def produce(self, stream):
        self.nat.call("ttsk_d2d", self.work, self.stage, self.image.nbytes, stream)

    def assert_kept(self, what):
        assert_bits_equal(self.work, self.image, "%s: an operand" % what)


class Outs:
    """Outputs of `sizes` elements behind one another in a sentinel buffer on the device -- PRE guard elements in front, POST
    behind each (equal sizes: `stride` = size + POST apart; even: one more where the next would start on an odd element) --
    and `rounds` sentinel buffers that take its copies.  prefill: what the outputs hold before the call (accumulate), else
    they are sentinels too."""

    def __init__(self, nat, sizes, rounds, stream, prefill=None, even=False):
        from tt_sketch_amd.device import DevArray
        self.nat, self.sizes, self.off, tot = nat, list(sizes), [], PRE
        for n in self.sizes:
            self.off.append(tot)
            tot += n + POST
            tot += (tot & 1) if even else 0
        self.stride = self.sizes[0] + POST
        self.image = sentinel_buffer(tot - PRE, PRE, 0)
        self.prefill = prefill
        if prefill is not None:
            for o, n, p in zip(self.off, self.sizes, prefill):
                self.image[o:o + n] = p
        self.blank = sentinel_buffer(self.image.size, 0, 0)
        self.buf = DevArray.empty((self.image.size,), stream=stream)
        self.copies = [DevArray.empty((self.image.size,), stream=stream) for _ in range(rounds)]
        self.out = self.buf[PRE:]                                   # what an entry with one output pointer gets
        self.views = [(o, (n,), (1,)) for o, n in zip(self.off, self.sizes)]

    def ptr(self, i):
        return self.buf.ptr + 8 * self.off[i]

    def reset(self, stream):
        h2d(self.nat, self.buf, self.image, stream)
        for c in self.copies:
            h2d(self.nat, c, self.blank, stream)

    def copy(self, rnd, stream):
        self.nat.call("ttsk_d2d", self.copies[rnd], self.buf, self.image.nbytes, stream)

    def fetch(self, rnd, stream, what):
        """-> the outputs of round rnd from its copy (guards checked), each a flat host array"""
        got = self.copies[rnd].get(stream)
        assert_guards(got, self.views, what)
        return [got[o:o + n].copy() for o, n in zip(self.off, self.sizes)]


def pieces(flat, like):
    """the flat packed output cut into arrays of the shapes of `like`"""
    out, o = [], 0
    for w in like:
        out.append(flat[o:o + w.size].reshape(w.shape))
        o += w.size
    assert o == flat.size
    return out


def run_gated(nat, blocker, streams, prepare, enqueue, fetch, what):
    """streams: the caller streams, the blocker on the first.  prepare(): puts every buffer into its state before the call
    (blocking copies).  enqueue(): queues producers, the calls under test and the consumers, nothing that waits.  fetch():
    reads the consumers' copies after ttsk_sync of the caller streams alone.  -> fetch()'s result of the gated run."""
    first = streams[0]
    t_unit = blocker.unit_ms(first)
    with gpu_step(nat, what + " (warm-up)"):
        prepare()
        nat.call("ttsk_sync", -1)
        t0 = time.perf_counter()
        enqueue()
        t_enq = (time.perf_counter() - t0) * 1e3
    cap = max(1, int(GATE_CAP_MS / t_unit))
    k = min(cap, max(1, math.ceil(GATE_FACTOR * t_enq / t_unit)))
    for attempt in (0, 1):
        with gpu_step(nat, what):
            prepare()
            nat.call("ttsk_sync", -1)
            t0 = time.perf_counter()
            blocker.queue(first, k)
            for s in streams[1:]:
                nat.call("ttsk_stream_wait", s, first)
            enqueue()
            seen = (time.perf_counter() - t0) * 1e3
            for s in streams:
                nat.call("ttsk_sync", s)
            got = fetch()
        print("gate %s: stream %d, t_unit %.3f ms, t_enqueue %.3f ms, k %d, blocker %.3f ms, queued in %.3f ms"
              % (what, first, t_unit, t_enq, k, k * t_unit, seen))
        if seen < k * t_unit:
            return got
        if attempt == 0:
            k = min(cap, 2 * k)
    pytest.fail("%s: queuing took %.3f ms, the blocker (%d products of %.3f ms) only %.3f ms: the call was not gated"
                % (what, seen, k, t_unit, k * t_unit))


def restore_sketch_history(nat, plan, X):
    """One tiny synchronous one-call sketch on stream 0 (plan, X: any plan and the core pointers of one tensor of it):
    last_sketch_stream is 0 again, as every module that calls on stream 0 only leaves it."""
    from tt_sketch_amd.device import DevArray
    out = DevArray.empty((plan.size,))
    with gpu_step(nat, "restoring the sketch history"):
        plan.run(X, out, stream=0)
