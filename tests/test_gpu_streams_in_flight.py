"""The one-call drivers on every library stream and with calls in flight: what forks helper streams, shares per-stream state
and is what bench.py times, queued as a pipelining caller queues it -- on a stream s that is busy, with no host
synchronisation around the call (tests/stream_kit.py: blocker, NaN producer, copying consumer).

(a) ttsk_tt_sketch / _batch / _sum on every caller stream 0 .. 7 (7: the helper wraps to 0), one call at a time;
(b) two calls in flight on the stream pairs of the benchmark (0, 2) and on adjacent callers (0, 1), (7, 0), where the first
    call's helper stream is the second call's own, three rounds back to back into the same output slots;
(c) the one branch of the CU-budget policy that splits (csrc/sketch_split.h: a pipelined caller, 8 tensors or more), reached
    by alternating calls on streams 0 and 2, and that last_sketch_stream is all the history a call depends on;
(d) ttsk_tt_orth_sketch, ttsk_tt_orth_sketch_batch (one chain of launches; concurrent chains of 3 and of 9 tensors, more than
    there are stream pairs; one with a rank-deficient tensor), ttsk_tt_assemble at d = 12 (more pairs than streams, batched
    and pair by pair) and ttsk_tt_assemble_batch, gated on streams 0, 5 and 7.

Integer cores (tests/sketch_int_ref.py), (a) - (c): every Psi and Omega EQUALS the int64 einsum, whatever stream, order and grid.
Gaussian cores, (c): the oracle at the 1e-12 of tests/test_gpu_parity.py, and bits against a synchronous call.  (d): the oracle
(numpy's pinv for the assemblies) at the entrywise bar of tests/test_gpu_orth_one_call.py, the bits of a synchronous call on
stream 0 where two such calls agree in theirs, and the verdict words: dev_status, and ttsk_deferred_status of every stream."""
import ctypes

import numpy as np
import pytest

from oracle import ttsk_oracle as orc
from tests import stream_kit as sk
from tests.edge_kit import exact, nat, num_cu, same_bits, tsa  # noqa: F401
from tests.golden_io import rel
from tests.sketch_int_ref import Case, gpu_step, split_of
from tests.test_gpu_orth_one_call import _case, _close, _dev_drms
from tests.test_sketch_int_ref_host import policy_budgets

pytestmark = pytest.mark.gpu

TOL = 1e-12                 # tests/test_gpu_parity.py: test_batched_one_call_path, test_sketch_of_a_sum_in_one_call
STREAMS = tuple(range(8))
PAIRS = ((0, 2), (0, 1), (7, 0))
ROUNDS = 3

_cases, _orth, _assemble_refs = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def module_end(nat):  # noqa: F811
    """Whatever part of the module ran: the sketch history is put back and the caches (device arrays, references) are dropped."""
    yield
    # Calls went to other streams than 0 (the chains of the orthogonalising sketches count: tt_chains runs through
    # run_chains too): the next module's first stream-0 sketch would count as pipelined (tt_fused.hip, last_sketch_stream)
    # and a batch of 8 or more would get other grids, and so other bits, than it gets alone.
    plan, X, _ = (_cases.get("b2") or Case("b2")).on_device("gauss")
    sk.restore_sketch_history(nat, plan, X)
    _cases.clear()
    _orth.clear()
    _assemble_refs.clear()


@pytest.fixture(scope="module")
def cases():
    def get(name):
        if name not in _cases:
            _cases[name] = Case(name)
        return _cases[name]
    return get


@pytest.fixture(scope="module")
def blocker(nat):  # noqa: F811
    return sk.Blocker(nat)


class Call:
    """One entry (batch / sum / run) of one case and kind on one caller stream: its staged cores, its outputs, its reference."""

    def __init__(self, nat, case, kind, entry, stream, rounds, accumulate=False):  # noqa: F811
        self.nat, self.entry, self.stream, self.rounds, self.accumulate = nat, entry, stream, rounds, accumulate
        self.plan = case.on_device(kind)[0]
        _, _, tts, want, want_sum = case.data[kind]
        self.nb = 1 if entry == "run" else case.nb
        self.cores = sk.Staged(nat, [c for t in tts[:self.nb] for c in t], stream)
        self.want = [want_sum] if entry == "sum" else want[:self.nb]
        count = 1 if entry == "sum" else self.nb
        prefill = None
        if accumulate:
            rng = np.random.default_rng(stream + 17)
            prefill = [rng.integers(-3, 4, size=self.plan.size).astype(np.float64) for _ in range(count)]
        assert sum(w.size for w in self.want[0]) == self.plan.size
        self.outs = sk.Outs(nat, [self.plan.size] * count, rounds, stream, prefill)
        self.what = "%s %s %s on stream %d%s" % (case.name, kind, entry, stream, ", accumulating" if accumulate else "")

    def prepare(self):
        self.cores.poison(self.stream)
        self.outs.reset(self.stream)

    def produce(self):
        self.cores.produce(self.stream)

    def queue(self, rnd):
        p, X, out, acc, s = self.plan, self.cores.ptrs, self.outs.out, self.accumulate, self.stream
        if self.entry == "batch":
            p.run_batch(X, self.nb, out, self.outs.stride, accumulate=acc, stream=s)
        elif self.entry == "sum":
            p.run_sum(X, self.nb, out, accumulate=acc, stream=s)
        else:
            p.run(X, out, accumulate=acc, stream=s)
        self.outs.copy(rnd, s)

    def fetch(self):
        """-> per round, per output: the pieces Psi + Omega"""
        res = []
        for rnd in range(self.rounds):
            flats = self.outs.fetch(rnd, self.stream, "%s round %d" % (self.what, rnd))
            res.append([sk.pieces(f, w) for f, w in zip(flats, self.want)])
        self.cores.assert_kept(self.what)
        return res

    def expected(self, rnd):
        """round rnd's outputs: the reference, on top of the prefill once per round so far when accumulating"""
        if not self.accumulate:
            return self.want
        return [[p + (rnd + 1) * w for p, w in zip(sk.pieces(pre, ws), ws)] for pre, ws in zip(self.outs.prefill, self.want)]

    def check_exact(self, res):
        for rnd, outs in enumerate(res):
            for b, (got, want) in enumerate(zip(outs, self.expected(rnd))):
                for i, (a, c) in enumerate(zip(got, want)):
                    exact(a, c, "%s round %d output %d piece %d" % (self.what, rnd, b, i))


def in_flight(nat, blocker, calls, what):  # noqa: F811
    """the calls (one per caller stream, the blocker on the first one's) for their rounds, no host synchronisation in between"""
    def prepare():
        for c in calls:
            c.prepare()

    def enqueue():
        for c in calls:
            c.produce()
        for rnd in range(calls[0].rounds):
            for c in calls:
                c.queue(rnd)

    return sk.run_gated(nat, blocker, [c.stream for c in calls], prepare, enqueue, lambda: [c.fetch() for c in calls], what)


# ------------------------------------------------------------------------------------------------ (a)
@pytest.mark.parametrize("shape", ["a3", "b2"])
@pytest.mark.parametrize("s", STREAMS)
def test_every_caller_stream_gated_equals_the_int64_einsum(tsa, nat, blocker, cases, s, shape):  # noqa: F811
    case = cases(shape)
    for entry in ("batch", "sum", "run"):
        for accumulate in (False, True):
            call = Call(nat, case, "int", entry, s, 1, accumulate)
            (res,) = in_flight(nat, blocker, [call], call.what)
            call.check_exact(res)


# ------------------------------------------------------------------------------------------------ (b)
@pytest.mark.parametrize("split", ["auto", "full"])
@pytest.mark.parametrize("order", ["a5 batch, b2 sum", "b2 batch, a5 sum"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: "%d-%d" % p)
def test_two_calls_in_flight_for_three_rounds_equal_the_int64_einsum(tsa, nat, num_cu, blocker, cases, pair, order, split):  # noqa: F811
    (n0, e0), (n1, e1) = (x.split() for x in order.split(", "))
    calls = [Call(nat, cases(n0), "int", e0, pair[0], ROUNDS), Call(nat, cases(n1), "int", e1, pair[1], ROUNDS)]
    nat.call("ttsk_tt_sketch_split", *split_of(split, num_cu, 1))       # ("auto" and "full" do not depend on the batch size)
    try:
        res = in_flight(nat, blocker, calls, "streams %d and %d, %s, %s" % (pair[0], pair[1], order, split))
    finally:
        nat.call("ttsk_tt_sketch_split", -1, -1, -1)
    for c, r in zip(calls, res):
        c.check_exact(r)


# ------------------------------------------------------------------------------------------------ (c)
def alternating_b8(nat, blocker, cases, kind):  # noqa: F811
    """b8 as run_batch on streams 0 and 2 in turns under the policy, ROUNDS rounds in flight: every call of the gated run follows
    one on the other stream (the warm-up ends on stream 2), so each is a pipelined one.  -> the calls, their results"""
    case = cases("b8")
    calls = [Call(nat, case, kind, "batch", 0, ROUNDS), Call(nat, case, kind, "batch", 2, ROUNDS)]
    nat.call("ttsk_tt_sketch_split", -1, -1, -1)
    return calls, in_flight(nat, blocker, calls, "b8 %s alternating on streams 0 and 2" % kind)


def synchronous_b8(nat, cases, split, lead_in):  # noqa: F811
    """the Gaussian b8 batch on stream 0, host synchronised, after `lead_in` calls of the same kind -> per tensor the pieces"""
    from tt_sketch_amd.device import DevArray
    case = cases("b8")
    plan, X, _ = case.on_device("gauss")
    stride = plan.size + sk.POST
    out = DevArray.zeros((case.nb * stride,))
    nat.call("ttsk_tt_sketch_split", *split)
    try:
        for i in range(lead_in + 1):
            with gpu_step(nat, "b8 synchronous under %s, call %d" % (split, i)):
                plan.run_batch(X, case.nb, out, stride)
    finally:
        nat.call("ttsk_tt_sketch_split", -1, -1, -1)
    host = out.get()
    return [sk.pieces(host[b * stride:b * stride + plan.size], case.data["gauss"][3][b]) for b in range(case.nb)]


def test_the_policy_split_with_integer_cores_is_exact(tsa, nat, blocker, cases):  # noqa: F811
    calls, res = alternating_b8(nat, blocker, cases, "int")
    for c, r in zip(calls, res):
        c.check_exact(r)


def test_the_policy_split_is_taken_by_alternating_callers_only(tsa, nat, num_cu, blocker, cases, tmp_path_factory):  # noqa: F811
    case = cases("b8")
    budgets = policy_budgets(num_cu, case, tmp_path_factory)
    print("b8 on %d CUs: the policy's budgets %s" % (num_cu, budgets))
    assert budgets != (0, 0, 0)
    calls, res = alternating_b8(nat, blocker, cases, "gauss")
    want = case.data["gauss"][3]
    for c, r in zip(calls, res):
        for rnd, outs in enumerate(r):
            for b, (got, w) in enumerate(zip(outs, want)):
                for i, (a, x) in enumerate(zip(got, w)):
                    e = rel(a, x)
                    assert a.shape == x.shape and e < TOL, (c.what, rnd, b, i, e)
    forced = synchronous_b8(nat, cases, budgets, 0)
    full = synchronous_b8(nat, cases, (0, 0, 0), 0)
    for c, r in zip(calls, res):
        for rnd, outs in enumerate(r):
            same_bits(outs, forced, "%s round %d against the synchronous call under the policy's budgets" % (c.what, rnd))
    # A budget changes how many slab partials a chain matrix is summed from (include/ttsk.h, ttsk_tt_sketch_split), so the
    # two settings differ in their bits somewhere: equality with `forced` above says that the split was taken.
    assert any(not np.array_equal(a.view(np.uint64), b.view(np.uint64)) for x, y in zip(forced, full) for a, b in zip(x, y)), \
        "the policy's budgets and the whole device give the same bits: the comparison above shows nothing"
    # ... and a caller that stays on stream 0 gets the whole device: the third call in a row on stream 0 under "auto"
    alone = synchronous_b8(nat, cases, (-1, -1, -1), 2)
    same_bits(alone, full, "b8 under the policy after two calls on stream 0, against the whole device")


# ------------------------------------------------------------------------------------------------ (d)
OTHER_STREAMS = (0, 5, 7)

# name -> (mode sizes, TT rank, left rank, right rank, tensors or None for the single call, index of a rank-deficient tensor,
# the form of ttsk_tt_orth_sketch_batch the case is there for).  The form is asserted, not assumed: a batch with ONE
# rank-deficient tensor comes back with one verdict for all its tensors from the single chain of launches ("fused") and with
# that tensor's alone from the concurrent chains on stream pairs ("chains") -- include/ttsk.h.  So a change of the fused form's
# cover cannot take the stream-pair code (tt_orth.hip, the loop over pair_of) out of these tests silently.
ORTH_CASES = {
    "one": ((30, 28, 26, 24, 22), 12, 8, 16, None, None, None),
    "fused3": ((30, 28, 26, 24, 22), 12, 8, 16, 3, None, "fused"),
    "chains3": ((12, 20, 20, 12), 10, 8, 10, 3, None, "chains"),      # n_0 < 2 l: outside the fused form's cover
    "chains9": ((12, 20, 20, 12), 10, 8, 10, 9, None, "chains"),      # ... more tensors than there are stream pairs
    "verdict": ((12, 20, 20, 12), 10, 8, 10, 5, 2, "chains"),         # ... one of them of TT rank 5 < l: its factorisations are rejected
}
# name -> (mode sizes, left ranks, right ranks, sketches or None for the single call)
ASSEMBLE_CASES = {
    "d12": ((9, 12, 12, 12, 12, 12, 12, 12, 12, 10, 11, 13), (5,) * 11, (8,) * 11, None),       # batched pseudo-inverses, 11 pairs
    "d12 mixed": ((9, 12, 12, 12, 12, 12, 12, 12, 12, 10, 11, 13), (5, 4, 6, 5, 4, 6, 5, 4, 6, 5, 4), (8, 9, 7, 8, 9, 7, 8, 9, 7, 8, 9), None),
    "batch3": ((14, 15, 16, 17), (6, 6, 6), (9, 9, 9), 3),
}


class DriverCall:
    """What Call above is for the sketches, for an entry with pointer arrays: operands staged behind NaN, every output a piece
    of one sentinel buffer.  A subclass sets stream, what, operands (Staged), outs (Outs) and queues its entry in entry()."""
    rounds = 1

    def prepare(self):
        self.operands.poison(self.stream)
        self.outs.reset(self.stream)

    def produce(self):
        self.operands.produce(self.stream)

    def queue(self, rnd):
        self.entry()
        self.outs.copy(rnd, self.stream)

    def fetch(self):
        flats = self.outs.fetch(0, self.stream, self.what)
        self.operands.assert_kept(self.what)
        return flats

    def out_ptrs(self, lo, hi):
        return (ctypes.c_void_p * (hi - lo))(*[self.outs.ptr(i) for i in range(lo, hi)])

    def plain(self):
        """the call alone, the host synchronised around it -> its outputs"""
        with gpu_step(self.nat, self.what + " (synchronous)"):
            self.prepare()
            self.nat.call("ttsk_sync", -1)
            self.produce()
            self.queue(0)
            self.nat.call("ttsk_sync", -1)
            return self.fetch()


class OrthSetup:
    """tensors, DRMs and the oracle's cores and Omega of one of ORTH_CASES: built once per module"""

    def __init__(self, tsa, name):  # noqa: F811
        from tt_sketch_amd import tt_fused
        shape, s_in, l, r, count, low_at, self.form = ORTH_CASES[name]
        d = len(shape)
        seed = sum(map(ord, name))
        first, ld, rd = _case(shape, s_in, l, r, seed)
        rng = np.random.default_rng(seed + 1)
        self.drms = _dev_drms(tsa, shape, (l,) * (d - 1), (r,) * (d - 1), ld, rd)
        self.name, self.count, self.low_at, self.d = name, count, low_at, d
        self.tts = [first] + [orc.random_tt(shape, s_in, rng) for _ in range((count or 1) - 1)]
        # as in test_orthogonal_sketch_batch_verdict_per_tensor_and_fallbacks: the signature kept, rank 5 < l
        low = orc.random_tt(shape, 5, rng)
        low = [np.concatenate([c, np.zeros((c.shape[0], c.shape[1], s_in - c.shape[2]))], axis=2) if k < d - 1 else c for k, c in enumerate(low)]
        low = [np.concatenate([c, np.zeros((s_in - c.shape[0], c.shape[1], c.shape[2]))], axis=0) if k > 0 else c for k, c in enumerate(low)]
        if low_at is not None:
            self.tts[low_at] = low
        # what shows the form: the same batch with its LAST tensor rank deficient (the case's own tensors where it has one)
        self.probe_at = low_at if low_at is not None else (count or 1) - 1
        self.probe_tts = self.tts[:self.probe_at] + [low] + self.tts[self.probe_at + 1:]
        self.want_cores = [orc.general_sketch("tt", c, ld, rd, "orthogonal")[0] for c in self.tts]
        self.want_omega = [orc.general_sketch("tt", c, ld, rd, "streaming")[1] for c in self.tts]
        block = tt_fused._orth_block([tsa.TensorTrain(c) for c in self.tts], self.drms[0], self.drms[1], tsa.SketchMethod.orthogonal)
        assert block is not None
        self.args, outs, self.keep = block
        self.core_shapes = [a.shape for o in outs for a in o[0]]
        self.omega_shapes = [a.shape for o in outs for a in o[1]]
        self.refs = None                         # the outputs of two synchronous calls on stream 0, when they agree in their bits


class OrthCall(DriverCall):
    def __init__(self, nat, setup, stream, probe=False):  # noqa: F811
        self.nat, self.setup, self.stream = nat, setup, stream
        self.what = "orthogonal sketch %s%s on stream %d" % (setup.name, " (form probe)" if probe else "", stream)
        self.operands = sk.Staged(nat, [c for t in (setup.probe_tts if probe else setup.tts) for c in t], stream)
        sizes = [int(np.prod(sh)) for sh in setup.core_shapes + setup.omega_shapes]
        self.n_status = ((setup.count or 1) + 1) // 2                   # count int32 verdicts, in whole 8-byte elements
        self.outs = sk.Outs(nat, sizes + [self.n_status], 1, stream, even=True)
        nc = len(setup.core_shapes)
        self.cores, self.omega = self.out_ptrs(0, nc), self.out_ptrs(nc, len(sizes))

    def entry(self):
        d, n, s, lt, rt, _, DL, DR, _, _ = self.setup.args
        if self.setup.count is None:
            self.nat.call("ttsk_tt_orth_sketch", d, n, s, lt, rt, self.operands.ptrs, DL, DR, self.cores, self.omega, self.stream)
        else:
            self.nat.call("ttsk_tt_orth_sketch_batch", self.setup.count, d, n, s, lt, rt, self.operands.ptrs, DL, DR, self.cores, self.omega,
                          ctypes.c_void_p(self.outs.ptr(len(self.outs.sizes) - 1)), self.stream)

    def verdicts(self, flats):
        """-> dev_status (batch) or None"""
        return None if self.setup.count is None else flats[-1].view(np.int32)[:self.setup.count].tolist()

    def check(self, flats):
        su, d = self.setup, self.setup.d
        nc = len(su.core_shapes)
        cores = [f.reshape(sh) for f, sh in zip(flats[:nc], su.core_shapes)]
        omega = [f.reshape(sh) for f, sh in zip(flats[nc:-1], su.omega_shapes)]
        for b in range(su.count or 1):
            for mu, (a, w) in enumerate(zip(omega[b * (d - 1):(b + 1) * (d - 1)], su.want_omega[b])):
                e = rel(a, w)
                assert a.shape == w.shape and e < TOL, (self.what, "Omega", b, mu, e)
            if b != su.low_at:
                _close(cores[b * d:(b + 1) * d], su.want_cores[b])


def deferred_flags(nat):  # noqa: F811
    """ttsk_deferred_status of every library stream (read and cleared)"""
    flags = []
    for t in STREAMS:
        f = ctypes.c_int(-1)
        nat.call("ttsk_deferred_status", t, ctypes.byref(f))
        flags.append(f.value)
    return flags


@pytest.mark.parametrize("s", OTHER_STREAMS)
@pytest.mark.parametrize("name", sorted(ORTH_CASES))
def test_orthogonal_sketches_gated_on_other_streams(tsa, nat, blocker, name, s):  # noqa: F811
    if name not in _orth:
        _orth[name] = OrthSetup(tsa, name)
    su = _orth[name]
    deferred_flags(nat)                                           # (whatever earlier tests left)
    if su.refs is None:
        # the reference of the bits: the call twice on stream 0, synchronously; only if these agree is another stream held to them
        a, b = OrthCall(nat, su, 0).plain(), OrthCall(nat, su, 0).plain()
        agree = all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a, b))
        print("%s: two synchronous calls on stream 0 %s in their bits" % (name, "agree" if agree else "DO NOT agree"))
        su.refs = (agree, a)
        if su.form is not None:
            probe = OrthCall(nat, su, 0, probe=True)
            got = probe.verdicts(probe.plain())
            want = [1] * su.count if su.form == "fused" else [1 if b == su.probe_at else 0 for b in range(su.count)]
            assert got == want, "%s does not run in the %s form it is there for: verdicts %s" % (name, su.form, got)
        deferred_flags(nat)
    call = OrthCall(nat, su, s)
    (flats,) = in_flight(nat, blocker, [call], call.what)
    flags = deferred_flags(nat)
    call.check(flats)
    verdicts = call.verdicts(flats)
    # Verdicts: the single call leaves them in the deferred flag of ITS stream (helpers carry none); the batch hands every
    # tensor's verdict back in dev_status and leaves the flag of every stream it used clear (include/ttsk.h).
    assert [f for t, f in enumerate(flags) if t != s] == [0] * 7, (call.what, flags)
    assert flags[s] == 0, (call.what, flags)
    if verdicts is not None:
        assert verdicts == [1 if b == su.low_at else 0 for b in range(su.count)], (call.what, verdicts)
    agree, ref = su.refs
    if agree:                                                     # (the rejected tensor's meaningless cores included: same kernels, same bits)
        same_bits(flats, ref, call.what + " against the synchronous call on stream 0")


class AssembleCall(DriverCall):
    """ttsk_tt_assemble / _batch, direction "right", of Gaussian Psi and Omega: C_mu = Psi_mu pinv(Omega_mu), the last core copied"""

    def __init__(self, nat, name, stream):  # noqa: F811
        shape, lr, rr, count = ASSEMBLE_CASES[name]
        d = len(shape)
        self.nat, self.stream, self.count, self.d = nat, stream, count, d
        self.what = "assembly %s on stream %d" % (name, stream)
        rng = np.random.default_rng(sum(map(ord, name)))
        psi, om = [], []
        for _ in range(count or 1):
            psi += [rng.standard_normal((1 if mu == 0 else lr[mu - 1], shape[mu], 1 if mu == d - 1 else rr[mu])) for mu in range(d)]
            om += [rng.standard_normal((lr[mu], rr[mu])) for mu in range(d - 1)]
        self.operands = sk.Staged(nat, psi + om, stream)
        self.want_cores, self.want_pinv = [], []
        for b in range(count or 1):
            for mu in range(d):
                P = psi[b * d + mu]
                if mu < d - 1:
                    pinv = np.linalg.pinv(om[b * (d - 1) + mu])
                    self.want_pinv.append(pinv)
                    P = (P.reshape(-1, rr[mu]) @ pinv).reshape(P.shape[0], shape[mu], lr[mu])
                self.want_cores.append(P)
        sizes = [w.size for w in self.want_cores + self.want_pinv]
        self.outs = sk.Outs(nat, sizes, 1, stream, even=True)
        npsi = len(psi)
        self.psi = (ctypes.c_void_p * npsi)(*self.operands.ptrs[:npsi])
        self.om = (ctypes.c_void_p * len(om))(*self.operands.ptrs[npsi:])
        self.cores, self.work = self.out_ptrs(0, npsi), self.out_ptrs(npsi, len(sizes))
        self.dims = (d, nat.i64_array(shape), nat.i64_array(lr), nat.i64_array(rr))

    def entry(self):
        if self.count is None:
            self.nat.call("ttsk_tt_assemble", *self.dims, self.psi, self.om, self.cores, self.work, 0, self.stream)
        else:
            self.nat.call("ttsk_tt_assemble_batch", self.count, *self.dims, self.psi, self.om, self.cores, self.work, 0, self.stream)

    def check(self, flats):
        want = self.want_cores + self.want_pinv
        _close([f.reshape(w.shape) for f, w in zip(flats, want)], want)



@pytest.mark.parametrize("s", OTHER_STREAMS)
@pytest.mark.parametrize("name", sorted(ASSEMBLE_CASES))
def test_assemblies_gated_on_other_streams(tsa, nat, blocker, name, s):  # noqa: F811
    if name not in _assemble_refs:
        a, b = AssembleCall(nat, name, 0).plain(), AssembleCall(nat, name, 0).plain()
        agree = all(np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a, b))
        print("%s: two synchronous calls on stream 0 %s in their bits" % (name, "agree" if agree else "DO NOT agree"))
        _assemble_refs[name] = (agree, a)
    call = AssembleCall(nat, name, s)
    (flats,) = in_flight(nat, blocker, [call], call.what)
    call.check(flats)
    agree, ref = _assemble_refs[name]
    if agree:
        same_bits(flats, ref, call.what + " against the synchronous call on stream 0")
