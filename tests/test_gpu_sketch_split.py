"""The one-call TT sketches (ttsk_tt_sketch_batch, ttsk_tt_sketch_sum) under CU budgets (ttsk_tt_sketch_split,
csrc/sketch_split.h): a budget changes the grid of the chain steps and of the Psi products -- how many slices a workgroup
walks, how many slab partials are summed -- and must change nothing else.

Shapes: the smallest that reach the levelled 12-wave deal (two slices or more per workgroup) and both tile structures:
(a) TT rank 68, l = 36, r = 68 on n = (6, 5, 7, 6) with 3 and 5 tensors, (b) the headline structure -- TT rank 100, l = 50,
r = 100 -- at n = 4 with 2 tensors.  Splits: the policy, full width, nearly everything to the right chain, nearly everything to the
left chain and Psi, and halves.

Cores of small integers: every partial sum of every product is an integer below 2^53 (the largest entry, an Omega_0 of
shape (b), is below 2^42), so fp64 is exact whatever the order and the grid: every Psi and Omega must EQUAL the int64
einsum, under every split.  Gaussian cores: the oracle's general_sketch to the tolerance of tests/test_gpu_parity.py for
the one-call path (1e-12 in the Frobenius norm), and a second run of the same split gives the same bits."""
import contextlib
import ctypes
import faulthandler

import numpy as np
import pytest

from oracle import ttsk_oracle as orc
from tests.edge_kit import exact, nat, num_cu, same_bits, tsa  # noqa: F401
from tests.golden_io import rel

pytestmark = pytest.mark.gpu

TOL = 1e-12                 # tests/test_gpu_parity.py: test_batched_one_call_path, test_sketch_of_a_sum_in_one_call
STEP_LIMIT_S = 60           # a GPU step that takes longer has hung: the process ends there

# name -> (mode sizes, TT rank, left rank, right rank, tensors)
SHAPES = {"a3": ((6, 5, 7, 6), 68, 36, 68, 3), "a5": ((6, 5, 7, 6), 68, 36, 68, 5), "b2": ((4, 4, 4, 4), 100, 50, 100, 2)}
SPLITS = ("auto", "full", "right", "left", "halves")


def split_of(name, n_cu, nb):
    return {"auto": (-1, -1, -1), "full": (0, 0, 0), "right": (n_cu - nb, nb, nb), "left": (nb, n_cu - nb, n_cu - nb),
            "halves": (n_cu // 2,) * 3}[name]


@contextlib.contextmanager
def gpu_step(nat, what):
    """One GPU step under its own time limit; a HIP error ends the whole run (the device may have faulted)."""
    faulthandler.dump_traceback_later(STEP_LIMIT_S, exit=True)
    try:
        yield
        nat.call("ttsk_sync", -1)
    except nat.TtskError as e:
        pytest.exit("%s: %s" % (what, e), returncode=3)
    finally:
        faulthandler.cancel_dump_traceback_later()


def int64_sketch(cores, lcores, rcores):
    """Psi_0 .. Psi_{d-1}, Omega_0 .. Omega_{d-2} of one tensor train in int64 einsums (full rank ranges).  rcores in the right
    DRM's walking order (mode d-1 first)."""
    d = len(cores)
    X = [np.rint(c).astype(np.int64) for c in cores]
    D = [np.rint(c).astype(np.int64) for c in lcores]
    E = [np.rint(c).astype(np.int64) for c in rcores]
    L, T = [np.einsum("kp,kq->pq", X[0][0], D[0][0])], [None]
    for mu in range(1, d):
        T.append(np.einsum("pq,pks->qks", L[mu - 1], X[mu]))
        if mu < d - 1:
            L.append(np.einsum("qks,qkt->st", T[mu], D[mu]))
    R = [np.einsum("sk,kq->sq", X[d - 1][:, :, 0], E[0][0])]
    for j in range(1, d - 1):
        TR = np.einsum("pq,skp->qks", R[j - 1], X[d - 1 - j])
        R.append(np.einsum("qks,qkt->st", TR, E[j]))
    Psi = [np.einsum("aks,sc->akc", X[0], R[d - 2])]
    Psi += [np.einsum("qks,sc->qkc", T[mu], R[d - 2 - mu]) for mu in range(1, d - 1)]
    Psi.append(T[d - 1])
    Om = [np.einsum("sq,sc->qc", L[mu], R[d - 2 - mu]) for mu in range(d - 1)]
    return Psi + Om


class Case:
    """The tensors, the DRMs and the references of one shape, for integer and for Gaussian cores: built once per module."""

    def __init__(self, name):
        shape, s, l, r, nb = SHAPES[name]
        self.nb = nb
        rng = np.random.default_rng(sum(map(ord, name)))
        self.data = {}
        for kind in ("int", "gauss"):
            ld, rd = orc.random_tt_drm(shape, l, False, rng), orc.random_tt_drm(shape, r, True, rng)
            tts = [orc.random_tt(shape, s, rng) for _ in range(nb)]
            if kind == "int":
                for cs in [ld.cores, rd.cores] + tts:
                    for i, c in enumerate(cs):
                        cs[i] = rng.integers(-1, 2, size=c.shape).astype(np.float64)
                want = [int64_sketch(c, ld.cores, rd.cores) for c in tts]
                assert max(int(np.abs(a).max()) for w in want for a in w) * nb < 2**53
                for w, c in zip(want, tts):          # the einsums above follow the oracle's conventions (exact in fp64 too)
                    oP, oO = orc.general_sketch("tt", c, ld, rd, "streaming")
                    for a, b in zip(w, oP + oO):
                        assert a.shape == b.shape and np.array_equal(a.astype(np.float64), b)
                want = [[a.astype(np.float64) for a in w] for w in want]
            else:
                want = []
                for c in tts:
                    oP, oO = orc.general_sketch("tt", c, ld, rd, "streaming")
                    want.append(list(oP + oO))
            self.data[kind] = (ld, rd, tts, want, [sum(w[i] for w in want) for i in range(len(want[0]))])
        self.dev = {}

    def on_device(self, kind):
        """-> (plan, X pointers, keep-alive) of the tensors of `kind`"""
        if kind not in self.dev:
            from tests.gpu_build import make_drm, make_tensor
            from tt_sketch_amd import tt_fused
            ld, rd, tts, _, _ = self.data[kind]
            L, R = make_drm(ld), make_drm(rd)
            dev = [make_tensor("tt", c) for c in tts]
            plan = tt_fused.TTSketchPlan(dev[0].shape, dev[0].rank, L, R)
            keep, flat = [dev, L, R], []
            for t in dev:
                ptrs, k = plan.core_pointers(t)
                keep.append(k)
                flat += [ptrs[i] for i in range(plan.d)]
            self.dev[kind] = (plan, (ctypes.c_void_p * len(flat))(*flat), keep)
        return self.dev[kind]


_cases = {}


@pytest.fixture(scope="module")
def cases():
    def get(name):
        if name not in _cases:
            _cases[name] = Case(name)
        return _cases[name]
    yield get
    _cases.clear()


def sketches(nat, case, kind, split, what):
    """-> (the nb sketches of the batch call, the sketch of the sum call), each a list of host arrays Psi + Omega"""
    from tt_sketch_amd.device import DevArray
    plan, X, _ = case.on_device(kind)
    nb, stride = case.nb, plan.size + 5
    out, out_sum = DevArray.zeros((nb * stride,)), DevArray.zeros((plan.size,))
    nat.call("ttsk_tt_sketch_split", *split)
    try:
        with gpu_step(nat, what + " batch"):
            plan.run_batch(X, nb, out, stride)
        with gpu_step(nat, what + " sum"):
            plan.run_sum(X, nb, out_sum)
    finally:
        nat.call("ttsk_tt_sketch_split", -1, -1, -1)
    per = []
    for b in range(nb):
        Psi, Om = plan.views(out[b * stride:b * stride + plan.size])
        per.append([a.get() for a in Psi + Om])
    Psi, Om = plan.views(out_sum)
    return per, [a.get() for a in Psi + Om]


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_integer_cores_equal_the_int64_einsum_under_every_split(tsa, nat, num_cu, cases, shape, split):  # noqa: F811
    case = cases(shape)
    what = "%s %s" % (shape, split)
    per, total = sketches(nat, case, "int", split_of(split, num_cu, case.nb), what)
    _, _, _, want, want_sum = case.data["int"]
    for b, (got, w) in enumerate(zip(per, want)):
        for i, (a, c) in enumerate(zip(got, w)):
            exact(a, c, "%s tensor %d piece %d" % (what, b, i))
    for i, (a, c) in enumerate(zip(total, want_sum)):
        exact(a, c, "%s sum piece %d" % (what, i))


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_gaussian_cores_match_the_oracle_and_repeat_their_bits(tsa, nat, num_cu, cases, shape, split):  # noqa: F811
    case = cases(shape)
    what = "%s %s" % (shape, split)
    cfg = split_of(split, num_cu, case.nb)
    per, total = sketches(nat, case, "gauss", cfg, what)
    _, _, _, want, want_sum = case.data["gauss"]
    for b, (got, w) in enumerate(zip(per, want)):
        for i, (a, c) in enumerate(zip(got, w)):
            r = rel(a, c)
            print("%s tensor %d piece %d: rel %.3e" % (what, b, i, r))
            assert a.shape == c.shape and r < TOL, (what, b, i, r)
    for i, (a, c) in enumerate(zip(total, want_sum)):
        r = rel(a, c)
        print("%s sum piece %d: rel %.3e" % (what, i, r))
        assert a.shape == c.shape and r < TOL, (what, "sum", i, r)
    per2, total2 = sketches(nat, case, "gauss", cfg, what + " (second run)")
    same_bits(per, per2, what + ": the batch's sketches of two runs")
    same_bits(total, total2, what + ": the sum's sketch of two runs")


def test_the_setting_is_checked_and_restored(nat):  # noqa: F811
    with pytest.raises(ValueError):
        nat.call("ttsk_tt_sketch_split", -2, 0, 0)
    nat.call("ttsk_tt_sketch_split", -1, -1, -1)
