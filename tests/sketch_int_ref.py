"""What the tests of the one-call TT sketches (ttsk_tt_sketch, ttsk_tt_sketch_batch, ttsk_tt_sketch_sum) share: the shapes, the
CU-budget settings, the step limit of a GPU step, and one Case per shape -- tensors, DRMs and references for integer and for
Gaussian cores.  Plain module: it imports nothing of a device until Case.on_device or gpu_step is used.

Shapes: the smallest that reach the levelled 12-wave deal (two slices or more per workgroup) and both tile structures:
(a) TT rank 68, l = 36, r = 68 on n = (6, 5, 7, 6) with 3 and 5 tensors, (b) the headline structure -- TT rank 100, l = 50,
r = 100 -- at n = 4 with 2 tensors and with 8, the smallest batch the policy of csrc/sketch_split.h splits (a pipelined caller,
the fused family, wpp = min(n_cu / 8, 4) = 4 >= 3).

Cores of small integers: every partial sum of every product is an integer below 2^53 (the largest entry, an Omega_0 of
shape (b), is below 2^42), so fp64 is exact whatever the order and the grid: every Psi and Omega must EQUAL the int64
einsum.  Case.__init__ asserts that bound and that the einsums follow the oracle's conventions."""
import contextlib
import ctypes
import faulthandler

import numpy as np
import pytest

from oracle import ttsk_oracle as orc

STEP_LIMIT_S = 60           # a GPU step that takes longer has hung: the process ends there

# name -> (mode sizes, TT rank, left rank, right rank, tensors)
SHAPES = {"a3": ((6, 5, 7, 6), 68, 36, 68, 3), "a5": ((6, 5, 7, 6), 68, 36, 68, 5), "b2": ((4, 4, 4, 4), 100, 50, 100, 2),
          "b8": ((4, 4, 4, 4), 100, 50, 100, 8)}


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
        self.name, self.shape, self.s, self.l, self.r = name, shape, s, l, r
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
