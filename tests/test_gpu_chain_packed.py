"""ttsk_chain_step with its DRM core packed (ttsk_drm_pack, csrc/chain_pack.hip) against the same call on the unregistered
core: the packed image is byte for byte the LDS image the gather loader builds, so Out and T must be EQUAL
(np.array_equal), not close.  Shapes: the smallest that reach each loader variant of chain_step_kernel -- the levelled
12-wave deal with one E image (rank 100, right) and with two (rank 50, left, T stored), an image that is no whole number of
1 KB pieces before padding (A = 52: 1300 units), each at the two batch shapes of test_gpu_chain_level.py (unequal slice
ranges; phase A in runs of 25 and of 5), and the 8-wave deal of a single tensor with few rows."""
import ctypes

import numpy as np
import pytest

from tests.edge_kit import nat  # noqa: F401

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
BATCHES = ((32, 19, 100), (1, 600, 52))      # (nb, n, K1) of test_gpu_chain_level.py
CASES = [(J, A, A2, right, wt, nb, n, K1) for (J, A, A2, right, wt) in ((100, 100, 100, True, False), (100, 50, 50, False, True),
                                                                         (97, 52, 50, False, True))
         for (nb, n, K1) in BATCHES] + [(48, 100, 100, True, False, 1, 40, 100)]


class Step:
    """one chain step's operands on the device; run() -> (Out, T) of every tensor on the host"""

    def __init__(self, nat, seed, J, A, A2, right, wt, nb, n, K1):
        from tt_sketch_amd.device import DevArray
        rng = np.random.default_rng(seed)
        self.nat, self.dims, self.wt, self.nb = nat, (nb, n, K1, A, A2, J), wt, nb
        self.strides = (n * K1, K1, 1) if right else (1, J, n * J)
        self.xsize = J * n * K1
        self.W = [DevArray.from_host(rng.standard_normal((K1, A))) for _ in range(nb)]
        self.X = [DevArray.from_host(rng.standard_normal((J, n, K1) if right else (K1, n, J))) for _ in range(nb)]
        self.E = DevArray.from_host(rng.standard_normal((A, n, A2)))
        self.core = (A, n, A2)

    def run(self):
        from tt_sketch_amd.device import DevArray, sync
        nb, n, K1, A, A2, J = self.dims
        out = [DevArray.from_host(np.full((J, A2), np.nan)) for _ in range(nb)]
        T = [DevArray.from_host(np.full((A, n, J), np.nan)) for _ in range(nb)] if self.wt else None
        arr = lambda xs: (P * nb)(*[x.ptr for x in xs])
        self.nat.call("ttsk_chain_step", nb, n, K1, A, A2, J, arr(self.W), A, arr(self.X), *self.strides, self.xsize, P(self.E.ptr),
                      arr(T) if self.wt else None, arr(out), 0)
        sync()
        return [o.get() for o in out], [t.get() for t in T] if self.wt else []

    def pack(self, A=None, n=None, A2=None):
        a, k, a2 = self.core
        self.nat.call("ttsk_drm_pack", P(self.E.ptr), A or a, n or k, A2 or a2, 0)

    def unpack(self):
        self.nat.call("ttsk_drm_unpack", P(self.E.ptr))


def same(got, want):
    for g, w in zip(got[0] + got[1], want[0] + want[1]):
        assert not np.isnan(w).any() and np.array_equal(g, w)
    assert len(got[0]) == len(want[0]) and len(got[1]) == len(want[1])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "J%d-A%d-%d-%s-%s-nb%d-n%d-K%d" % (c[0], c[1], c[2], "right" if c[3] else "left",
                                                                                        "T" if c[4] else "noT", c[5], c[6], c[7]))
def test_packed_core_gives_the_same_bits(nat, case):
    s = Step(nat, 11, *case)
    want = s.run()
    s.pack()
    try:
        got = s.run()
    finally:
        s.unpack()
    same(got, want)


def test_a_packed_run_reads_the_image_not_the_core(nat):
    """equal results could also mean that the registration was never found.  Here the core is zeroed behind the library's
    back while it is registered (what no caller may do): a run that still gives the original result has read every slice
    from the image; after ttsk_drm_unpack the same call sees the zeros."""
    s = Step(nat, 14, 100, 50, 50, False, True, 2, 24, 52)
    want = s.run()
    s.pack()
    try:
        nat.call("ttsk_memset", P(s.E.ptr), 0, ctypes.c_size_t(8 * 50 * 24 * 50), 0)
        same(s.run(), want)
    finally:
        s.unpack()
    out, T = s.run()
    assert all(not o.any() for o in out)
    same((out[:0], T), (want[0][:0], want[1]))           # T does not depend on E


def test_other_extents_take_the_gather_path_and_unpack_restores_it(nat):
    """registered as (A, n, A2) = (50, n / 2, 100) -- the same bytes seen as another core -- and called as (50, n, 50): the
    registration does not match, the loader gathers, the result is the unregistered one; then registered as it is, and
    after ttsk_drm_unpack again"""
    J, A, A2, right, wt, nb, n, K1 = 100, 50, 50, False, True, 2, 24, 52
    s = Step(nat, 12, J, A, A2, right, wt, nb, n, K1)
    want = s.run()
    s.pack(A=50, n=n // 2, A2=100)
    try:
        same(s.run(), want)
        s.pack()                     # registering the true extents replaces the other registration
        same(s.run(), want)
    finally:
        s.unpack()
    same(s.run(), want)
    s.unpack()                       # unregistered: a no-op


def test_pack_refuses_ranks_without_an_image(nat):
    from tt_sketch_amd.device import DevArray
    E = DevArray.from_host(np.zeros((18, 5, 3)))
    with pytest.raises(nat.TtskUnsupported):
        nat.call("ttsk_drm_pack", P(E.ptr), 18, 5, 3, 0)
    nat.call("ttsk_drm_unpack", P(E.ptr))


REINIT_CHILD = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, %(root)r)
from tt_sketch_amd import _native as nat
from tests.test_gpu_chain_packed import Step, same
nat.call("ttsk_init", 0)
s = Step(nat, 13, 100, 50, 50, False, True, 2, 24, 52)
want = s.run()
s.pack()
nat.call("ttsk_memset", ctypes.c_void_p(s.E.ptr), 0, ctypes.c_size_t(8 * 50 * 24 * 50), 0)
same(s.run(), want)                  # registered: the image is read
nat.call("ttsk_sync", -1)
nat.call("ttsk_shutdown")
nat.call("ttsk_init", 0)
out, T = s.run()                     # the registry is empty: the (zeroed) core is read
assert all(not o.any() for o in out)
s.pack()                             # and a core can be registered again
s.unpack()
print("REGISTRY-EMPTY-OK")
"""


def test_registry_is_empty_after_reinit():
    """ttsk_shutdown + ttsk_init with a core left registered, in a child process (the session's library state is left
    alone): the next call no longer finds the image"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", REINIT_CHILD % dict(root=root)], cwd=root, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "REGISTRY-EMPTY-OK" in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]
