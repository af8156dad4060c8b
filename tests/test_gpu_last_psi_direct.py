"""Psi_{d-1} of ttsk_tt_sketch_batch: the left chain's last product T_{d-1} = L_{d-2}[:, l_lo:l_hi]^T X_{d-1} is written
straight into each sketch (csrc/tt_fused.hip, left_step) instead of to the workspace and copied (or added) from there.
Checked against the oracle at test_gpu_parity's TOL for whole and sliced left ranks, overwriting and accumulating; an
overwriting call on a NaN-filled `out` must leave no NaN in Psi_{d-1} (every element is stored, none is added to)."""
import ctypes

import numpy as np
import pytest

from oracle import ttsk_oracle as orc
from tests.golden_io import rel
from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

TOL = 1e-12      # test_gpu_parity.TOL
SHAPE, TT_RANK, NB = (6, 7, 5, 9), (3, 5, 4), 3
LEFT, RIGHT = (4, 6, 5), (5, 7, 6)
# (left rank_min, left rank_max): the whole ranks, and a slice whose last entry -- the rows of Psi_{d-1} -- starts above 0
SLICES = {"whole": ((0, 0, 0), LEFT), "sliced": ((1, 0, 2), (4, 5, 5))}


@pytest.fixture(scope="module", params=sorted(SLICES))
def setup(request, tsa):
    """the plan, the device tensors and the oracle's sketches of one rank slice, computed once"""
    from tests.gpu_build import make_drm, make_tensor
    from tt_sketch_amd import tt_fused
    rng = np.random.default_rng(41)
    ld, rd = orc.random_tt_drm(SHAPE, LEFT, False, rng), orc.random_tt_drm(SHAPE, RIGHT, True, rng)
    ld.rank_min, ld.rank_max = SLICES[request.param]
    rd.rank_min, rd.rank_max = (0, 2, 1), (5, 6, 5)          # walking order of the right DRM: ranks (6, 7, 5)
    L, R = make_drm(ld), make_drm(rd)
    tts = [orc.random_tt(SHAPE, TT_RANK, rng) for _ in range(NB)]
    dev = [make_tensor("tt", c) for c in tts]
    plan = tt_fused.TTSketchPlan(dev[0].shape, dev[0].rank, L, R)
    keep, flat = [], []
    for t in dev:
        ptrs, k = plan.core_pointers(t)
        keep.append(k)
        flat += [ptrs[i] for i in range(plan.d)]
    X = (ctypes.c_void_p * len(flat))(*flat)
    want = []
    for cores in tts:
        oP, oO = orc.general_sketch("tt", cores, ld, rd, "streaming")
        want.append([np.asarray(a) for a in oP + oO])
    assert want[0][len(SHAPE) - 1].shape == (ld.rank_max[2] - ld.rank_min[2], SHAPE[-1], 1)
    return plan, X, want, (keep, dev, L, R)


@pytest.mark.parametrize("accumulate", (0, 1))
def test_last_psi_against_the_oracle(setup, accumulate):
    from tt_sketch_amd.device import DevArray
    plan, X, want, _ = setup
    stride = plan.size + 5                                    # odd offsets: Psi_{d-1} of the second sketch is not 16-byte aligned
    before = np.random.default_rng(5).standard_normal(NB * stride)
    out = DevArray.from_host(before)
    plan.run_batch(X, NB, out, stride, accumulate=bool(accumulate))
    got_all = out.get()
    for b in range(NB):
        Psi, Om = plan.views(out[b * stride:b * stride + plan.size])
        off = 0
        for mu, (a, w) in enumerate(zip(Psi + Om, want[b])):
            base = before[b * stride + off:b * stride + off + w.size].reshape(w.shape) if accumulate else 0.0
            err = rel(a.get(), w + base)
            print("sketch", b, "part", mu, "accumulate", accumulate, err)
            assert err < TOL, (b, mu, err)
            off += w.size
        assert off == plan.size
        # the padding between two sketches is nobody's
        assert np.array_equal(got_all[b * stride + plan.size:(b + 1) * stride], before[b * stride + plan.size:(b + 1) * stride])


def test_overwriting_call_stores_every_element_of_the_last_psi(setup):
    from tt_sketch_amd.device import DevArray
    plan, X, want, _ = setup
    stride = plan.size + (plan.size & 1)
    out = DevArray.from_host(np.full(NB * stride, np.nan))
    plan.run_batch(X, NB, out, stride, accumulate=False)
    d = len(SHAPE)
    for b in range(NB):
        Psi, _ = plan.views(out[b * stride:b * stride + plan.size])
        last = Psi[d - 1].get()
        assert not np.isnan(last).any(), (b, np.argwhere(np.isnan(last))[:4])
        assert rel(last, want[b][d - 1]) < TOL
