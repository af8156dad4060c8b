"""bench.py --dump-outputs: what dump_sketches writes (host arrays only, no device needed)."""
import os

import numpy as np

import bench


def _sketch(rng, shape, left, right):
    lr, rr = (1,) + left, right + (1,)
    psis = [rng.standard_normal((lr[mu], n, rr[mu])) for mu, n in enumerate(shape)]
    omegas = [rng.standard_normal((left[mu], right[mu])) for mu in range(len(shape) - 1)]
    return psis, omegas


def _packed(sk):
    return np.concatenate([a.ravel() for a in sk[0] + sk[1]])


def _files(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_first_sketch_whole_and_every_sketch_sampled(tmp_path):
    rng = np.random.default_rng(0)
    sks = [_sketch(rng, (7, 8, 9), (3, 4), (5, 6)) for _ in range(3)]
    bench.dump_sketches(str(tmp_path), sks[0], [lambda s=s: _packed(s) for s in sks])
    got = _files(str(tmp_path))
    assert sorted(got) == ["omega_0", "omega_1", "psi_0", "psi_1", "psi_2", "sketch_norms", "sketch_sample"]
    assert all(a.dtype == np.float64 for a in got.values())
    for mu, a in enumerate(sks[0][0]):
        np.testing.assert_array_equal(got[f"psi_{mu}"], a)
    for mu, a in enumerate(sks[0][1]):
        np.testing.assert_array_equal(got[f"omega_{mu}"], a)
    np.testing.assert_allclose(got["sketch_norms"], [np.linalg.norm(_packed(s)) for s in sks])
    size = _packed(sks[0]).size
    assert got["sketch_sample"].shape == (3, min(size, bench.DUMP_SAMPLE_COLS))
    # the sampled positions are the same in every row and in every run
    bench.dump_sketches(str(tmp_path / "again"), sks[1], [lambda: _packed(sks[1])])
    np.testing.assert_array_equal(_files(str(tmp_path / "again"))["sketch_sample"][0], got["sketch_sample"][1])


def test_dump_stays_within_its_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 << 10)
    rng = np.random.default_rng(1)
    big = _sketch(rng, (40, 40, 40), (20, 20), (20, 20))          # 8 * 33 200 bytes: more than half the budget
    bench.dump_sketches(str(tmp_path), big, [lambda: _packed(big)] * 5)
    got = _files(str(tmp_path))
    assert sorted(got) == ["sketch_norms", "sketch_sample"]
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_LIMIT_BYTES
    assert got["sketch_sample"].shape[0] == 5
