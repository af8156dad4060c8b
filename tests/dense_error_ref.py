"""Plain NumPy restatement of what the device pass of a tensor train over a dense tensor forms (csrc/tt_dense_stats.hip):
the full tensor, the four sums with the sums of the absolute values of their terms, and the scale
``s = full(|cores|) + |x|`` that the element-wise and the residual bounds are stated against.
"""
import json
import os

import numpy as np


def full(cores, absolute=False):
    """The dense tensor of a train, mode by mode from the left."""
    cs = [np.abs(np.asarray(c)) if absolute else np.asarray(c) for c in cores]
    acc = cs[0].reshape(cs[0].shape[1], cs[0].shape[2])
    for c in cs[1:]:
        acc = (acc @ c.reshape(c.shape[0], -1)).reshape(-1, c.shape[2])
    return acc.reshape([c.shape[1] for c in cs])


def stats(t, x):
    """(sum x t, sum t^2, sum (t - x)^2, sum x^2) and, per sum, the sum of the absolute values of its terms."""
    t, x = np.asarray(t, dtype=np.float64).ravel(), np.asarray(x, dtype=np.float64).ravel()
    r = t - x
    return (np.array([np.sum(x * t), np.sum(t * t), np.sum(r * r), np.sum(x * x)]),
            np.array([np.sum(np.abs(x * t)), np.sum(t * t), np.sum(r * r), np.sum(x * x)]))


def scale(cores, x):
    """s = full(|cores|) + |x|: what a rounding error of an entry of t - x is measured against."""
    return full(cores, absolute=True) + np.abs(np.asarray(x))


def fast_error(tt_sq, x_sq, dot):
    """Tensor.error(fast=True) (reference tensor.py:68-72) from <t, t>, <x, x> and <x, t>."""
    tot = tt_sq + x_sq
    return np.sqrt(tot) * np.sqrt(abs(1 - 2 * dot / tot))


def errors(s, size):
    """The recorded figures of a fixture case from the four sums: plain, relative, rmse, fast, dot, ||x||."""
    return dict(error=np.sqrt(s[2]), relative=np.sqrt(s[2] / s[3]), rmse=np.sqrt(s[2] / size),
                fast=fast_error(s[1], s[3], s[0]), dot=s[0], norm=np.sqrt(s[3]))


def split_cores(flat, shape, rank):
    rk = (1,) + tuple(rank) + (1,)
    cores, pos = [], 0
    for k, n in enumerate(shape):
        size = rk[k] * n * rk[k + 1]
        cores.append(flat[pos:pos + size].reshape(rk[k], n, rk[k + 1]))
        pos += size
    return cores


def load_cases(path=None):
    """The fixtures of tests/golden/make_golden_dense_error.py (runs of the reference) as a list of dicts.  A case with
    ``transposed`` holds the cores and the array of the tensor as the reference saw them: ``x`` is then a ``.T`` view
    (reversed strides) of the C-ordered buffer ``x_buffer``."""
    if path is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_error_cases.npz")
    z = np.load(path)
    cases = []
    for name, m in json.loads(str(z["meta"])).items():
        shape = tuple(m["shape"])
        buf = z[f"{name}/x"]
        x = buf.T if m["transposed"] else buf
        assert x.shape == shape
        err, rel, rmse, fast, dot, norm = z[f"{name}/scalars"]
        cases.append(dict(name=name, shape=shape, rank=tuple(m["rank"]), transposed=m["transposed"], exact=m["exact"],
                          cores=split_cores(z[f"{name}/cores"], shape, m["rank"]), x=x, x_buffer=buf,
                          error=float(err), relative=float(rel), rmse=float(rmse), fast=float(fast), dot=float(dot),
                          norm=float(norm)))
    return cases
