"""Plain NumPy restatement of TensorTrain.gather / CPTensor.gather and of the sums the device pass forms.

The TT chain runs left to right, t_e = G_0[0, i_0, :] G_1[:, i_1, :] ... G_{d-1}[:, i_{d-1}, 0], one row of the
running vector at a time (``nxt += v[:, a] * G_k[a, i_k, :]``), so no (r, N, r') array is ever built, and in chunks
of the index list, so the temporaries stay cache sized whatever N is.  ``absolute=True`` evaluates the same chain on
|cores|: the scale s_e that an element-wise error bound is stated against.
"""
import numpy as np

CHUNK = 1 << 14


def tt_gather(cores, idx, absolute=False, chunk=CHUNK):
    cs = [np.abs(np.asarray(c)) if absolute else np.asarray(c) for c in cores]
    idx = np.asarray(idx)
    N = idx.shape[1]
    out = np.empty(N)
    for lo in range(0, N, chunk):
        sl = idx[:, lo:lo + chunk]
        v = cs[0][0][sl[0]]                              # (m, r_1)
        for k in range(1, len(cs)):
            c = cs[k]
            nxt = np.zeros((v.shape[0], c.shape[2]))
            for a in range(c.shape[0]):
                nxt += v[:, a:a + 1] * c[a][sl[k]]
            v = nxt
        out[lo:lo + chunk] = v[:, 0]
    return out


def cp_gather(factors, idx, absolute=False, chunk=CHUNK):
    fs = [np.abs(np.asarray(f)) if absolute else np.asarray(f) for f in factors]
    idx = np.asarray(idx)
    N = idx.shape[1]
    out = np.empty(N)
    for lo in range(0, N, chunk):
        sl = idx[:, lo:lo + chunk]
        acc = fs[0][sl[0]]
        for k in range(1, len(fs)):
            acc = acc * fs[k][sl[k]]
        out[lo:lo + chunk] = acc.sum(axis=1)
    return out


def stats(t, x):
    """(sum x t, sum t^2, sum (t - x)^2) and, per sum, the sum of the absolute values of its terms."""
    t, x = np.asarray(t), np.asarray(x)
    r = t - x
    return (np.array([np.sum(x * t), np.sum(t * t), np.sum(r * r)]),
            np.array([np.sum(np.abs(x * t)), np.sum(t * t), np.sum(r * r)]))


def fast_error(norm_self, norm_other, dot, relative=True):
    """Tensor.error(fast=True) (reference tensor.py:68-78) from its three ingredients."""
    tot = norm_self ** 2 + norm_other ** 2
    err = np.sqrt(tot) * np.sqrt(abs(1 - 2 * dot / tot))
    return err / norm_other if relative else err


def tt_norm(cores):
    """|| tt || by the Gram chain (sums of squares only: nothing cancels)."""
    acc = np.ones((1, 1))
    for c in cores:
        c = np.asarray(c)
        acc = np.einsum("ij,ika,jkb->ab", acc, c, c, optimize=True)
    return float(np.sqrt(acc[0, 0]))


def load_cases(path=None):
    """The fixtures of tests/golden/make_golden_gather.py (runs of the reference) as a list of dicts."""
    import json
    import os
    if path is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gather_cases.npz")
    z = np.load(path)
    cases = []
    for name, m in json.loads(str(z["meta"])).items():
        shape, d = tuple(m["shape"]), len(m["shape"])
        rk = (1,) + tuple(m["rank"]) + (1,)
        flat, cores, pos = z[f"{name}/cores"], [], 0
        for k in range(d):
            size = rk[k] * shape[k] * rk[k + 1]
            cores.append(flat[pos:pos + size].reshape(rk[k], shape[k], rk[k + 1]))
            pos += size
        flat, factors, pos = z[f"{name}/factors"], [], 0
        for n in shape:
            factors.append(flat[pos:pos + n * m["cp_rank"]].reshape(n, m["cp_rank"]))
            pos += n * m["cp_rank"]
        dot_tt, dot_cp, norm, err = z[f"{name}/scalars"]
        cases.append(dict(name=name, shape=shape, idx=z[f"{name}/indices"], entries=z[f"{name}/entries"], cores=cores,
                          factors=factors, tt_gather=z[f"{name}/tt_gather"], cp_gather=z[f"{name}/cp_gather"],
                          dot_tt=float(dot_tt), dot_cp=float(dot_cp), norm=float(norm), error=float(err)))
    return cases
