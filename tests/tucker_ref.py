"""NumPy restatement of the evaluation of a Tucker tensor at an index list,
    t_e = sum_{a_1..a_d} C[a_1..a_d] prod_k U_k[a_k, i_k(e)],      C (s_1..s_d), U_k (s_k, n_k),
of its inner products with a Tucker tensor, a tensor train and a CP tensor, and of the numbers of tucker_gather_plan.h, in
float64 or any other dtype for a check of the bars.  No array of the size of the tensor is formed anywhere.

The bars are derived, not measured.  With u = 2^-53 a sum of depth L over terms with absolute values summing to T_abs
is off by at most L u T_abs to first order in ANY order of the additions; the bars are twice that for the second-order
terms.
  * An entry.  ``ttsk_tucker_gather`` forms per tuple the d factor products and sums the P = prod_{k<m} s_k rows through the
    matrix instructions in ascending blocks of four, then the Q = prod_{k>=m} s_k columns as column tiles and a butterfly
    over 16 lanes (tucker_gather.hip): the plan's ``depth`` d + 4 ceil(P / 4) + 8 counts the padding too.  Additions of
    the exact zeros of the padding round nothing, so a term passes at most prod s_k - 1 rounding additions in any order,
    and at most d rounding products (m - 1 for the row factors, d - m - 1 for the column factors, one inside the matrix
    instruction, one for the column weight).  The bar uses L = prod s_k + d:  |t - t_true| <= 2 (prod s_k + d) u T_abs,
    T_abs the same formula on |C| and |U_k|.
  * The three sums over the list (x . t, t . t, |t - x|^2) add N terms, each carrying the error of its entry: the bar is
    the entries' bars propagated plus 2 (N + 3) u of the sum of the |terms| (any order of N additions, two roundings
    for the product and one for t - x).
  * The inner products (tensor_tucker.py) are chains of contractions: every term passes sums over the n_k (the factor
    products), over the s_k mode by mode and a closing sum.  Depths:
      tucker x tucker   sum_k n_k + sum_k s_k + prod s'_k + 2 d
      tucker x tt       sum_k n_k r_{k-1} + prod s_k + sum_k r_k + 2 d      (ttsk_tt_dense_stats sums over the core)
      tucker x cp       sum_k n_k + sum_k s_k + R + 2 d
    and the bar is 2 L u of the same chain on absolute values.
tests/test_tucker_gather_host.py holds float64 NumPy against np.longdouble inside every bar.
"""
import numpy as np

U53 = 2.0 ** -53

# tucker_gather_plan.h
MAX_MODES = 8
MAX_CORE = 1 << 20
MAX_EXTENT = 2 ** 31 - 1
TILES = 4
BATCH = 256
MAX_CT = 4
KC = 16
A_PITCH = 80
WG_PER_CU = 3
LDS_LIMIT = 64 * 1024 - 512
TAIL_SUMS = MAX_CT + 4
BLOCK_SUMS = 8
CHIP_CUS = 256


def prod(xs):
    out = 1
    for x in xs:
        out *= int(x)
    return out


# ---- the gather
def gather(factors, core, idx, dtype=np.float64, absolute=False, chunk=1 << 12):
    """t (N,) in ``dtype``: mode 0 by a matrix product, the other modes one by one with the tuple as batch index"""
    fs = [np.abs(np.asarray(U, dtype=dtype)) if absolute else np.asarray(U, dtype=dtype) for U in factors]
    C = np.abs(np.asarray(core, dtype=dtype)) if absolute else np.asarray(core, dtype=dtype)
    idx = np.asarray(idx)
    N = idx.shape[1]
    out = np.empty(N, dtype=dtype)
    for lo in range(0, N, chunk):
        sl = idx[:, lo:lo + chunk]
        v = fs[0][:, sl[0]].T @ C.reshape(C.shape[0], -1)
        for k in range(1, len(fs)):
            v = np.einsum("esr,se->er", v.reshape(v.shape[0], C.shape[k], -1), fs[k][:, sl[k]])
        out[lo:lo + chunk] = v[:, 0]
    return out


def entry_depth(ranks):
    return prod(ranks) + len(ranks)


def entry_bar(factors, core, idx):
    """2 L u T_abs per entry, L = prod s_k + d"""
    return 2.0 * entry_depth(np.shape(core)) * U53 * gather(factors, core, idx, absolute=True)


def stats(t, x):
    """(sum x t, sum t^2, sum (t - x)^2)"""
    t, x = np.asarray(t), np.asarray(x)
    r = t - x
    return np.array([np.sum(x * t), np.sum(t * t), np.sum(r * r)])


def stats_bar(t_true, x, bar):
    """the bars of the three sums for entries within ``bar`` of ``t_true``"""
    t, x, bar = np.abs(np.asarray(t_true, dtype=np.float64)), np.asarray(x, dtype=np.float64), np.asarray(bar, dtype=np.float64)
    r = np.abs(np.asarray(t_true, dtype=np.float64) - x) + 2 * U53 * (t + np.abs(x))
    own = 2.0 * (len(x) + 3) * U53
    return np.array([np.sum(np.abs(x) * bar) + own * np.sum(np.abs(x) * t),
                     np.sum(2 * t * bar + bar * bar) + own * np.sum(t * t),
                     np.sum(2 * r * bar + bar * bar) + own * np.sum(r * r) + 4 * U53 * np.sum(r * (t + np.abs(x)))])


# ---- the inner products
def _abs_or(a, dtype, absolute):
    a = np.asarray(a, dtype=dtype)
    return np.abs(a) if absolute else a


def tucker_dot(fa, ca, fb, cb, dtype=np.float64, absolute=False):
    T = _abs_or(ca, dtype, absolute)
    for k, (U, V) in enumerate(zip(fa, fb)):
        M = _abs_or(U, dtype, absolute) @ _abs_or(V, dtype, absolute).T
        T = np.moveaxis(np.tensordot(T, M, axes=(k, 0)), -1, k)
    return (T * _abs_or(cb, dtype, absolute)).sum()


def tucker_dot_bar(fa, ca, fb, cb):
    L = sum(U.shape[1] + U.shape[0] for U in fa) + prod(np.shape(cb)) + 2 * len(fa)
    return 2.0 * L * U53 * float(tucker_dot(fa, ca, fb, cb, absolute=True))


def tucker_tt_dot(factors, core, cores, dtype=np.float64, absolute=False):
    """the projected train against the core, left to right"""
    C = _abs_or(core, dtype, absolute)
    v = C.reshape(1, -1)                                   # (r_0 = 1, s_0 ... s_{d-1})
    for U, G in zip(factors, cores):
        Gp = np.einsum("aib,si->asb", _abs_or(G, dtype, absolute), _abs_or(U, dtype, absolute))
        v = np.einsum("asx,asb->bx", v.reshape(Gp.shape[0], Gp.shape[1], -1), Gp)
    return v.sum()


def tucker_tt_dot_bar(factors, core, cores):
    L = sum(G.shape[0] * G.shape[1] + G.shape[2] for G in cores) + prod(np.shape(core)) + 2 * len(factors)
    return 2.0 * L * U53 * float(tucker_tt_dot(factors, core, cores, absolute=True))


def tucker_cp_dot(factors, core, A, dtype=np.float64, absolute=False):
    C = _abs_or(core, dtype, absolute)
    R = np.shape(A[0])[1]
    v = None
    for k, (U, Ak) in enumerate(zip(factors, A)):
        W = _abs_or(U, dtype, absolute) @ _abs_or(Ak, dtype, absolute)            # (s_k, R)
        if v is None:
            v = W.T @ C.reshape(C.shape[0], -1)
        else:
            v = np.einsum("rsx,sr->rx", v.reshape(R, C.shape[k], -1), W)
    return v.sum()


def tucker_cp_dot_bar(factors, core, A):
    L = sum(U.shape[1] + U.shape[0] for U in factors) + np.shape(A[0])[1] + 2 * len(factors)
    return 2.0 * L * U53 * float(tucker_cp_dot(factors, core, A, absolute=True))


def fast_error(norm_a, norm_b, dot_ab, relative):
    """the reference's fast formula (tensor.py:68-72) on three numbers"""
    tot = norm_a ** 2 + norm_b ** 2
    err = np.sqrt(tot) * np.sqrt(abs(1 - 2 * dot_ab / tot))
    return err / norm_b if relative else err


# ---- the plan's numbers
def b_pitch(ct):
    return 16 if ct == 1 else 16 * ct + 16


def col_tiles(Q):
    ct = -(-Q // 16)
    return 4 if ct == 3 else ct


def split_cost(P, Q, d, m):
    return 4 * (-(-P // 4) * 4) * col_tiles(Q) + P + Q * (d - m)


def plan(ranks, N, n_cu=CHIP_CUS):
    """dict(m, P, Q, ct, chunks, lds, grid, run, depth, stat_depth, flops) of a call inside the cover"""
    d, core = len(ranks), prod(ranks)
    best = None
    for m in range(d, 0, -1):
        Q = prod(ranks[m:])
        if Q > 16 * MAX_CT:
            break
        cost = split_cost(core // Q, Q, d, m)
        if best is None or cost < best[0]:
            best = (cost, m, Q)
    _, m, Q = best
    P, ct = core // Q, col_tiles(Q)
    batches = -(-N // BATCH)
    grid = min(batches, WG_PER_CU * max(n_cu, 1))
    run = -(-batches // grid) if grid else 0
    return dict(m=m, P=P, Q=Q, ct=ct, chunks=-(-P // KC),
                lds=(KC * b_pitch(ct) + 4 * KC * A_PITCH + 256) * 8 + 4 * d * 64 * 4,
                grid=grid, run=run, depth=d + -(-P // 4) * 4 + TAIL_SUMS,
                stat_depth=2 + run + BLOCK_SUMS + -(-grid // 256) + BLOCK_SUMS, flops=2.0 * core * N)


# ---- the cases of the GPU test: (tag, ranks, shape, N, reverse_rows, pad).  Tags name the branch of the plan they reach.
CASES = [
    ("d1_q1", (5,), (9,), 17, False, 0),
    ("d1_two_chunks", (17,), (40,), 65, True, 3),
    ("d2_rank1", (1, 1), (7, 1), 15, False, 0),
    ("d2_ct1_full", (16, 16), (20, 20), 64, False, 0),
    ("d2_ct2", (5, 17), (9, 30), 63, True, 2),
    ("d2_ct3_as_4", (3, 33), (8, 40), 16, False, 0),
    ("d2_ct4", (4, 64), (6, 70), 1, False, 0),
    ("d2_q_over_64", (3, 65), (5, 70), 100, False, 0),
    ("d3_chunks", (17, 16, 33), (21, 18, 35), 300, True, 5),
    ("d3_unit_mode", (4, 1, 3), (6, 1, 5), 257, False, 0),
    ("d3_mixed", (16, 17, 5), (40, 40, 40), 1100, False, 1),
    ("d5_r4", (4, 4, 4, 4, 4), (9, 8, 7, 6, 5), 255, True, 0),
    ("d5_mixed", (1, 3, 4, 5, 3), (2, 5, 6, 7, 4), 513, False, 0),
    ("d8_r2", (2,) * 8, (3, 4, 3, 4, 3, 4, 3, 4), 600, True, 7),
    ("d8_slow_odometer", (3, 2, 1, 3, 2, 2, 3, 2), (4, 3, 2, 4, 3, 3, 4, 3), 130, False, 0),
]


def case_data(tag, ranks, shape, N, integer=False):
    """(factors, core, idx, entries) of a case, seeded by its tag; ``integer``: small integers, so that float64 is exact.
    The list holds index 0 and n_k - 1 in every mode and repeated tuples."""
    rng = np.random.default_rng(sum(map(ord, tag)) + (1 if integer else 0))
    if integer:
        factors = [rng.integers(-2, 3, (s, n)).astype(np.float64) for s, n in zip(ranks, shape)]
        core = rng.integers(-3, 4, ranks).astype(np.float64)
    else:
        factors = [rng.standard_normal((s, n)) for s, n in zip(ranks, shape)]
        core = rng.standard_normal(ranks)
    idx = np.stack([rng.integers(0, n, N) for n in shape]).astype(np.int64).reshape(len(shape), N)
    idx[:, 0] = 0
    idx[:, -1] = np.asarray(shape) - 1
    if N > 4:
        idx[:, N // 2] = idx[:, 1]                          # a repeated tuple
        idx[:, N - 2] = idx[:, 1]
    return factors, core, idx, rng.standard_normal(N)


def random_tt(rng, shape, ranks):
    rk = (1,) + tuple(ranks) + (1,)
    return [rng.standard_normal((rk[k], n, rk[k + 1])) / np.sqrt(rk[k]) for k, n in enumerate(shape)]


def load_cases(path=None):
    """The fixtures of tests/golden/make_golden_tucker.py (runs of the reference) as a list of dicts."""
    import json
    import os
    if path is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tucker_cases.npz")
    z = np.load(path)
    cases = []

    def cut(flat, shapes):
        out, pos = [], 0
        for sh in shapes:
            out.append(flat[pos:pos + prod(sh)].reshape(sh))
            pos += prod(sh)
        return out

    for name, m in json.loads(str(z["meta"])).items():
        shape, ranks, ranks_b = tuple(m["shape"]), tuple(m["ranks"]), tuple(m["ranks_b"])
        rk = (1,) + tuple(m["tt_rank"]) + (1,)
        keys = ("norm", "norm_b", "dot_tucker", "dot_tt", "dot_tt_rev", "dot_cp", "dot_cp_rev", "dot_sparse", "norm_tt",
                "norm_cp", "error_tt", "error_cp", "error_tucker", "error_self_tt")
        cases.append(dict(
            name=name, shape=shape, ranks=ranks, ranks_b=ranks_b,
            factors=cut(z[f"{name}/factors"], [(s, n) for s, n in zip(ranks, shape)]), core=z[f"{name}/core"].reshape(ranks),
            factors_b=cut(z[f"{name}/factors_b"], [(s, n) for s, n in zip(ranks_b, shape)]), core_b=z[f"{name}/core_b"].reshape(ranks_b),
            cores=cut(z[f"{name}/cores"], [(rk[k], shape[k], rk[k + 1]) for k in range(len(shape))]),
            cp=cut(z[f"{name}/cp"], [(n, m["cp_rank"]) for n in shape]),
            idx=z[f"{name}/indices"], entries=z[f"{name}/entries"], gather=z[f"{name}/gather"],
            **{k: float(v) for k, v in zip(keys, z[f"{name}/scalars"])}))
    return cases
