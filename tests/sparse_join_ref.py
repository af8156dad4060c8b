"""Plain NumPy restatement of the sorted-key join of sparse tensors (csrc/sparse_join.hip, plan in csrc/sparse_join_plan.h):
the key, the stable sort, the splitters at the plan's stride, the two searches with their fixed step counts and the last
occurrence winning, the order in which the dot is summed, and a long-double truth of that dot.  Also the cases the CPU
and GPU tests share, and the loader of the fixture recorded from runs of the reference.
"""
import json
import os

import numpy as np

THREADS = 256
QPT = 8                     # queries of a thread in flight: a thread's loop steps by THREADS * QPT
WG_PER_CU = 2
BLOCK_SUMS = 6 + 2          # the butterfly of a wave, the four waves as (w0 + w1) + (w2 + w3)
CLOSE_SUMS = 6 + 2          # the same in the closing sum of the workgroups' totals
CHIP_CUS = 256              # compute units of an MI355X
MAX_N = 2 ** 31 - 1
I64_MAX = 2 ** 63 - 1


def cdiv(a, b):
    return -(-a // b)


def ceil_log2(n):
    s = 0
    while (1 << s) < n:
        s += 1
    return s


def mults(shape):
    """C-order multipliers (Python integers: exact whatever the shape)."""
    out, acc = [], 1
    for n in reversed(shape):
        out.append(acc)
        acc *= int(n)
    return out[::-1], acc


def keys_of(idx, shape):
    """C-order flat index of every column of ``idx`` (d, N) in ``shape``, int64 (the shape has at most 2^63 - 1 entries)."""
    m, total = mults(shape)
    assert total <= I64_MAX
    idx = np.asarray(idx, dtype=np.int64).reshape(len(shape), -1)
    key = np.zeros(idx.shape[1], dtype=np.int64)
    for k in range(len(shape)):
        key += idx[k] * np.int64(m[k])
    return key


def unravel(keys, shape):
    """The inverse: (d, N) int64 indices of flat C-order keys."""
    m, _ = mults(shape)
    rest = np.asarray(keys, dtype=np.int64).copy()
    rows = []
    for k in range(len(shape)):
        rows.append(rest // np.int64(m[k]))
        rest = rest - rows[-1] * np.int64(m[k])
    return np.stack(rows).reshape(len(shape), -1)


def sort_bits(shape):
    total = mults(shape)[1]
    bits = 1
    while bits < 63 and (1 << bits) < total:
        bits += 1
    return bits


def split(N, max_split):
    """(stride, splitter count) of a table of N nonzeros."""
    stride = cdiv(N, max_split) if N else 1
    return stride, cdiv(N, stride)


def layout(N_table, Nq, max_split, n_cu=CHIP_CUS):
    stride, n_split = split(N_table, max_split)
    grid = min(cdiv(Nq, THREADS), WG_PER_CU * max(n_cu, 1))
    run = cdiv(Nq, grid) if grid else 0
    return dict(max_split=max_split, stride=stride, n_split=n_split, lds_steps=ceil_log2(n_split), seg_steps=ceil_log2(stride),
                grid=grid, run=run, depth=cdiv(run, THREADS) + BLOCK_SUMS + cdiv(grid, 256) + CLOSE_SUMS)


def build_index(idx, val, shape, max_split):
    """dict(keys, vals, splitters, stride): the nonzeros sorted stably by key, every stride-th sorted key."""
    key = keys_of(idx, shape)
    perm = np.argsort(key, kind="stable")
    ks = key[perm]
    stride, n_split = split(len(ks), max_split)
    spl = ks[::stride]
    assert len(spl) == n_split
    return dict(keys=ks, vals=np.asarray(val, dtype=np.float64)[perm], splitters=spl, stride=stride)


def search(index, qkeys):
    """Position of the LAST sorted key <= each query (0 if there is none) by the two searches of the kernel: a fixed number
    of halvings over the splitters, then over the one segment of at most ``stride`` keys the splitter opens."""
    ks, spl, stride = index["keys"], index["splitters"], index["stride"]
    N, q = len(ks), np.asarray(qkeys, dtype=np.int64)
    base = np.zeros(len(q), dtype=np.int64)
    length = len(spl)
    for _ in range(ceil_log2(len(spl))):
        half = length >> 1
        base += np.where(spl[base + half] <= q, half, 0)
        length -= half
    assert length == 1
    pos = base * stride
    glen = np.minimum(N - pos, stride)
    assert (glen >= 1).all()
    for _ in range(ceil_log2(stride)):
        half = glen >> 1
        pos += np.where(ks[pos + half] <= q, half, 0)
        glen -= half
    assert (glen == 1).all()
    return pos


def join(index, qkeys):
    """out[q]: the entry of the last nonzero of the table with the key of query q, 0.0 if there is none."""
    q = np.asarray(qkeys, dtype=np.int64)
    if len(index["keys"]) == 0:
        return np.zeros(len(q))
    pos = search(index, q)
    return np.where(index["keys"][pos] == q, index["vals"][pos], 0.0)


def _block_total(x):
    """block_total of csrc/wave.h over the 256 threads (last axis): the xor butterfly 32 .. 1 inside each wave, then
    (w0 + w1) + (w2 + w3)."""
    x = x.reshape(x.shape[:-1] + (4, 64)).copy()
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lanes ^ o]
    w = x[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def dot_ordered(qval, tval, n_cu=CHIP_CUS):
    """sum_q qval[q] tval[q] in float64 in the order the plan states: workgroup g owns the run g run .. of queries, thread t
    adds lo + t, lo + t + 256, ... in that order, block_total, then the closing sum of the totals (thread t adds the
    totals t, t + 256, ..., block_total)."""
    qval, tval = np.asarray(qval, dtype=np.float64), np.asarray(tval, dtype=np.float64)
    lay = layout(0, len(qval), 1, n_cu)
    grid, run = lay["grid"], lay["run"]
    if grid == 0:
        return 0.0
    per = cdiv(run, THREADS)
    prod = np.zeros((grid, per * THREADS))
    for g in range(grid):
        seg = (qval[g * run:(g + 1) * run] * tval[g * run:(g + 1) * run])
        prod[g, :len(seg)] = seg
    acc = np.zeros((grid, THREADS))
    for j in range(per):
        acc = acc + prod[:, j * THREADS:(j + 1) * THREADS]
    part = _block_total(acc)
    rounds = cdiv(grid, 256)
    padded = np.zeros(rounds * 256)
    padded[:grid] = part
    close = np.zeros(256)
    for j in range(rounds):
        close = close + padded[j * 256:(j + 1) * 256]
    return float(_block_total(close))


def dot_truth(qval, tval):
    """(sum qval tval, sum |qval tval|) in np.longdouble."""
    p = np.asarray(qval, dtype=np.longdouble) * np.asarray(tval, dtype=np.longdouble)
    return p.sum(), float(np.abs(p).sum())


def bound(depth, abs_sum):
    """|dot - truth| <= (1 + D) 2^-53 sum |terms|: one rounding of the product (none with an fma) and at most D additions
    on the way of any term, each with relative error 2^-53 (first order; the (1 + u)^D - 1 excess is below D^2 2^-106)."""
    return (1 + depth) * 2.0 ** -53 * abs_sum * (1 + 1e-9)


# ---- the cases the CPU and GPU tests share ---------------------------------------------------------------------------------
BIG_SHAPE = (2 ** 31, 2 ** 31 - 1, 2)        # 2^63 - 2^32 entries: keys use all 63 bits


SIZE_NAMES = ["n0", "n1", "n2", "ms-1", "ms", "ms+1", "2ms+1", "12ms+7"]


def table_sizes(max_split):
    return [0, 1, 2, max_split - 1, max_split, max_split + 1, 2 * max_split + 1, 12 * max_split + 7]


def make_table(rng, shape, N, kind="random"):
    """(idx (d, N), val (N,)) of a table in shuffled storage order.  kind: 'random' (distinct keys), 'all_equal', 'run'
    (a run of equal keys over positions 1 .. 7 of the sorted order: across the splitters of any stride up to 6),
    'near_top' (keys around 2^62 and at the very top of BIG_SHAPE)."""
    total = mults(shape)[1]
    if kind == "all_equal":
        keys = np.full(N, total // 3, dtype=np.int64)
    elif kind == "near_top":
        lo = rng.integers(2 ** 62 - 10 ** 6, 2 ** 62 + 10 ** 6, N // 2, dtype=np.int64)
        hi = total - 1 - rng.integers(0, 10 ** 6, N - N // 2, dtype=np.int64)
        keys = np.concatenate([lo, hi])
    else:
        # distinct keys with gaps: every third number of a random subset, so that key - 1 and key + 1 are absent
        keys = np.sort(rng.choice(max((total - 2) // 3, N), size=N, replace=False).astype(np.int64)) * 3 + 1 if N else np.zeros(0, dtype=np.int64)
        keys = np.minimum(keys, total - 1)
        if kind == "run" and N >= 9:
            keys[1:8] = keys[1]
    keys = keys[rng.permutation(N)]
    return unravel(keys, shape), rng.standard_normal(N)


def make_queries(rng, shape, index, Nq):
    """Nq query keys against a table: below the first and above the last key, the first and the last, splitters and their
    two neighbours, absent keys between neighbouring ones, hits, misses and repeats; in shuffled order."""
    total = mults(shape)[1]
    ks, spl = index["keys"], index["splitters"]
    special = [0, total - 1]
    if len(ks):
        special += [ks[0] - 1, ks[0], ks[0] + 1, ks[-1] - 1, ks[-1], ks[-1] + 1]
        for s in np.unique(np.concatenate([spl[:3], spl[-3:], spl[len(spl) // 2:len(spl) // 2 + 1]])):
            special += [s - 1, s, s + 1]
        mid = ks[len(ks) // 2]
        special += [mid, mid + 1]
    special = np.array([k for k in special if 0 <= k < total], dtype=np.int64)
    n_hit = (Nq - len(special)) // 2 if len(ks) else 0
    hits = ks[rng.integers(0, len(ks), max(n_hit, 0))] if len(ks) else np.zeros(0, dtype=np.int64)
    rest = max(Nq - len(special) - len(hits), 0)
    misses = rng.integers(0, total, rest, dtype=np.int64)
    q = np.concatenate([special, hits, misses])
    if len(q) > 4:
        q[-2:] = q[:2]                               # repeated queries
    q = q[rng.permutation(len(q))][:Nq]
    if len(q) < Nq:
        q = np.concatenate([q, rng.integers(0, total, Nq - len(q), dtype=np.int64)])
    return unravel(q, shape), rng.standard_normal(Nq)


def case_list(max_split):
    """(name, shape, table size, table kind, Nq): seeded by the name, the same on every run."""
    mid = (97, 89, 83)
    out = [(name, mid, N, "random", 700) for name, N in zip(SIZE_NAMES, table_sizes(max_split))]
    out += [("run_over_splitters", mid, 2 * max_split + 1, "run", 500),
            ("all_equal", mid, max_split + 1, "all_equal", 300),
            ("d1", (50000,), 3000, "random", 1000),
            ("d5_unit_modes", (1, 300, 1, 1, 200), 2000, "random", 1000),
            ("big_shape", BIG_SHAPE, 4000, "near_top", 1500)]
    out += [(f"nq{nq}", mid, 1000, "random", nq) for nq in (0, 1, 255, 256, 257)]
    # beyond what the grid cap takes in one step of the threads' loops: the loop over the queries runs twice
    out.append(("nq_beyond_grid", mid, 5000, "random", WG_PER_CU * CHIP_CUS * THREADS * QPT + 5000))
    return out


def make_case(spec):
    name, shape, N, kind, Nq = spec
    rng = np.random.default_rng(sum(map(ord, name)) + 7 * N + Nq)
    tidx, tval = make_table(rng, shape, N, kind)
    return dict(name=name, shape=shape, tidx=tidx, tval=tval, kind=kind, Nq=Nq, rng=rng)


def case_queries(case, index):
    return make_queries(case["rng"], case["shape"], index, case["Nq"])


# ---- the fixture recorded from the reference ------------------------------------------------------------------------------
def load_cases():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sparse_join_cases.npz")
    with np.load(path) as z:
        meta = json.loads(str(z["meta"]))
        out = []
        for name, m in meta.items():
            c = dict(name=name, shape=tuple(m["shape"]), dup_a=m["dup_a"], dup_b=m["dup_b"])
            for k in ("idx_a", "val_a", "idx_b", "val_b", "gather_idx", "gather_b", "dense", "scalars"):
                c[k] = z[f"{name}/{k}"]
            c.update(dict(zip(("dot_ab", "dot_ba", "dot_abT", "dot_a_dense", "dot_dense_a", "dot_aT_denseT"), c["scalars"])))
            out.append(c)
    return out
