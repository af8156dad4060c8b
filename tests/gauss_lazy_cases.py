"""The table of calls the tests of the lazy-Gaussian products share (csrc/gauss_lazy.hip, plan in csrc/gauss_lazy_plan.h):
tests/test_gauss_lazy_plan.py holds every case against the plan branch its tag names, tests/test_gpu_gauss_lazy.py runs
every case on the device.  Plain module: no GPU, no tt_sketch_amd.

Both entry points are D[m, n] = sum_k G[lo + m, k] X[k, n] (m < w, k < K, n < N): for `left` K = P and N = Q, for `right`
K = cols and N = rows.  A tag is "<branch><16-row tiles of w>": "direct" is one launch into the product, "split" cuts K into
chunks of a multiple of 256, writes partial products and sums them in a closing launch."""
from collections import namedtuple

Case = namedtuple("Case", "side lo w K N tag")

EDGES = (1, 3, 15, 16, 17, 63, 64, 65)
WIDTHS = (1, 16, 17, 33, 64)
TRUE_ROWS = 5 + 64 + 2                            # rows of the stored matrix every case is a row range of
SEED = (77 << 20) + 0x5A5A0000 + 2                # a seed_mu as DenseGaussianDRM forms it


def _tiles(w):
    return (w + 15) // 16


def cases(side):
    out = []
    for i, w in enumerate(WIDTHS):
        for K in EDGES:
            for N in EDGES:
                lo = 5 if (i + EDGES.index(K) + EDGES.index(N)) % 2 else 0
                out.append(Case(side, lo, w, K, N, "direct%d" % _tiles(w)))
    # beyond one workgroup's columns, and a contracted extent at, one past and well past a chunk boundary
    for w, lo in ((1, 5), (17, 0), (33, 5), (64, 0)):
        t = _tiles(w)
        out += [Case(side, lo, w, 17, 257, "direct%d" % t),           # two column tiles, the second one column wide
                Case(side, lo, w, 256, 3, "direct%d" % t),            # exactly one chunk: not split
                Case(side, lo, w, 257, 3, "split%d" % t),             # one past the chunk boundary: chunks of 256 and 1
                Case(side, lo, w, 513, 300, "split%d" % t),           # three chunks, two column tiles
                Case(side, lo, w, 700, 1, "split%d" % t)]
    return out


ALL = cases("left") + cases("right")
TAGS = sorted({c.tag for c in ALL})
assert TAGS == ["direct%d" % t for t in (1, 2, 3, 4)] + ["split%d" % t for t in (1, 2, 3, 4)]
