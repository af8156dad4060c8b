"""The lazy-Gaussian products on the device (csrc/gauss_lazy.hip) and ``LazyGaussianDRM`` at the API.

Both entry points are D[m, n] = sum_k G[lo + m, k] X[k, n] with G the rows [lo, lo + w) of the matrix ``random_normal_dev`` stores
for the seed (tests/gauss_lazy_cases.py: the table of calls, each tagged with its plan branch).

* Samples, bit for bit: X holds a single 1 per column, so every output is one sample plus exact zeros and must have the bits
  of the stored matrix's entry.
* Products: Gaussian X; every entry within (K + 2) 2^-53 sum |g| |x| of the long-double product with the stored matrix (K
  roundings of the sum in any order, one per product formed, one for the stored reference's own rounding to a double), and the same
  bits on a second call.
* Operands and outputs have leading dimensions beyond their extents; the operand's padding holds 1e300, the output lies
  between guard bands (tests/edge_kit.py).
* Whole sketches with ``LazyGaussianDRM`` against the same call with ``DenseGaussianDRM`` of the same seed."""
import numpy as np
import pytest

from tests import gauss_lazy_cases as glc
from tests.edge_kit import LD, PAD, assert_guards, bounded, rel_fro, same_bits, sentinel_buffer, strided, tsa  # noqa: F401

pytestmark = pytest.mark.gpu

GUARD = 64
_stored = {}          # K -> the stored matrix (TRUE_ROWS, K) of the table's seed, on the host: computed once, never written


def stored_matrix(K):
    if K not in _stored:
        from tt_sketch_amd.utils import random_normal_dev
        G = random_normal_dev((glc.TRUE_ROWS, K), seed=glc.SEED).get()
        G.setflags(write=False)
        _stored[K] = G
    return _stored[K]


def _dev(a):
    from tt_sketch_amd.device import DevArray
    return DevArray.from_host(np.ascontiguousarray(a))


def run_case(c, X, pad_x=3, pad_d=5):
    """the entry point of case c on the (K, N) operand X -> D (w, N) as the host sees it"""
    from tt_sketch_amd import _native as nat
    left = c.side == "left"
    op = X if left else X.T                               # as it lies in memory: Xu (K, N), or S (N, K)
    R, C = op.shape
    ldx = C + pad_x
    xbuf = np.full((R - 1) * ldx + C + pad_x, PAD)
    strided(xbuf, 0, (R, C), (ldx, 1))[...] = op
    Ro, Co = (c.w, c.N) if left else (c.N, c.w)
    ldd = Co + pad_d
    n_out = (Ro - 1) * ldd + Co
    dbuf = _dev(sentinel_buffer(n_out, GUARD, GUARD))
    entry = "ttsk_gauss_lazy_left" if left else "ttsk_gauss_lazy_right"
    nat.call(entry, glc.SEED, c.lo, c.lo + c.w, c.K, _dev(xbuf), c.N, ldx, dbuf[GUARD:], ldd, 0)
    host = dbuf.get()
    assert_guards(host, [(GUARD, (Ro, Co), (ldd, 1))], (entry, c))
    out = strided(host, GUARD, (Ro, Co), (ldd, 1)).copy()
    return out if left else out.T


def selection(c):
    """X (K, N) with a single 1 per column, at row p[n]; the first and last rows of G's columns are both hit"""
    p = (5 * np.arange(c.N) + 2) % c.K
    p[0], p[-1] = 0, c.K - 1
    X = np.zeros((c.K, c.N))
    X[p, np.arange(c.N)] = 1.0
    return X, p


def _by_width(side):
    groups = {}
    for c in glc.cases(side):
        groups.setdefault(c.w, []).append(c)
    return [pytest.param(side, w, id="%s-w%d" % (side, w)) for w in sorted(groups)], groups


_PARAMS, _GROUPS = [], {}
for _side in ("left", "right"):
    _p, _g = _by_width(_side)
    _PARAMS += _p
    _GROUPS[_side] = _g


@pytest.mark.parametrize("side,w", _PARAMS)
def test_samples_bit_for_bit(tsa, side, w):
    for c in _GROUPS[side][w]:
        X, p = selection(c)
        D = run_case(c, X)
        want = stored_matrix(c.K)[c.lo:c.lo + c.w][:, p]
        same_bits(D, np.ascontiguousarray(want), ("samples", c))


@pytest.mark.parametrize("side,w", _PARAMS)
def test_products_under_the_derived_bound(tsa, side, w):
    if np.finfo(LD).eps >= np.finfo(np.float64).eps:
        pytest.skip("long double is no wider than double here")
    rng = np.random.default_rng(1000 * w + (side == "right"))
    worst = 0.0
    for c in _GROUPS[side][w]:
        X = rng.standard_normal((c.K, c.N))
        G = stored_matrix(c.K)[c.lo:c.lo + c.w]
        ref = G.astype(LD) @ X.astype(LD)
        hi = ref.astype(np.float64)
        lo = (ref - hi).astype(np.float64)
        tol = (c.K + 2) * 2.0 ** -53 * (np.abs(G) @ np.abs(X))
        D = run_case(c, X)
        worst = max(worst, bounded(D, hi, lo, tol, ("product", c), np.inf))
        same_bits(D, run_case(c, X), ("a second call", c))
    print("%s w = %d: largest |err| / bound %.3f" % (side, w, worst))


def test_entry_refusals_write_nothing(tsa):
    from tt_sketch_amd import _native as nat
    x = _dev(np.ones(70 * 70))
    for entry in ("ttsk_gauss_lazy_left", "ttsk_gauss_lazy_right"):
        for args, exc in (((glc.SEED, 0, 65, 8, x, 8, 8), nat.TtskUnsupported), ((glc.SEED, 2 ** 40, 2 ** 40 + 1, 2 ** 30, x, 8, 2 ** 30), nat.TtskUnsupported),
                          ((glc.SEED, 3, 2, 8, x, 8, 8), ValueError), ((glc.SEED, 0, 4, 8, None, 8, 8), ValueError),
                          ((glc.SEED, 0, 4, 8, x, 8, 7), ValueError)):
            out = _dev(sentinel_buffer(70 * 70, 0, 0))
            with pytest.raises(exc):
                nat.call(entry, *args, out, 70, 0)
            nat.call("ttsk_sync", -1)
            assert (out.get().view(np.uint64) == sentinel_buffer(1, 0, 0).view(np.uint64)[0]).all(), (entry, args)
        nat.call(entry, glc.SEED, 4, 4, 8, None, 8, 8, None, 8, 0)            # no rows of G: nothing to do


# ================================================================== the API
# (4-mode: l = 2, not 3 -- the pseudo-inverse of Omega_2, (r, l), would have the shape of the last right matrix, (r, n_3))
SHAPES = {"4-mode": ((6, 5, 4, 3), 2, 5), "5-mode": ((16, 8, 8, 8, 16), 5, 7), "2-mode": ((9, 7), 4, 5)}


@pytest.fixture(scope="module")
def tensors(tsa):
    """a dense tensor per shape: TT rank 2 plus a perturbation of 1e-3, so that recovery errors are neither zero nor one"""
    out = {}
    for name, (shape, l, r) in SHAPES.items():
        rng = np.random.default_rng(len(shape))
        X = tsa.TensorTrain.random(shape, 2, seed=4).to_numpy()
        X = X / np.linalg.norm(X) + 1e-3 * rng.standard_normal(shape) / np.sqrt(X.size)
        out[name] = (tsa.DenseTensor(X), X, (l,) * (len(shape) - 1), (r,) * (len(shape) - 1))
    return out


def _arrays(stt):
    return [np.asarray(a) for a in list(stt.Psi_cores) + list(stt.Omega_mats)]


def _close(got, want, what, bar=1e-12):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, (what, i, a.shape, b.shape)
        r = rel_fro(a, b)
        print("%s[%d]: %.3e" % (what, i, r))
        assert r <= bar, (what, i, r)


def _matrix_shapes(shape, l, r, lazy_left, lazy_right, formed_rank=None):
    """The (rows, cols) of the matrices the lazy sides stand for, without the shapes a sketch forms anyway.  Sizes alone do
    not tell the two apart -- Omega_mu (l, r) has the elements of a right matrix (r, n) where n = l, a Psi core those of
    another -- so the watch compares shapes; a left product Z_mu (l, n_{mu+1} ... n_{d-1}) can even have the shape of a left
    matrix (l, n_0 ... n_mu) where the tensor's shape is a palindrome, and is taken out.  ``formed_rank``: the rank of the
    left products where it is not l -- an hmt sketch has no left DRM and forms Z_mu with the right ranks, (r, n_{mu+1} ...
    n_{d-1}), which IS the shape of the right matrix of the level: there the shapes tell nothing, and the watch on the fills
    and on ``LazyGaussian.materialise`` is what holds."""
    d = len(shape)
    head = [int(np.prod(shape[:mu + 1])) for mu in range(d - 1)]
    tail = [int(np.prod(shape[mu + 1:])) for mu in range(d - 1)]
    mats = set()
    if lazy_left:
        mats |= {(l[mu], head[mu]) for mu in range(d - 1)}
    if lazy_right:
        mats |= {(r[mu], tail[mu]) for mu in range(d - 1)}
    L = l if formed_rank is None else formed_rank
    return mats - {(L[mu], tail[mu]) for mu in range(d - 1)}


class Watch:
    """while active: every DevArray.empty, every Gaussian fill and every materialisation of a recipe is recorded"""

    def __init__(self, monkeypatch):
        from tt_sketch_amd import _native as nat
        from tt_sketch_amd.device import DevArray
        from tt_sketch_amd.drm import LazyGaussian
        self.shapes, self.fills, self.materialised = [], [], []
        real_empty, real_call, real_mat = DevArray.empty.__func__, nat.call, LazyGaussian.materialise

        def materialise(recipe):
            self.materialised.append(recipe.shape)
            return real_mat(recipe)

        def empty(cls, shape, *a, **kw):
            arr = real_empty(cls, shape, *a, **kw)
            self.shapes.append(tuple(arr.shape))
            return arr

        def call(name, *args):
            if name.startswith("ttsk_fill_normal"):
                self.fills.append(name)
            return real_call(name, *args)
        monkeypatch.setattr(DevArray, "empty", classmethod(empty))
        monkeypatch.setattr(nat, "call", call)
        monkeypatch.setattr(LazyGaussian, "materialise", materialise)
        monkeypatch.setattr(LazyGaussian, "__dev_array__", materialise)

    def check(self, shape, l, r, what, lazy_left=True, lazy_right=True, formed_rank=None):
        assert self.materialised == [], (what, self.materialised)
        mats = _matrix_shapes(shape, l, r, lazy_left, lazy_right, formed_rank)
        bad = [sh for sh in self.shapes if sh in mats]
        assert not bad, "%s: arrays of the shape of a sketching matrix were allocated: %s" % (what, bad)
        assert self.shapes, what                       # (a palindrome shape leaves no left shape to watch: the fills do)


@pytest.mark.parametrize("pairing", ["both", "lazy-left", "lazy-right"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_stream_sketch_equals_the_stored_run(tsa, tensors, monkeypatch, name, pairing):
    T, X, l, r = tensors[name]
    shape = X.shape
    lazy = {"both": (True, True), "lazy-left": (True, False), "lazy-right": (False, True)}[pairing]
    types = lambda mine: tuple(mine if on else tsa.TensorTrainDRM for on in lazy)
    lt, rt = types(tsa.DenseGaussianDRM)
    want = _arrays(tsa.stream_sketch(T, l, r, seed=21, left_drm_type=lt, right_drm_type=rt))
    lt, rt = types(tsa.LazyGaussianDRM)
    watch = Watch(monkeypatch)
    stt = tsa.stream_sketch(T, l, r, seed=21, left_drm_type=lt, right_drm_type=rt)
    got = _arrays(stt)
    monkeypatch.undo()
    assert type(stt.left_drm) is lt and type(stt.right_drm) is rt
    if pairing == "both":
        assert watch.fills == [], watch.fills
    watch.check(shape, stt.left_drm.rank, stt.right_drm.rank[::-1], (name, pairing), *lazy)
    _close(got, want, "stream %s %s" % (name, pairing))


@pytest.mark.parametrize("name", list(SHAPES))
def test_orthogonal_and_hmt_recover_as_the_stored_run(tsa, tensors, monkeypatch, name):
    T, X, l, r = tensors[name]
    calls = {
        "orthogonal": lambda cls: tsa.orthogonal_sketch(T, l, r, seed=5, left_drm_type=cls, right_drm_type=cls, return_drm=True),
        "hmt": lambda cls: tsa.hmt_sketch(T, r, seed=5, drm_type=cls, return_drm=True),
        "orthogonal with a train on the left": lambda cls: tsa.orthogonal_sketch(T, l, r, seed=5, left_drm_type=tsa.TensorTrainDRM,
                                                                                 right_drm_type=cls, return_drm=True),
    }
    for what, run in calls.items():
        stored = rel_fro(run(tsa.DenseGaussianDRM)[0].to_numpy(), X)
        watch = Watch(monkeypatch)
        out, *drms = run(tsa.LazyGaussianDRM)
        got = rel_fro(out.to_numpy(), X)
        monkeypatch.undo()
        right = drms[-1]
        assert type(right) is tsa.LazyGaussianDRM
        assert not [f for f in watch.fills if f == "ttsk_fill_normal"], watch.fills      # (a train fills its cores: _many)
        rr = right.rank[::-1]
        if what == "hmt":
            watch.check(X.shape, rr, rr, (name, what), lazy_left=False, formed_rank=rr)
        else:
            watch.check(X.shape, drms[0].rank, rr, (name, what), lazy_left=type(drms[0]) is tsa.LazyGaussianDRM)
        print("%s %s: error %.3e lazy, %.3e stored" % (name, what, got, stored))
        assert abs(got - stored) <= 1e-10 and got < 0.1, (name, what, got, stored)


def test_blocked_sketch_and_increase_rank(tsa, tensors):
    T, X, _, _ = tensors["4-mode"]
    shape, k = X.shape, 3
    l0, r0, l1, r1 = (2,) * k, (3,) * k, (4,) * k, (6,) * k
    ld, rd = tsa.LazyGaussianDRM(l0, shape, False, seed=31), tsa.LazyGaussianDRM(r0, shape, True, seed=32)
    small = tsa.stream_sketch(T, l0, r0, left_drm=ld, right_drm=rd)
    grown = small.increase_rank(T, l1, r1)
    assert type(grown.left_drm) is tsa.LazyGaussianDRM and grown.left_drm.rank == l1 and grown.right_drm.rank == r1
    ld2, rd2 = ld.increase_rank(l1), rd.increase_rank(r1)
    fresh = _arrays(tsa.stream_sketch(T, l1, r1, left_drm=ld2, right_drm=rd2))
    _close(_arrays(grown), fresh, "increase_rank")
    zeros = (0,) * k
    blk = tsa.blocked_stream_sketch(T, ld2, rd2, [zeros, l0, l1], [zeros, r0, r1])
    _close([np.asarray(a) for a in list(blk.Psi_cores) + list(blk.Omega_mats)], fresh, "blocked")
    stored = _arrays(tsa.stream_sketch(T, l1, r1, left_drm=tsa.DenseGaussianDRM(l1, shape, False, seed=31),
                                       right_drm=tsa.DenseGaussianDRM(r1, shape, True, seed=32)))
    _close(fresh, stored, "one shot against the stored DRMs")


def test_width_65_takes_the_stored_route(tsa, tensors):
    """65 rows are beyond the kernels: the matrix is filled for the one product, and the sketch is the stored run's"""
    T, X, _, _ = tensors["5-mode"]
    k = X.ndim - 1
    l, r = (60,) * k, (65,) * k
    want = _arrays(tsa.stream_sketch(T, l, r, left_drm=tsa.DenseGaussianDRM(l, X.shape, False, seed=7),
                                     right_drm=tsa.DenseGaussianDRM(r, X.shape, True, seed=8)))
    got = _arrays(tsa.stream_sketch(T, l, r, left_drm=tsa.LazyGaussianDRM(l, X.shape, False, seed=7),
                                    right_drm=tsa.LazyGaussianDRM(r, X.shape, True, seed=8)))
    _close(got, want, "w = 65")


def test_other_tensor_kinds_through_the_filled_matrix(tsa):
    shape = (6, 5, 4, 3)
    T = tsa.TensorTrain.random(shape, 2, seed=1)
    a = tsa.stream_sketch(T, (3,) * 3, (5,) * 3, seed=9, left_drm_type=tsa.DenseGaussianDRM, right_drm_type=tsa.DenseGaussianDRM)
    b = tsa.stream_sketch(T, (3,) * 3, (5,) * 3, seed=9, left_drm_type=tsa.LazyGaussianDRM, right_drm_type=tsa.LazyGaussianDRM)
    same_bits(_arrays(a), _arrays(b), "a tensor train with lazy DRMs")
