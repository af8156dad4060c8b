"""DevArray's views, copy_into's dimension merge and contract's lowering (tt_sketch_amd/device.py) against NumPy, with
nothing of a device: device._Buffer is a NumPy-backed buffer and nat.call goes to Python emulations of ttsk_copy_strided
(the index formula of its header), ttsk_gemm (the GemmDesc formula, five nested loops), ttsk_h2d / d2h / d2d, ttsk_memset
and ttsk_axpby.  Every emulated access is bounds-checked against the buffer it falls in, so a view that leaves its
allocation fails here rather than on a device; fresh buffers hold NaN, so a result that depends on unwritten memory shows.

Operands are small integers: every comparison with NumPy is equality."""
import ctypes
import itertools

import numpy as np
import pytest

import tt_sketch_amd.device as dev
from tt_sketch_amd import _native as nat_mod
from tt_sketch_amd.device import DevArray, axpby, contract, copy_into


# ------------------------------------------------------------------------------------------------ the emulated library
class Memory:
    """the live buffers and the recorded calls of one test"""

    def __init__(self):
        self.buffers, self.calls = [], []

    def locate(self, addr, nbytes):
        """-> (the uint8 array of the buffer that holds [addr, addr + nbytes), the byte offset in it)"""
        for base, mem in self.buffers:
            if base <= addr and addr + nbytes <= base + mem.size:
                return mem, addr - base
        raise AssertionError("access of %d bytes at %#x is inside no buffer" % (nbytes, addr))

    def doubles(self, addr, shape, strides):
        """the float64 view of a strided array at addr, element strides; checked against its buffer"""
        assert all(s >= 0 for s in strides) and addr % 8 == 0
        span = 1 + sum((n - 1) * s for n, s in zip(shape, strides))
        mem, off = self.locate(addr, 8 * span)
        return np.lib.stride_tricks.as_strided(mem[off:off + 8 * span].view(np.float64), shape=tuple(shape), strides=tuple(8 * s for s in strides))

    def names(self, *only):
        return [c[0] for c in self.calls if not only or c[0] in only]


def addr_of(x):
    if x is None:
        return 0
    if isinstance(x, DevArray):
        return x.ptr
    if isinstance(x, ctypes.c_void_p):
        return x.value or 0
    return int(x)


def emulate(mem, name, *args):
    mem.calls.append((name, args))
    if name in ("ttsk_h2d", "ttsk_d2h", "ttsk_d2d"):
        dst, src, nbytes = addr_of(args[0]), addr_of(args[1]), int(args[2])
        assert nbytes > 0, "%s of nothing" % name
        if name != "ttsk_h2d":
            mem.locate(src, nbytes)
        if name != "ttsk_d2h":
            mem.locate(dst, nbytes)
        ctypes.memmove(dst, src, nbytes)
    elif name == "ttsk_memset":
        buf, off = mem.locate(addr_of(args[0]), int(args[2]))
        buf[off:off + int(args[2])] = int(args[1])
    elif name == "ttsk_copy_strided":
        dst, src, nd = addr_of(args[0]), addr_of(args[1]), int(args[2])
        assert 0 <= nd <= 5
        shape, ds, ss = (list(a)[:nd] for a in args[3:6])
        assert all(n >= 1 for n in shape), "an empty copy reached the library"
        s = mem.doubles(src, shape, ss).copy()
        d = mem.doubles(dst, shape, ds)
        d[...] = s                                               # dst[i0..i4] = src[i0..i4], the strides in the two views
    elif name == "ttsk_gemm":
        g = args[0]._obj
        A, B, C, ks = (addr_of(a) for a in args[1:5])
        assert min(g.batch, g.M, g.N) >= 1 and min(g.Ko, g.Ki) >= 0
        a = mem.doubles(A, (g.batch, g.M, g.Ko, g.Ki), (g.a_b, g.a_m, g.a_ko, g.a_ki)) if g.Ko * g.Ki else None
        b = mem.doubles(B, (g.batch, g.Ko, g.Ki, g.N), (g.b_b, g.b_ko, g.b_ki, g.b_n)) if g.Ko * g.Ki else None
        c = mem.doubles(C, (g.batch, g.M, g.N), (g.c_b, g.c_m, g.c_n))
        scale = mem.doubles(ks, (g.Ko * g.Ki,), (1,)) if ks else None
        out = np.zeros((g.batch, g.M, g.N))
        for ib in range(g.batch):
            for m in range(g.M):
                for n in range(g.N):
                    acc = 0.0
                    for ko in range(g.Ko):
                        for ki in range(g.Ki):
                            acc += a[ib, m, ko, ki] * (scale[ko * g.Ki + ki] if scale is not None else 1.0) * b[ib, ko, ki, n]
                    out[ib, m, n] = g.alpha * acc + (c[ib, m, n] if g.accumulate else 0.0)
        c[...] = out
    elif name == "ttsk_axpby":
        n = int(args[4])
        y, x = mem.doubles(addr_of(args[0]), (n,), (1,)), mem.doubles(addr_of(args[1]), (n,), (1,))
        y[...] = args[2] * x + (0.0 if args[3] == 0 else args[3] * y)
    else:
        raise AssertionError("unexpected call of %s" % name)


@pytest.fixture
def mem(monkeypatch):
    m = Memory()

    class Buffer:
        """what device._Buffer is to DevArray: ptr and nbytes; the memory is NumPy's, filled with 0xff (NaN as doubles)"""

        def __init__(self, nbytes, stream=0):
            self.nbytes = int(nbytes)
            self.mem = np.full(max(self.nbytes, 8) + 8, 0xFF, dtype=np.uint8)
            self.ptr = self.mem.ctypes.data
            m.buffers.append((self.ptr, self.mem))
            assert self.ptr % 8 == 0

    monkeypatch.setattr(dev, "_Buffer", Buffer)
    monkeypatch.setattr(nat_mod, "call", lambda name, *args: emulate(m, name, *args))
    return m


def ints(shape, seed=0):
    return np.random.default_rng(seed).integers(-3, 4, size=shape).astype(np.float64)


def counting(shape):
    return np.arange(1.0, 1.0 + int(np.prod(shape))).reshape(shape)


# ------------------------------------------------------------------------------------------------ __getitem__
KEYS = (1, -1, 7, slice(None), slice(1, 3), slice(2, 2), slice(3, 1), slice(-2, None), None, Ellipsis, slice(2, 9), slice(-9, 2))
GETITEM_SHAPES = ((4, 5, 6), (1, 5, 3), (3, 1, 4), (0, 3), (5,))


def outcome(f):
    """("ok", the array) or ("raise", the exception's type)"""
    try:
        return "ok", f()
    except Exception as e:          # noqa: BLE001 -- the type is what is compared
        return "raise", type(e)


@pytest.mark.parametrize("shape", GETITEM_SHAPES, ids=str)
def test_getitem_is_numpys(mem, shape):
    h = counting(shape)
    a = DevArray.from_host(h)
    keys = [(k,) for k in KEYS] + list(itertools.product(KEYS, repeat=2)) + [(1, None, slice(1, 3)), (Ellipsis, None, -1), (slice(None), Ellipsis, 0, None)]
    seen = {"ok": 0, "raise": 0}
    for key in keys:
        want = outcome(lambda: h[key])
        got = outcome(lambda: a[key])
        assert got[0] == want[0], (shape, key, got, want)
        if want[0] == "raise":
            assert got[1] is want[1] is IndexError, (shape, key, got, want)
        else:
            v, w = got[1], want[1]
            assert v.shape == w.shape and v.buf is a.buf, (shape, key, v.shape, w.shape)
            assert np.array_equal(v.get(), w), (shape, key)
        seen[want[0]] += 1
        one = outcome(lambda: a[key[0]])
        assert one[0] == outcome(lambda: h[key[0]])[0], (shape, key[0])
    assert seen["ok"] >= 30 and seen["raise"] >= 4, seen


def test_getitem_refuses_steps(mem):
    a = DevArray.from_host(counting((4, 5)))
    for key in (slice(None, None, 2), slice(None, None, -1), (0, slice(1, 4, 3))):
        with pytest.raises(IndexError, match="unit-step"):
            a[key]
    assert np.array_equal(a[::1, 1:4:1].get(), counting((4, 5))[:, 1:4])


# ------------------------------------------------------------------------------------------------ reshape
def bases(h):
    """[(name, view of h)] for a 3-d h: what the sketch path reshapes"""
    return [("contiguous", lambda x: x), ("row-sliced", lambda x: x[1:3]), ("column-sliced", lambda x: x[:, :, 1:3]),
            ("middle-sliced", lambda x: x[:, 1:3]), ("transposed", lambda x: x.T), ("swapped", lambda x: x.transpose(1, 0, 2)),
            ("indexed", lambda x: x[:, 1]), ("none-inserted", lambda x: x[:, None]), ("none-sliced", lambda x: x[None, 1:, :, 0]),
            ("unit-sliced", lambda x: x[1:2, :, 2:3])]


def targets(size):
    """shapes of `size` elements: the ordered factorisations into up to three factors, unit extents in every place, -1 in each"""
    fact = {(size,)}
    for p in range(1, size + 1):
        if size % p == 0:
            fact.add((p, size // p))
            for q in range(1, size // p + 1):
                if (size // p) % q == 0:
                    fact.add((p, q, size // p // q))
    out = set(fact)
    for t in fact:
        for i in range(len(t) + 1):
            out.add(t[:i] + (1,) + t[i:])
        for i in range(len(t)):
            out.add(t[:i] + (-1,) + t[i + 1:])
    return sorted(out)


def test_reshape_views_where_numpy_views(mem):
    h = counting((4, 3, 4))
    a = DevArray.from_host(h)
    viewed = copied = 0
    for name, f in bases(h):
        v, w = f(a), f(h)
        assert v.shape == w.shape, name
        for t in targets(w.size):
            want = w.reshape(t)
            st = dev._view_strides(v.shape, v.strides, want.shape)
            if np.shares_memory(want, h):                     # NumPy needed no copy: neither may DevArray
                assert st is not None, (name, v.shape, v.strides, t)
            del mem.calls[:]
            got = v.reshape(*t) if len(t) % 2 else v.reshape(t)      # both call forms
            first = mem.names()[:1]
            assert got.shape == want.shape and np.array_equal(got.get(), want), (name, t)
            if st is not None:
                assert got.buf is a.buf and got.strides == tuple(st) and got.offset == v.offset and first == [], (name, t)
                assert np.array_equal(DevArray(a.buf, v.offset, want.shape, st).get(), want), (name, t)
                viewed += 1
            else:
                assert got.buf is not a.buf and got.is_contiguous() and first == ["ttsk_copy_strided"], (name, t)
                copied += 1
    assert viewed >= 100 and copied >= 50, (viewed, copied)


def test_reshape_sizes_must_agree_and_size_zero(mem):
    a = DevArray.from_host(counting((4, 6)))
    for bad in ((5, 5), (4, 7), (-1, 5), (0,)):
        with pytest.raises(ValueError, match="cannot reshape"):
            a.reshape(bad)
    z = DevArray.from_host(np.empty((0, 3)))
    del mem.calls[:]
    assert z.reshape(3, 0).shape == (3, 0) and z.reshape(-1, 3).shape == (0, 3) and z.reshape(0).shape == (0,) and z.T.reshape(-1).shape == (0,)
    assert z.reshape(5, 0, -1).shape == (5, 0, 0) and z.reshape(0, -1).size == 0          # -1 beside a zero: 0 (NumPy refuses; nothing to address either way)
    with pytest.raises(ValueError, match="cannot reshape"):
        z.reshape(1, 3)
    assert a[:, 2:2].reshape(2, 0, 2).shape == (2, 0, 2)
    assert mem.calls == []


# ------------------------------------------------------------------------------------------------ transpose, T, is_contiguous
@pytest.mark.parametrize("shape", ((2, 3, 4), (1, 3, 4), (3, 1, 4), (3, 4, 1), (1, 1, 5), (2, 0, 3), (4,), (1,), (3, 5)), ids=str)
def test_transpose_and_is_contiguous(mem, shape):
    h = counting(shape)
    a = DevArray.from_host(h)
    assert a.is_contiguous() and a.T.shape == h.T.shape and np.array_equal(a.T.get(), h.T) and len(a) == shape[0]
    for perm in itertools.permutations(range(len(shape))):
        for v in (a.transpose(*perm), a.transpose(perm), a.transpose(list(perm))):
            w = h.transpose(perm)
            assert v.buf is a.buf and v.shape == w.shape and (v.strides == tuple(s // 8 for s in w.strides) or not w.size)
            assert np.array_equal(v.get(), w)
            if w.size:                                       # (NumPy calls every empty array contiguous; none is ever copied here)
                assert v.is_contiguous() == w.flags.c_contiguous, (shape, perm)
    assert a.transpose().shape == h.T.shape
    if len(shape) == 3 and h.size:
        for key in ((slice(1, None),), (slice(None), slice(0, 1)), (Ellipsis, slice(0, 3)), (0,), (slice(None), None)):
            assert a[key].is_contiguous() == h[key].flags.c_contiguous, (shape, key)


# ------------------------------------------------------------------------------------------------ copy_into and friends
def fewest_dims(dims):
    """brute force: the fewest groups of neighbouring (extent, dst stride, src stride) dimensions, each group one run in both"""
    dims = [d for d in dims if d[0] != 1]
    k = len(dims)
    if k == 0:
        return 0
    joins = [dims[i][1] == dims[i + 1][1] * dims[i + 1][0] and dims[i][2] == dims[i + 1][2] * dims[i + 1][0] for i in range(k - 1)]
    best = k
    for cut in itertools.product((0, 1), repeat=k - 1):          # 0: joined to its successor
        if all(joins[i] for i in range(k - 1) if not cut[i]):
            best = min(best, 1 + sum(cut))
    return best


def views5(h):
    """views of a 5-d h, from one run to five non-mergeable dimensions"""
    return [("whole", lambda x: x), ("reversed", lambda x: x.transpose(4, 3, 2, 1, 0)), ("rotated", lambda x: x.transpose(1, 2, 3, 4, 0)),
            ("pairs", lambda x: x.transpose(2, 3, 4, 0, 1)), ("inner-slice", lambda x: x[..., 1:3]), ("outer-slice", lambda x: x[1:]),
            ("middle-slice", lambda x: x[:, :, 1:2]), ("all-sliced", lambda x: x[:1, 1:, :2, 1:, :3].transpose(1, 0, 3, 2, 4)),
            ("indexed", lambda x: x[:, 1, :, 0]), ("with-none", lambda x: x[:, None, 1, ..., None, 2]), ("swap-last", lambda x: x.transpose(0, 1, 2, 4, 3))]


def test_copy_into_merges_to_the_fewest_dimensions(mem):
    h = counting((2, 3, 2, 3, 4))
    a = DevArray.from_host(h)
    seen = set()
    for name, f in views5(h):
        v, w = f(a), f(h)
        for where in ("contiguous", "slice", "transposed"):
            if where == "contiguous":
                big = np.full(w.shape, -7.0)
                dview, hview = (lambda d: d), (lambda x: x)
            elif where == "slice":                           # a block of a larger array, every extent padded
                big = np.full(tuple(n + 2 for n in w.shape), -7.0)
                key = tuple(slice(1, n + 1) for n in w.shape)
                dview, hview = (lambda d: d[key]), (lambda x: x[key])
            else:
                big = np.full(w.shape[::-1], -7.0)
                dview, hview = (lambda d: d.T), (lambda x: x.T)
            d = DevArray.from_host(big)
            want = big.copy()
            hview(want)[...] = w
            del mem.calls[:]
            copy_into(dview(d), v)
            assert mem.names() == ["ttsk_copy_strided"], (name, where)
            args = mem.calls[0][1]
            dd = dview(d)
            assert args[2] == fewest_dims(list(zip(v.shape, dd.strides, v.strides))) == len(args[3]), (name, where, args[2])
            assert int(np.prod(list(args[3]))) == w.size
            seen.add(args[2])
            assert np.array_equal(d.get(), want), (name, where)            # the view written, the rest unchanged
        for how, got in (("get", v.get()), ("copy", v.copy().get()), ("contiguous", v.contiguous().get()), ("asarray", np.asarray(v)), ("float32", np.asarray(v, dtype=np.float32))):
            assert np.array_equal(got, w), (name, how)
        assert v.copy().buf is not a.buf and v.copy().is_contiguous()
        assert (v.contiguous() is v) == v.is_contiguous()
    assert seen == {1, 2, 3, 4, 5}, seen


def test_copy_into_limits_and_empty(mem):
    h = counting((2,) * 6)
    a = DevArray.from_host(h)
    with pytest.raises(ValueError, match="copy_into supports at most 5 non-mergeable dimensions"):
        a.transpose(5, 4, 3, 2, 1, 0).contiguous()
    assert np.array_equal(a.transpose(1, 0, 3, 2, 4, 5).get(), h.transpose(1, 0, 3, 2, 4, 5))      # six dimensions, five runs
    with pytest.raises(ValueError, match="copy_into: shape"):
        copy_into(DevArray.empty((3, 2)), DevArray.empty((2, 3)))
    del mem.calls[:]
    z = DevArray.from_host(np.empty((3, 0, 2)))
    copy_into(DevArray.empty((2, 0, 3)), z.T)
    assert z.T.copy().shape == (2, 0, 3) and z.T.contiguous().shape == (2, 0, 3) and z.T.get().shape == (2, 0, 3) and z.copy().shape == (3, 0, 2)
    assert DevArray.zeros((0, 4)).fill_zero().get().shape == (0, 4)
    assert mem.calls == []
    i = DevArray.from_host(np.arange(12).reshape(3, 4))
    assert i.dtype == np.int64 and np.array_equal(i.copy().get(), np.arange(12).reshape(3, 4)) and mem.names() == ["ttsk_h2d", "ttsk_d2d", "ttsk_d2h"]
    with pytest.raises(ValueError, match="strided copies are implemented for fp64 only"):
        i.T.contiguous()
    with pytest.raises(ValueError, match="fp64 only"):
        i[:, 1:3].get()
    with pytest.raises(ValueError, match="fill_zero needs a contiguous array"):
        a.T.fill_zero()
    assert not DevArray.zeros((2, 3)).get().any() and not DevArray.from_host(h).fill_zero().get().any()


# ------------------------------------------------------------------------------------------------ contract: the fuzz
def permuted_view(rng, shape):
    """(DevArray, ndarray) of `shape`, stored in a random axis order"""
    order = rng.permutation(len(shape))
    stored = rng.integers(-3, 4, size=[shape[i] for i in order]).astype(np.float64)
    back = np.argsort(order)
    return DevArray.from_host(stored).transpose(*back) if len(shape) else DevArray.from_host(stored), stored.transpose(back)


def random_spec(rng):
    """letters a.. each in one group: M (A and out), N (B and out), batch (all three), K (A and B); every order random"""
    while True:
        letters = "abcde"[:rng.integers(1, 6)]
        group = {c: "MNBK"[rng.integers(0, 4)] for c in letters}
        ia = [c for c in letters if group[c] in "MBK"]
        ib = [c for c in letters if group[c] in "NBK"]
        co = [c for c in letters if group[c] in "MNB"]
        if ia and ib:
            break
    for lst in (ia, ib, co):
        rng.shuffle(lst)
    size = {c: int(rng.integers(1, 5)) for c in letters}
    return "".join(ia), "".join(ib), "".join(co), size


def test_contract_fuzz_equals_einsum_or_is_refused(mem):
    rng = np.random.default_rng(20240521)
    total, refused, copies, routes = 1200, 0, 0, set()
    for it in range(total):
        del mem.buffers[:]                                       # (the operands of the specs before are gone)
        ia, ib, co, size = random_spec(rng)
        spec = "%s,%s->%s" % (ia, ib, co)
        (A, hA), (B, hB) = (permuted_view(rng, [size[c] for c in idx]) for idx in (ia, ib))
        want = np.einsum(spec, hA, hB)
        del mem.calls[:]
        try:
            got = contract(spec, A, B)
        except ValueError as e:
            assert "cannot be lowered onto the strided GEMM" in str(e), (spec, size, str(e))
            refused += 1
            continue
        assert got.shape == want.shape and np.array_equal(got.get(), want), (spec, size, A.strides, B.strides)
        n = mem.names("ttsk_copy_strided", "ttsk_gemm")
        assert n[-1:] == ["ttsk_gemm"] and n.count("ttsk_gemm") == 1 and len(n) <= 3, (spec, n)
        copies += len(n) - 1
        routes.add(len(n))
        assert np.array_equal(A.get(), hA) and np.array_equal(B.get(), hB)
    print("contract fuzz: %d specs, %d refused, %d operand copies" % (total, refused, copies))
    assert total >= 1000 and refused <= total // 10, refused
    assert routes == {1, 2, 3}


# ------------------------------------------------------------------------------------------------ contract: named cases
def run_contract(mem, spec, hA, hB, **kw):
    """-> (result on the host, the gemm's descriptor or None, the names of the copies and gemms)"""
    A, B = DevArray.from_host(hA), DevArray.from_host(hB)
    del mem.calls[:]
    got = contract(spec, A, B, **kw)
    g = [c[1][0]._obj for c in mem.calls if c[0] == "ttsk_gemm"]
    return got.get(), (g[0] if g else None), mem.names("ttsk_copy_strided", "ttsk_gemm", "ttsk_memset")


def test_contract_batch_letter_and_two_level_k(mem):
    hA, hB = ints((3, 4), 1), ints((4, 2), 2)
    got, g, names = run_contract(mem, "kj,jm->jkm", hA, hB)
    assert names == ["ttsk_gemm"] and np.array_equal(got, np.einsum("kj,jm->jkm", hA, hB))
    assert (g.batch, g.M, g.N, g.Ko * g.Ki) == (4, 3, 2, 1) and (g.a_b, g.b_b, g.c_b) == (1, 2, 6)
    # an M letter that does not merge with the rest of its group rides in the batch, stride 0 on the operand without it
    hA, hB = ints((3, 4, 2), 3), ints((2, 5), 4)
    got, g, names = run_contract(mem, "abk,kn->anb", hA, hB)
    assert names == ["ttsk_gemm"] and np.array_equal(got, np.einsum("abk,kn->anb", hA, hB))
    assert (g.batch, g.M, g.N, g.b_b) == (3, 4, 5, 0)
    hA, hB = ints((3, 4, 2), 5), ints((4, 3, 5), 6)
    got, g, names = run_contract(mem, "ijk,jil->kl", hA, hB)
    assert names == ["ttsk_gemm"] and np.array_equal(got, np.einsum("ijk,jil->kl", hA, hB))
    assert sorted((g.Ko, g.Ki)) == [3, 4] and (g.M, g.N, g.batch) == (2, 5, 1)


def test_contract_falls_back_by_copying(mem):
    hA, hB = ints((3, 4, 2, 2), 7), ints((2, 2, 4), 8)
    got, g, names = run_contract(mem, "abcd,dcb->a", hA, hB)
    assert names == ["ttsk_copy_strided", "ttsk_gemm"] and np.array_equal(got, np.einsum("abcd,dcb->a", hA, hB))
    assert (g.M, g.N, g.Ko * g.Ki) == (3, 1, 16)
    hA, hB = ints((3, 4, 2), 9), ints((3, 2, 2), 10)
    got, g, names = run_contract(mem, "iaj,ibj->abij", hA, hB)
    assert names == ["ttsk_copy_strided", "ttsk_copy_strided", "ttsk_gemm"] and np.array_equal(got, np.einsum("iaj,ibj->abij", hA, hB))


def test_contract_scalar_empty_and_unit_extents(mem):
    hA, hB = ints((5,), 11), ints((5,), 12)
    got, g, names = run_contract(mem, "a,a->", hA, hB)
    assert got.shape == () and got == hA @ hB and names == ["ttsk_gemm"] and (g.batch, g.M, g.N, g.Ki) == (1, 1, 1, 5)
    got, g, names = run_contract(mem, "ab,b->a", np.empty((3, 0)), np.empty((0,)))             # K = 0: zeros, and they are written
    assert names == ["ttsk_gemm"] and g.Ko * g.Ki == 0 and np.array_equal(got, np.zeros(3))
    got, g, names = run_contract(mem, "ab,b->a", np.empty((0, 4)), ints((4,), 13))             # an empty result: nothing to do
    assert got.shape == (0,) and mem.calls == []
    for spec, sa, sb in (("ak,kb->ab", (1, 1), (1, 1)), ("bak,bkn->ban", (1, 1, 1), (1, 1, 1)), ("ak,kb->ba", (1, 3), (3, 1)), ("abk,kcd->dacb", (1, 2, 1), (1, 1, 3)),
                         ("ka,kb->ab", (1, 4), (1, 1)), ("bak,bkn->nab", (2, 1, 3), (2, 3, 1))):
        hA, hB = ints(sa, 14), ints(sb, 15)
        try:
            got, g, names = run_contract(mem, spec, hA, hB)
        except ValueError as e:
            assert "cannot be lowered onto the strided GEMM" in str(e), (spec, str(e))
            continue
        assert np.array_equal(got, np.einsum(spec, hA, hB)), spec


def test_contract_into_a_strided_out(mem):
    hA, hB, hC = ints((4, 3), 16), ints((3, 5), 17), ints((4, 9), 18)
    want = np.einsum("ik,kj->ij", hA, hB)
    A, B = DevArray.from_host(hA), DevArray.from_host(hB)
    C = DevArray.from_host(hC)
    del mem.calls[:]
    out = contract("ik,kj->ij", A, B, out=C[:, 2:7])
    assert out.buf is C.buf and mem.names() == ["ttsk_gemm"]
    exp = hC.copy()
    exp[:, 2:7] = want
    assert np.array_equal(C.get(), exp)
    contract("ik,kj->ij", A, B, out=C[:, 2:7], alpha=-2.0, accumulate=True)
    exp[:, 2:7] += -2.0 * want
    assert np.array_equal(C.get(), exp)
    contract("ik,kj->ji", A, B, out=C[:, 1:6].T[:, :], accumulate=True)                         # a transposed, strided out
    exp[:, 1:6] += want
    assert np.array_equal(C.get(), exp)
    # out=None with accumulate=True: the fresh buffer (NaN here) is not read
    del mem.calls[:]
    got = contract("ik,kj->ij", A, B, accumulate=True)
    assert mem.calls[0][1][0]._obj.accumulate == 0 and np.array_equal(got.get(), want)
    # k_scale multiplies along the contracted index
    s = ints((3,), 19)
    got = contract("ik,kj->ij", A, B, k_scale=DevArray.from_host(s))
    assert np.array_equal(got.get(), np.einsum("ik,k,kj->ij", hA, s, hB))


def test_contract_errors(mem):
    A, B = DevArray.from_host(ints((3, 4), 20)), DevArray.from_host(ints((4, 5), 21))
    with pytest.raises(ValueError, match=r"operand ranks 2, 2"):
        contract("ijk,kl->ijl", A, B)
    with pytest.raises(ValueError, match=r"operand ranks"):
        contract("ik,k->i", A, B)
    with pytest.raises(ValueError, match=r"extent mismatch on 'k'"):
        contract("ik,jk->ij", A, B)
    with pytest.raises(ValueError, match=r"out has shape \(3, 4\), expected \(3, 5\)"):
        contract("ik,kj->ij", A, B, out=DevArray.empty((3, 4)))
    with pytest.raises(ValueError, match=r"index 'k' is summed in one operand only"):
        contract("ik,lj->ij", A, B)
    with pytest.raises(ValueError, match=r"index 'j' is summed in one operand only"):
        contract("ik,kj->i", A, B)
    for ks in (DevArray.from_host(ints((5,), 22)), DevArray.from_host(ints((4, 2), 23))[:, 0]):
        with pytest.raises(ValueError, match="k_scale must be a contiguous vector over the contracted index"):
            contract("ik,kj->ij", A, B, k_scale=ks)
    # groups that interleave in the output: refused once the operands have been materialised
    P, Q = DevArray.from_host(ints((2, 3), 24)), DevArray.from_host(ints((2, 3), 25))
    del mem.calls[:]
    with pytest.raises(ValueError, match="contract ab,cd->acbd: cannot be lowered onto the strided GEMM"):
        contract("ab,cd->acbd", P, Q)
    assert "ttsk_gemm" not in mem.names()
    # the fall-back writes a contiguous out only
    X, Y = DevArray.from_host(ints((3, 4, 2, 2), 26)), DevArray.from_host(ints((2, 2, 4), 27))
    big = DevArray.from_host(ints((3, 2), 28))
    del mem.calls[:]
    with pytest.raises(ValueError, match="a strided `out` needs mergeable index groups"):
        contract("abcd,dcb->a", X, Y, out=big[:, 0])
    assert mem.calls == [] and np.array_equal(big.get(), ints((3, 2), 28))


# ------------------------------------------------------------------------------------------------ axpby(): the wrapper
def test_axpby_wrapper_checks(mem):
    hy, hx = ints((3, 4), 29), ints((4, 3), 30)
    y, x = DevArray.from_host(hy), DevArray.from_host(hx)
    with pytest.raises(ValueError, match="axpby: shape mismatch"):
        axpby(y, x)
    with pytest.raises(ValueError, match="axpby: destination must be contiguous"):
        axpby(y.T, x)
    del mem.calls[:]
    assert axpby(y, x.T, 2.0, -1.0) is y                                   # a strided x is made contiguous first
    assert mem.names() == ["ttsk_copy_strided", "ttsk_axpby"]
    args = mem.calls[1][1]
    assert addr_of(args[0]) == y.ptr and addr_of(args[1]) not in (x.ptr, y.ptr) and args[2:5] == (2.0, -1.0, 12)
    assert np.array_equal(y.get(), 2.0 * hx.T - hy) and np.array_equal(x.get(), hx)
    del mem.calls[:]
    axpby(y, y, 3.0, 0.0)                                                  # tensor.py's in-place scaling
    assert mem.names() == ["ttsk_axpby"] and np.array_equal(y.get(), 3.0 * (2.0 * hx.T - hy))
    fresh = DevArray.empty((3, 4))                                         # NaN here: b == 0 must not read it
    axpby(fresh, y, 1.0, 0.0)
    assert np.array_equal(fresh.get(), y.get())
    del mem.calls[:]
    axpby(DevArray.empty((0, 2)), DevArray.empty((0, 2)))
    assert mem.calls == []
