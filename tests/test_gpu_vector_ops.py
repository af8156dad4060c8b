"""The three vector entry points -- ttsk_copy_strided, ttsk_sum_slices, ttsk_axpby (csrc/vector_ops.hip, host plans in
csrc/vector_plan.h) -- through their C entry points at every edge of their plans, and DevArray's views on the device.

The cases, operands and references are those of tests/vector_ops_ref.py (read its docstring); tests/test_vector_plan.py
shows without a GPU that each case is accepted by the plan, takes the route it is named for and, at the caps, makes the
trips of the grid-stride loop it is there for -- and that every refusal below is the plan's, so no kernel ever sees a NULL
pointer or an oversize extent from this module.

Every case: 64 guard elements around each buffer (sentinels, compared by their bits; the gaps of a strided destination
are guards too), the operands read back bit-identical, a second call on a fresh destination gives the same bits.
- copy: the whole destination buffer EQUALS, bit for bit, the image NumPy's strided assignment gives: NaN payloads,
  signalling NaNs, -0.0 and subnormals among the elements.
- sum_slices: bits equal those of the ascending NumPy float64 sum from dst or from +0.0 (dst holds NaN where accumulate = 0).
- axpby: every element is one of the three legal roundings; b == 0 leaves no NaN or inf of y behind.
A refused call raises with its message and leaves sentinel-filled buffers untouched.

The four cap cases of sum_slices with nb = 9 move up to 300 MB each; the largest was measured at half a second, nearly all
of it on the host (values, reference, the read-back of the operand), so nb = 9 is kept at the caps."""
import ctypes
import zlib

import numpy as np
import pytest

from tests import vector_ops_ref as ref
from tests.edge_kit import SENT, assert_bits_equal, assert_guards, assert_untouched, exact, guarded, nat, run_entry, same_bits, sentinel_buffer  # noqa: F401

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
G = ref.GUARD
COPY, SUM, AXPBY = ref.copy_cases(), ref.sum_cases() + ref.sum_cap_cases(), ref.axpby_cases()


def seed_of(id):
    return zlib.crc32(id.encode())


def upload(host):
    from tt_sketch_amd.device import DevArray
    d = DevArray.from_host(host)
    assert d.ptr % 256 == 0 and d.size == host.size
    return d


def at(d, off):
    return P(d.ptr + 8 * off)


def i64(nat, values):
    return nat.i64_array(list(values))


# ====================================================================================================== ttsk_copy_strided
@pytest.mark.parametrize("c", COPY, ids=[c.id for c in COPY])
def test_copy_strided_moves_bits(nat, c):
    src, dst, want = ref.copy_operands(c, seed_of(c.id))
    # both views inside the interiors of their buffers
    assert G + c.soff + ref.extent(c.shape, c.ss) + G == src.size and G + c.doff + ref.extent(c.shape, c.ds) + G == dst.size
    dS, outs = upload(src), []
    for rep in range(2):
        dD = upload(dst)
        args = [at(dD, G + c.doff), at(dS, G + c.soff), len(c.shape), i64(nat, c.shape), i64(nat, c.ds), i64(nat, c.ss), 0]
        run_entry(nat, "ttsk_copy_strided", args, c.id)
        outs.append(dD.get())
    assert_guards(outs[0], [(G + c.doff, c.shape, c.ds)], c.id)
    same_bits(outs[0], want, c.id + ": the destination buffer")
    same_bits(outs[1], outs[0], c.id + ", second call")
    assert_bits_equal(dS, src, c.id + ": src")


def _expect(nat, r, entry, args, bufs):
    """a refusal of the table: the status, the message, nothing written"""
    if r.status == "ok":
        run_entry(nat, entry, args, r.id)
    else:
        with pytest.raises(ValueError if r.status == "arg" else nat.TtskUnsupported) as e:
            run_entry(nat, entry, args, r.id)
        assert r.fragment in str(e.value), (r.id, str(e.value))
    assert_untouched({k: d.get() for k, d in bufs.items()}, "%s %s" % (entry, r.id))


COPY_REFUSED = ref.copy_refusals()


@pytest.mark.parametrize("r", COPY_REFUSED, ids=[r.id for r in COPY_REFUSED])
def test_copy_strided_refusals_write_nothing(nat, r):
    ndim, shape = r.args
    strides = ref.c_strides([max(n, 1) for n in shape])
    bufs = {"dst": upload(sentinel_buffer(32, G, G)), "src": upload(sentinel_buffer(32, G, G))}
    arr = lambda k, v: None if k in r.null else i64(nat, v)
    args = [None if "dst" in r.null else at(bufs["dst"], G), None if "src" in r.null else at(bufs["src"], G), ndim,
            arr("shape", shape), arr("ds", strides), arr("ss", strides), 0]
    _expect(nat, r, "ttsk_copy_strided", args, bufs)


# ======================================================================================================== ttsk_sum_slices
@pytest.mark.parametrize("c", SUM, ids=[c.id for c in SUM])
def test_sum_slices_adds_in_ascending_order(nat, c):
    src, dst, slices, prior = ref.sum_operands(c, ref.sum_seed(c))
    want = ref.sum_reference(c, slices, prior)
    assert G + c.soff + (c.nb - 1) * c.stride + c.n + G == src.size and G + c.doff + c.n + G == dst.size
    dS, outs = upload(src), []
    for rep in range(2):
        dD = upload(dst)
        assert ((dD.ptr + 8 * (G + c.doff)) % 16 == 0, (dS.ptr + 8 * (G + c.soff)) % 16 == 0) == ref.sum_vector_route(c)[2:]
        run_entry(nat, "ttsk_sum_slices", [at(dD, G + c.doff), at(dS, G + c.soff), c.nb, c.stride, c.n, c.acc, 0], c.id)
        outs.append(dD.get())
    assert_guards(outs[0], [(G + c.doff, (c.n,), (1,))], c.id)
    got = outs[0][G + c.doff:G + c.doff + c.n]
    if not np.array_equal(got.view(np.uint64), want.view(np.uint64)):
        exact(got, want, c.id)                                  # names the first element
        same_bits(got, want, c.id + ": a zero of the wrong sign")
    same_bits(outs[1], outs[0], c.id + ", second call")
    assert_bits_equal(dS, src, c.id + ": src")


SUM_REFUSED = ref.sum_refusals()


@pytest.mark.parametrize("r", SUM_REFUSED, ids=[r.id for r in SUM_REFUSED])
def test_sum_slices_refusals_write_nothing(nat, r):
    nb, acc, n = r.args
    bufs = {"dst": upload(sentinel_buffer(32, G, G)), "src": upload(sentinel_buffer(32, G, G))}
    args = [None if "dst" in r.null else at(bufs["dst"], G), None if "src" in r.null else at(bufs["src"], G), nb, n, n, acc, 0]
    _expect(nat, r, "ttsk_sum_slices", args, bufs)


# ============================================================================================================= ttsk_axpby
@pytest.mark.parametrize("c", AXPBY, ids=[c.id for c in AXPBY])
def test_axpby_is_one_of_the_legal_roundings(nat, c):
    x, y = ref.axpby_operands(c, seed_of(c.id))
    hx, hy = guarded(x, G, G, c.xoff), guarded(y, G, G, c.yoff)
    dX, outs = upload(hx), []
    for rep in range(2):
        dY = upload(hy)
        py = at(dY, G + c.yoff)
        run_entry(nat, "ttsk_axpby", [py, py if c.alias else at(dX, G + c.xoff), c.a, c.b, c.n, 0], c.id)
        outs.append(dY.get())
    assert_guards(outs[0], [(G + c.yoff, (c.n,), (1,))], c.id)
    got = outs[0][G + c.yoff:G + c.yoff + c.n]
    ref.axpby_check(c, got, x, y)
    if c.b == 0:
        assert np.isfinite(got).all() and np.array_equal(got, c.a * x), c.id      # exactly fl(a x): nothing of y is left
    same_bits(outs[1], outs[0], c.id + ", second call")
    assert_bits_equal(dX, hx, c.id + ": x")


AXPBY_REFUSED = ref.axpby_refusals()


@pytest.mark.parametrize("r", AXPBY_REFUSED, ids=[r.id for r in AXPBY_REFUSED])
def test_axpby_refusals_write_nothing(nat, r):
    bufs = {"y": upload(sentinel_buffer(32, G, G)), "x": upload(sentinel_buffer(32, G, G))}
    args = [None if "y" in r.null else at(bufs["y"], G), None if "x" in r.null else at(bufs["x"], G), 1.5, 2.5, r.args[0], 0]
    _expect(nat, r, "ttsk_axpby", args, bufs)


# ================================================================================================== DevArray on the device
@pytest.fixture
def calls(nat, monkeypatch):
    """the names of the entry points called from here on (the calls go through)"""
    seen, real = [], nat.call

    def recording(name, *args):
        seen.append(name)
        return real(name, *args)

    monkeypatch.setattr(nat, "call", recording)
    return seen


def patterns(rng, shape):
    """random finite doubles with every mantissa bit in play"""
    return np.ldexp(rng.random(shape) - 0.5, rng.integers(-40, 40, size=shape, dtype=np.int32))


VIEWS = {
    "transposed": lambda a: a.T,
    "permuted": lambda a: a.transpose(1, 2, 0),
    "sliced": lambda a: a[1:5, :, 2:7],
    "indexed": lambda a: a[:, 3],
    "none-indexed": lambda a: a[:, None, 2:6, 1],
    "sliced-transposed": lambda a: a[2:, 1:6].T,
}


@pytest.mark.parametrize("name", sorted(VIEWS))
def test_devarray_views_materialise_the_same_bits(nat, calls, name):
    from tt_sketch_amd.device import DevArray
    h = patterns(np.random.default_rng(seed_of(name)), (6, 7, 8))
    a = DevArray.from_host(h)
    v, w = VIEWS[name](a), VIEWS[name](h)
    assert v.shape == w.shape and not v.is_contiguous()
    del calls[:]
    same_bits(v.get(), np.ascontiguousarray(w), name + ".get()")
    same_bits(v.copy().get(), np.ascontiguousarray(w), name + ".copy()")
    c = v.contiguous()
    assert c.is_contiguous() and c.buf is not a.buf
    same_bits(c.get(), np.ascontiguousarray(w), name + ".contiguous()")
    assert calls.count("ttsk_copy_strided") == 3
    r = v.reshape(-1, 2) if w.size % 2 == 0 else v.reshape(-1)
    same_bits(r.get(), w.reshape(r.shape), name + ".reshape")
    assert calls.count("ttsk_copy_strided") == (4 if r.buf is not a.buf else 3)
    same_bits(np.asarray(v), np.ascontiguousarray(w), "np.asarray(%s)" % name)
    assert_bits_equal(a, h, name + ": the base array")


def test_devarray_copying_reshape_of_a_transposed_view(nat, calls):
    from tt_sketch_amd.device import DevArray
    h = patterns(np.random.default_rng(5), (9, 14))
    a = DevArray.from_host(h)
    r = a.T.reshape(7, 18)
    assert r.buf is not a.buf and calls.count("ttsk_copy_strided") == 1
    same_bits(r.get(), h.T.reshape(7, 18), "a.T.reshape")
    assert a.reshape(3, 3, 14).buf is a.buf and calls.count("ttsk_copy_strided") == 1


def test_copy_into_a_column_block_leaves_the_rest(nat, calls):
    from tt_sketch_amd.device import DevArray, copy_into
    h = patterns(np.random.default_rng(6), (7, 10))
    big = sentinel_buffer(10 * 20, 0, 0).reshape(10, 20)
    want = big.copy()
    want[:, 5:12] = h.T
    d = DevArray.from_host(big)
    copy_into(d[:, 5:12], DevArray.from_host(h).T)
    assert calls.count("ttsk_copy_strided") == 1
    same_bits(d.get(), want, "the larger array")
    with pytest.raises(ValueError, match="copy_into: shape"):
        copy_into(d[:, 5:11], DevArray.from_host(h).T)


def test_zeros_fill_zero_and_from_host_types(nat):
    from tt_sketch_amd.device import DevArray
    rng = np.random.default_rng(7)
    z = DevArray.zeros((5, 7))
    assert z.dtype == np.float64 and not z.get().view(np.uint64).any()
    f = DevArray.from_host(patterns(rng, (33,)))
    assert f.fill_zero() is f and not f.get().view(np.uint64).any()
    with pytest.raises(ValueError, match="contiguous"):
        DevArray.from_host(patterns(rng, (4, 4))).T.fill_zero()
    i = rng.integers(-(1 << 62), 1 << 62, size=(5, 6), dtype=np.int64)
    u = rng.integers(0, 1 << 64, size=(4, 3), dtype=np.uint64)
    s = rng.standard_normal((6, 5)).astype(np.float32)
    fo = np.asfortranarray(patterns(rng, (5, 8)))
    for h, dtype in ((i, np.int64), (u, np.uint64), (s, np.float64), (fo, np.float64)):
        d = DevArray.from_host(h)
        got = d.get()
        assert d.dtype == dtype and d.shape == h.shape and d.is_contiguous() and got.dtype == dtype
        assert np.array_equal(got, h.astype(dtype))
    assert np.array_equal(DevArray.zeros((3, 4), dtype=np.int64).get(), np.zeros((3, 4), dtype=np.int64))
    with pytest.raises(ValueError, match="fp64 only"):
        DevArray.from_host(i).T.contiguous()


def test_size_zero_arrays_launch_nothing(nat, calls):
    from tt_sketch_amd.device import DevArray, axpby, contract, copy_into
    e = DevArray.from_host(np.empty((0, 3)))
    z = DevArray.zeros((4, 0, 2))
    full, ones = DevArray.from_host(np.arange(12.0).reshape(3, 4)), DevArray.from_host(np.ones(3))
    del calls[:]
    assert e.get().shape == (0, 3) and e.T.get().shape == (3, 0) and e.T.copy().shape == (3, 0) and e.copy().shape == (0, 3)
    assert z.transpose(2, 0, 1).contiguous().shape == (2, 4, 0) and z.reshape(0, 8).shape == (0, 8) and z.reshape(-1, 4).shape == (0, 4)
    assert np.asarray(z.T).shape == (2, 0, 4) and full[1:1].get().shape == (0, 4) and full[:, 4:].T.copy().get().shape == (0, 3)
    assert z.fill_zero() is z and DevArray.zeros((0,)).size == 0 and DevArray.from_host(np.empty((2, 0), dtype=np.int64)).get().shape == (2, 0)
    copy_into(DevArray.empty((3, 0)), e.T)
    axpby(DevArray.empty((0, 3)), e, 2.0, 3.0)
    assert contract("ab,b->a", e, ones).shape == (0,)
    assert set(calls) <= {"ttsk_malloc"}, calls


def _ints(rng, shape):
    return rng.integers(-4, 5, size=shape).astype(np.float64)


def test_contract_fall_backs_copy_and_equal_einsum(nat, calls):
    """the two materialise-and-retry cases and the strided accumulate of tests/test_device_views_host.py, on the device:
    integer operands, equality with einsum, the copies seen among the calls"""
    from tt_sketch_amd.device import DevArray, contract
    rng = np.random.default_rng(8)
    A, B = _ints(rng, (3, 4, 5, 2)), _ints(rng, (2, 5, 4))
    del calls[:]
    got = contract("abcd,dcb->a", DevArray.from_host(A), DevArray.from_host(B))
    assert [c for c in calls if c in ("ttsk_copy_strided", "ttsk_gemm")] == ["ttsk_copy_strided", "ttsk_gemm"]
    exact(got.get(), np.einsum("abcd,dcb->a", A, B), "abcd,dcb->a")
    A, B = _ints(rng, (3, 4, 5)), _ints(rng, (3, 2, 5))
    del calls[:]
    got = contract("iaj,ibj->abij", DevArray.from_host(A), DevArray.from_host(B))
    assert [c for c in calls if c in ("ttsk_copy_strided", "ttsk_gemm")] == ["ttsk_copy_strided", "ttsk_copy_strided", "ttsk_gemm"]
    exact(got.get(), np.einsum("iaj,ibj->abij", A, B), "iaj,ibj->abij")
    # a strided out with mergeable groups, accumulating: only its view changes
    A, B, C = _ints(rng, (6, 5)), _ints(rng, (5, 4)), _ints(rng, (6, 11))
    dC = DevArray.from_host(C)
    del calls[:]
    out = contract("ik,kj->ij", DevArray.from_host(A), DevArray.from_host(B), out=dC[:, 3:7], alpha=2.0, accumulate=True)
    assert out.buf is dC.buf and [c for c in calls if c in ("ttsk_copy_strided", "ttsk_gemm")] == ["ttsk_gemm"]
    want = C.copy()
    want[:, 3:7] += 2.0 * (A @ B)
    exact(dC.get(), want, "strided out, accumulate")
