"""What the exact, element-wise edge tests share.  Host part: the sentinel and padding values, guarded buffers and the checks
on them, the two acceptance rules (equality; an element-wise bound, then a Frobenius bar).  Device part: the fixtures that
initialise the library and the one guarded call of a C entry point.  Plain module: it imports neither tt_sketch_amd nor
anything of a device until a fixture or run_entry is used.  Guard widths and the Frobenius bar differ per kernel family:
they are arguments, each tests/*_ref.py passes its own.

Fixtures are imported by name into the test modules that use them (pytest registers them there, one instance per module)."""
import ctypes

import numpy as np
import pytest

C_BOUND = 2.0                                    # the factor of every derived rounding bound (the argument: tests/test_gpu_gemm_families.py)
PAD = 1e300                                      # operand elements outside the view: a read that meets a nonzero partner shows
SENT_F = np.float64(-1.0 / 3.0)                  # finite, no multiple of 1/2: an unwritten element fails an integer pass,
SENT = np.float64(-1.0 / 3.0).view(np.uint64)    # a stray store changes a guard (compared by its bits)
LD = np.longdouble
PROF_OTHER = 11                                  # csrc/prof.h: the bracket class of an entry point called directly


# ------------------------------------------------------------------------------------------------ buffers
def strided(buf, off, shape, strides):
    """the view of 8-byte elements at buf[off:] with the given element strides"""
    return np.lib.stride_tricks.as_strided(buf[off:], shape=shape, strides=tuple(8 * s for s in strides))


def sentinel_buffer(n, pre, post):
    """n elements with pre / post guard elements around them, every one the sentinel"""
    return np.full(pre + n + post, SENT, dtype=np.uint64).view(np.float64)


def guarded(arr, pre, post, off=0, fill=SENT):
    """arr, flat, `off` elements behind the first guard; everything around it is `fill` (the sentinel's bits or a float)"""
    b = sentinel_buffer(off + arr.size, pre, post) if isinstance(fill, np.uint64) else np.full(pre + off + arr.size + post, fill)
    b[pre + off:pre + off + arr.size] = arr.reshape(-1)
    return b


def inside_mask(size, views):
    """True where a buffer of `size` elements is addressed by one of the views (offset, shape, element strides)"""
    idx = np.arange(size, dtype=np.int64)
    mark = np.zeros(size, dtype=bool)
    for off, shape, strides in views:
        mark[strided(idx, off, shape, strides).reshape(-1)] = True
    return mark


# ------------------------------------------------------------------------------------------------ checks
def assert_guards(buf, views, what):
    """every element of buf that no view addresses still holds the sentinel"""
    bad = np.flatnonzero(~inside_mask(buf.size, views) & (buf.view(np.uint64) != SENT))
    assert bad.size == 0, "%s: %d guard / padding elements overwritten, first at buffer index %s" % (what, bad.size, bad[:8].tolist())


def _named(x):
    return x.items() if isinstance(x, dict) else enumerate(x)


def assert_untouched(bufs, what):
    """a refused call: nothing written at all.  bufs: a list or a dict of sentinel buffers"""
    for name, b in _named(bufs):
        assert (b.view(np.uint64) == SENT).all(), "%s[%s] was written by a refused call" % (what, name)


def exact(got, want, what):
    if not np.array_equal(got, want):
        diff = np.argwhere(~(got == want))
        i = tuple(int(x) for x in diff[0])
        raise AssertionError("%s: %d of %d elements differ from the exact result, first at %s: got %r, exact %r" % (what, len(diff), got.size, i, got[i], want[i]))


def bounded(got, hi, lo, tol, what, frob):
    """|got - (hi + lo)| <= tol in every element (a NaN fails), then the Frobenius ratio against `frob`; -> the largest |err| / tol"""
    err = np.abs((got - hi) - lo)
    over = ~(err <= tol)
    if over.any():
        i = tuple(int(x) for x in np.argwhere(over)[0])
        raise AssertionError("%s: %d of %d elements outside the bound, first at %s: got %r, ref %r, |err| %.3e > %.3e"
                             % (what, int(over.sum()), got.size, i, got[i], hi[i], err[i], tol[i]))
    rn = float(np.linalg.norm(hi))
    if rn > 0:
        r = float(np.linalg.norm(err)) / rn
        assert r <= frob, "%s: Frobenius ratio %.3e" % (what, r)
    return float(np.max(err / np.where(tol > 0, tol, 1.0), initial=0.0))


def same_bits(a, b, what):
    """a and b -- arrays, or lists / tuples / dicts of them, nested alike; None only against None -- hold the same bits"""
    if a is None or b is None:
        assert a is None and b is None, "%s: one of the two is missing" % what
    elif isinstance(a, np.ndarray):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64)), "%s differs in its bits" % what
    else:
        assert len(a) == len(b), "%s: %d against %d pieces" % (what, len(a), len(b))
        for k, x in _named(a):
            same_bits(x, b[k], "%s[%s]" % (what, k))


def rel_max(a, b):
    """max |a - b| over max |b|"""
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


def rel_fro(a, b):
    """the Frobenius norm of a - b over that of b"""
    return float(np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b))


# ------------------------------------------------------------------------------------------------ device
@pytest.fixture(scope="module")
def tsa():
    import tt_sketch_amd
    from tt_sketch_amd import _native
    _native.call("ttsk_init", 0)
    return tt_sketch_amd


@pytest.fixture(scope="module")
def nat():
    from tt_sketch_amd import _native
    _native.call("ttsk_init", 0)
    return _native


@pytest.fixture(scope="module")
def num_cu(nat):
    cu, hbm, name = ctypes.c_int(), ctypes.c_size_t(), ctypes.create_string_buffer(128)
    nat.call("ttsk_device_info", name, ctypes.c_size_t(len(name)), ctypes.byref(cu), ctypes.byref(hbm))
    if cu.value != 256:
        print("note: %d compute units, the tags assume 256: the kernel names are not compared" % cu.value)
    return cu.value


def run_entry(nat, entry, args, what, profile_cls=None):
    """Sync, call the C entry point, sync.  TtskUnsupported (and an argument error's ValueError) reach the caller.  Any other
    TtskError is a HIP error: the device may have faulted, so the whole pytest run ends there with status 3 and nothing
    more is started on it.  profile_cls: the call runs with profiling on and the kernel name its bracket of that class
    recorded is returned (else None); profiling is switched off again whatever happens."""
    nat.call("ttsk_sync", -1)
    if profile_cls is not None:
        nat.call("ttsk_prof_enable", 1)
    try:
        try:
            nat.call(entry, *args)
            nat.call("ttsk_sync", -1)
        except nat.TtskUnsupported:
            raise
        except nat.TtskError as e:
            pytest.exit("%s: %s" % (what, e), returncode=3)
        if profile_cls is None:
            return None
        buf = ctypes.create_string_buffer(160)
        nat.call("ttsk_prof_kernel_name", profile_cls, buf, ctypes.c_size_t(len(buf)))
        return buf.value.decode()
    finally:
        if profile_cls is not None:
            nat.call("ttsk_prof_enable", 0)


def assert_bits_equal(dev_array, host_array, what):
    """the operand on the device still holds the bits of its host image"""
    assert np.array_equal(dev_array.get().view(np.uint64), host_array.view(np.uint64)), "%s was written" % what
