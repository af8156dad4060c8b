"""The library's stated summation order (csrc/wave.h: ``wave_sum``, ``block_total``; csrc/reduce.hip: ``sum_partials``),
pinned bit for bit where a host model can reproduce it exactly: ``ttsk_sumsq`` = ``sumsq_kernel`` -> ``block_total<1>`` ->
``sum_partials`` at W = 1.

Inputs are doubles whose significand fits 24 bits (float32 values, scaled by exact powers of two over 2^-20 .. 2^20), so
x * x is exact and the kernel's ``fma(x, x, s)`` is NumPy's ``s + x * x``: the model below then gives the device's bits, and a
different order of the very same terms gives other bits (``test_model_sees_the_order``).

The order.  blocks = min(ceil(n / 2048), 4096) workgroups of 256 threads; thread t of block b adds the elements
b 256 + t + k blocks 256 in ascending k; the 64 lanes of a wave by the xor butterfly 32, 16, ..., 1; the four waves as
(w0 + w1) + (w2 + w3).  The closing kernel: thread t adds the blocks' partials t, t + 256, ... in ascending order, then
the same butterfly and the same combination of the four waves.
"""
import ctypes
import functools

import numpy as np
import pytest

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 2048, 2049, 4097, 524289)     # 524289: 257 blocks, thread 0 of the closing
                                                                        # kernel takes a second partial


def paired(w):
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def left_to_right(w):
    return ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]


def block_total(s, combine):
    """s (..., 256): one value per thread -> (...): what thread 0 gets"""
    v = s.reshape(s.shape[:-1] + (4, 64)).copy()
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lane ^ o]
    return combine(v[..., 0])


def strided_sum(terms, width):
    """terms (m,) non-negative -> (width,): entry t is terms[t] + terms[t + width] + ... added in ascending order from 0.0
    (the zeros that pad the last step change no bit of a non-negative sum)"""
    steps = -(-terms.size // width)
    padded = np.zeros(steps * width)
    padded[:terms.size] = terms
    acc = np.zeros(width)
    for row in padded.reshape(steps, width):
        acc = acc + row
    return acc


def model(x, combine=paired):
    blocks = min(-(-x.size // 2048), 4096)
    if blocks == 0:
        return 0.0
    part = block_total(strided_sum(x * x, blocks * 256).reshape(blocks, 256), combine)
    return float(block_total(strided_sum(part, 256), combine))


@functools.lru_cache(maxsize=None)
def inputs(n):
    rng = np.random.default_rng(1000 + n)
    x = np.ldexp(rng.standard_normal(n).astype(np.float32), rng.integers(-20, 21, n).astype(np.int32))
    assert x.dtype == np.float32
    return x.astype(np.float64)


def test_model_sees_the_order():
    """the four waves combined left to right give other bits on some of the inputs: the device test can see the order"""
    assert any(model(inputs(n)) != model(inputs(n), left_to_right) for n in SIZES)
    for n in SIZES:                                 # and the model sums what it should
        x = inputs(n)
        assert abs(model(x) - float(x @ x)) <= 1e-12 * float(x @ x)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_sumsq_bits(n):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    nat.call("ttsk_init", 0)
    x = inputs(n)
    out = DevArray.from_host(np.full(1, np.nan))
    dx = DevArray.from_host(x) if n else None
    nat.call("ttsk_sumsq", None if dx is None else ctypes.c_void_p(dx.ptr), ctypes.c_size_t(n), ctypes.c_void_p(out.ptr), 0)
    nat.call("ttsk_sync", -1)
    got, want = out.get(), np.array([model(x)])
    print(f"n={n}: device {got[0].hex()} model {want[0].hex()} left-to-right {model(x, left_to_right).hex()}")
    assert np.array_equal(got, want)
