"""What each fused sketch path accepts, pinned without a device: the five tensor-train ``try_*`` functions and the
batched-or-one-by-one decision of ``stream_sketch_batch`` on tiny host objects, for every DRM pair that is wrong in one way
and every method.  An outcome is ``None`` (declined), the name of the first library entry the path was about to call
(accepted), or the exception's type and message.  The library is replaced by a recorder: allocations, uploads and memsets
pass (nothing is dereferenced), every other entry raises with its name."""
import sys

import numpy as np
import pytest

import tt_sketch_amd as tsa
from tt_sketch_amd import _native as nat, cp_fused, device, operator_fused, operator_product, sketch, tt_fused
from tt_sketch_amd.drm_base import DRM
from tt_sketch_amd.tt_gmres import MPO

SHAPE = (4, 5, 6)
LEFT_RANK, RIGHT_RANK = (2, 2), (3, 3)
METHODS = ("streaming", "orthogonal", "hmt")
CASES = ("correct", "swapped", "right not transposed", "other class", "subclass", "left of shape 4 5 7", "right of shape 4 5 7",
         "core short", "rank slice", "d = 1", "core short, of shape 4 5 7", "rank slice of shape 4 5 7")


class _Reached(Exception):
    """the path got as far as this library entry"""


class _SubDRM(tsa.TensorTrainDRM):
    pass


@pytest.fixture
def recorder(monkeypatch):
    ptr, made_up = [1 << 20], set()

    def call(name, *args):
        if name == "ttsk_malloc":
            ptr[0] += 1 << 20
            made_up.add(ptr[0])
            args[0]._obj.value = ptr[0]
        elif name not in ("ttsk_h2d", "ttsk_memset"):
            raise _Reached(name)

    class _Lib:
        def __getattr__(self, name):
            raise _Reached(name)

    monkeypatch.setattr(nat, "call", call)
    monkeypatch.setattr(nat, "lib", lambda: _Lib())
    monkeypatch.setattr(device, "_pool", {})                       # the made-up addresses stay out of the real pool
    monkeypatch.setattr(device, "_pool_bytes", {True: 0, False: 0})
    monkeypatch.setattr(operator_product, "_one", None)            # chain_start() caches its array there
    monkeypatch.setattr(sketch, "stream_sketch", _one_by_one)
    yield
    # nothing of the package may keep an array at a made-up address once the test is over: a later test on a real device
    # in the same process would hand it to the library
    monkeypatch.undo()
    held = [f"{name}.{key}" for name, mod in list(sys.modules.items()) if name.startswith("tt_sketch_amd") and mod is not None
            for key, val in vars(mod).items() for a in _arrays(val) if a.buf.ptr in made_up]
    assert not held, held


def _arrays(val, depth=2):
    """the device arrays a module global holds, itself or inside a list / tuple / dict"""
    if isinstance(val, device.DevArray):
        yield val
    elif depth and isinstance(val, (list, tuple, dict)):
        for v in (val.values() if isinstance(val, dict) else val):
            yield from _arrays(v, depth - 1)


def _one_by_one(*args, **kwargs):
    raise _Reached("one by one")


def _drm(cls, shape, rank, transpose, cores=None, **kw):
    walk = shape[::-1] if transpose else shape
    rk = (1,) + tuple(kw.get("true_rank", rank))
    if cores is None:
        cores = [np.ones((rk[k], walk[k], rk[k + 1])) for k in range(len(shape) - 1)]
    if cls is DRM:
        return DRM(rank, shape, transpose, seed=1, **kw)
    return cls(rank, shape, transpose, seed=1, cores=cores, **kw)


def _pair(case):
    """(shape of the tensors, left DRM, right DRM)"""
    T = tsa.TensorTrainDRM
    L, R = _drm(T, SHAPE, LEFT_RANK, False), _drm(T, SHAPE, RIGHT_RANK, True)
    if case == "correct":
        return SHAPE, L, R
    if case == "swapped":
        return SHAPE, R, L
    if case == "right not transposed":
        return SHAPE, L, _drm(T, SHAPE, RIGHT_RANK, False)
    if case == "other class":
        return SHAPE, L, _drm(DRM, SHAPE, RIGHT_RANK, True)
    if case == "subclass":
        return SHAPE, L, _drm(_SubDRM, SHAPE, RIGHT_RANK, True)
    if case == "left of shape 4 5 7":
        return SHAPE, _drm(T, (4, 5, 7), LEFT_RANK, False), R
    if case == "right of shape 4 5 7":
        return SHAPE, L, _drm(T, (4, 5, 7), RIGHT_RANK, True)
    if case == "core short":
        return SHAPE, L, _drm(T, SHAPE, RIGHT_RANK, True, cores=[np.ones((1, 6, 3))])
    if case == "rank slice":
        return SHAPE, L, _drm(T, SHAPE, (4, 4), True, rank_min=(1, 1), rank_max=(4, 4), true_rank=(4, 4))
    if case == "core short, of shape 4 5 7":
        return SHAPE, L, _drm(T, (4, 5, 7), RIGHT_RANK, True, cores=[np.ones((1, 7, 3))])
    if case == "rank slice of shape 4 5 7":
        return SHAPE, L, _drm(T, (4, 5, 7), (4, 4), True, rank_min=(1, 1), rank_max=(4, 4), true_rank=(4, 4))
    if case == "d = 1":
        return (4,), _drm(T, (4,), (), False), _drm(T, (4,), (), True)
    raise KeyError(case)


def _train(shape, r=2):
    rk = (1,) + (r,) * (len(shape) - 1) + (1,)
    return tsa.TensorTrain([np.ones((rk[k], n, rk[k + 1])) for k, n in enumerate(shape)])


def _tensor(kind, shape):
    if kind == "train":
        return _train(shape)
    if kind == "sum":
        return tsa.TensorSum([_train(shape), _train(shape, 1)])
    if kind == "cp":
        return tsa.CPTensor([np.ones((n, 3)) for n in shape])
    if kind == "product":
        rk = (1,) + (2,) * (len(shape) - 1) + (1,)
        return tsa.OperatorProduct(MPO([np.ones((rk[k], n, n, rk[k + 1])) for k, n in enumerate(shape)]), _train(shape))
    raise KeyError(kind)


def _batch_decision(tensors, left, right, method):
    return sketch.stream_sketch_batch(tensors, left.rank, tuple(right.rank[::-1]), left_drm=left, right_drm=right)


# caller -> (function, the tensor it is made for, as a list where it takes one)
CALLERS = {
    "stream": (tt_fused.try_stream_sketch, "train", False),
    "stream of a sum": (tt_fused.try_stream_sketch, "sum", False),
    "orth": (tt_fused.try_orth_sketch, "train", False),
    "orth batch": (tt_fused.try_orth_sketch_batch, "train", True),
    "operator": (operator_fused.try_operator_sketch, "product", False),
    "cp": (cp_fused.try_cp_sketch, "cp", False),
    "batch decision": (_batch_decision, "train", True),
}


def _outcome(caller, case, method):
    fn, kind, many = CALLERS[caller]
    shape, left, right = _pair(case)
    tensor = _tensor(kind, shape)
    try:
        out = fn([tensor, _tensor(kind, shape)] if many else tensor, left, right, tsa.SketchMethod(method))
    except _Reached as e:
        return str(e)
    except Exception as e:
        return f"{type(e).__name__}: {e}"
    assert out is None
    return None


SIZE, ORTH, BATCH, GEMM, WAIT, ONE = ("ttsk_tt_sketch_size", "ttsk_tt_orth_sketch", "ttsk_tt_orth_sketch_batch", "ttsk_gemm",
                                      "ttsk_stream_wait", "one by one")
LEFT_7 = "ValueError: Shape (4, 5, 7) of DRM doesn't match tensor's shape (4, 5, 6)"
RIGHT_7 = "ValueError: Shape (4, 5, 6) of DRM doesn't match tensor's shape (4, 5, 6)"          # the message names the left DRM's shape
# (caller, method) -> the outcome per case, in the order of CASES; every pair not listed declines all of them
#                                   correct swapped not-T  class  subcl. left 7  right 7  short  slice  d = 1  short 7  slice 7
EXPECT = {
    ("stream", "streaming"):          (SIZE,  None,   None,  None,  None,  LEFT_7, RIGHT_7, None,  SIZE,  None,  None,    RIGHT_7),
    ("stream of a sum", "streaming"): (SIZE,  None,   None,  None,  None,  LEFT_7, RIGHT_7, None,  SIZE,  None,  None,    RIGHT_7),
    ("orth", "orthogonal"):           (ORTH,  None,   None,  None,  None,  None,   None,    None,  None,  None,  None,    None),
    ("orth", "hmt"):                  (ORTH,  None,   None,  None,  None,  ORTH,   None,    None,  None,  None,  None,    None),
    ("orth batch", "orthogonal"):     (BATCH, None,   None,  None,  None,  None,   None,    None,  None,  None,  None,    None),
    ("orth batch", "hmt"):            (BATCH, None,   None,  None,  None,  BATCH,  None,    None,  None,  None,  None,    None),
    ("operator", "streaming"):        (GEMM,  None,   None,  None,  None,  LEFT_7, RIGHT_7, None,  None,  None,  None,    None),
    ("cp", "streaming"):              (WAIT,  None,   None,  None,  None,  LEFT_7, RIGHT_7, None,  WAIT,  None,  None,    RIGHT_7),
}
for _m in METHODS:          # the decision does not look at a method
    EXPECT[("batch decision", _m)] = (SIZE,  ONE,    ONE,   ONE,   ONE,   LEFT_7, RIGHT_7, SIZE,  SIZE,  SIZE,  RIGHT_7, RIGHT_7)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("caller", list(CALLERS))
def test_acceptance_of_every_drm_pair(recorder, caller, method):
    want = EXPECT.get((caller, method), (None,) * len(CASES))
    assert len(want) == len(CASES)
    got = tuple(_outcome(caller, case, method) for case in CASES)
    for case, g, w in zip(CASES, got, want):
        print(f"{caller} / {method} / {case}: {g}")
    assert got == want


@pytest.mark.parametrize("caller", [c for c in CALLERS if c != "batch decision"])
def test_another_kind_of_tensor_is_declined(recorder, caller):
    fn, kind, many = CALLERS[caller]
    _, left, right = _pair("correct")
    for other in ("train", "sum", "cp", "product"):
        if other == kind or (caller, other) in (("stream", "sum"), ("stream of a sum", "train")):
            continue
        t = _tensor(other, SHAPE)
        for method in METHODS:
            assert fn([t, t] if many else t, left, right, tsa.SketchMethod(method)) is None, (other, method)


def test_batch_decision_needs_trains_of_one_signature(recorder):
    _, left, right = _pair("correct")
    for tensors in ([_train(SHAPE), _train(SHAPE, 1)], [_train(SHAPE), _tensor("cp", SHAPE)], [_train(SHAPE), _train((4, 5, 5))]):
        with pytest.raises(_Reached, match=ONE):
            _batch_decision(tensors, left, right, None)
    assert _batch_decision([], left, right, None) == []
