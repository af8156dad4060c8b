"""Which path a call takes, asked before anything touches the device: the sketch methods, the one rule by which a fused
path accepts a pair of DRMs (``drm_pair``), and the one switch between a path's kernel and its ``contract`` composition
(``forced`` / ``resolve`` / ``taken``).  Imported by ``sketch_dispatch``, ``sketch``, ``tensor``, ``operator_product`` and
the fused modules, and imports none of them.
"""
from __future__ import annotations

import contextlib
import enum
from typing import Optional

from .drm.tensor_train_drm import TensorTrainDRM


class SketchMethod(enum.Enum):
    streaming = "streaming"
    orthogonal = "orthogonal"
    hmt = "hmt"


# ------------------------------------------------------------------ acceptance of a DRM pair
def drm_pair(shape, left_drm, right_drm, *, kinds=(TensorTrainDRM,), need_left: bool = True, cores: bool = True,
             sliced_ok: bool = True, mismatch_raises: bool = True) -> bool:
    """Whether a fused path takes this pair of DRMs for tensors of ``shape``.  In this order:

    1. each DRM is of exactly one of ``kinds`` (no subclass: it may sample or cut differently), the left one is not
       transposed and the right one is;
    2. ``cores``: at least two modes, and ``d - 1`` cores in each DRM;
    3. unless ``sliced_ok``: neither DRM is a rank slice (a block of a blocked sketch, which hands out only the columns
       ``rank_min:rank_max`` of its cores);
    4. both DRMs have the tensor's shape -- where they do not, ``mismatch_raises`` decides between the ``ValueError`` of the
       generic path (``drm_base.handle_transpose``; it names the shape of the first DRM looked at, the left one) and a decline.

    ``need_left=False`` (the one-sided ``hmt`` sketch) looks at the right DRM only.  False is a decline: the caller returns
    None and the next path is asked.  What each caller asks, after its own tests of the method and of the tensor's type:

    ========================================  ==============  ==========  =====  =========  ===============
    caller                                    kinds           need_left   cores  sliced_ok  mismatch_raises
    ========================================  ==============  ==========  =====  =========  ===============
    ``tt_fused.try_stream_sketch``            TensorTrainDRM  yes         yes    yes        yes
    ``cp_fused.try_cp_sketch``                TensorTrainDRM  yes         yes    yes        yes
    ``operator_fused.try_operator_sketch``    TensorTrainDRM  yes         yes    no         yes
    ``hadamard_fused.try_hadamard_sketch``    TensorTrainDRM  yes         yes    no         yes
    ``tt_fused.try_orth_sketch``              TensorTrainDRM  orthogonal  yes    no         no
    ``tt_fused.try_orth_sketch_batch``        TensorTrainDRM  orthogonal  yes    no         no
    ``sketch.stream_sketch_batch``            TensorTrainDRM  yes         no     yes        yes
    ``sparse_fused.try_sparse_gauss_sketch``  hashed, train,  yes         no     yes        yes
                                              Khatri-Rao
    ========================================  ==============  ==========  =====  =========  ===============

    ``stream_sketch_batch`` leaves the count of cores to ``TTSketchPlan``.  The sparse path takes SparseGaussianDRM,
    SparseSignDRM, TensorTrainDRM and KhatriRaoDRM in any pairing: the hashed DRMs have no cores, so it asks for no count
    here and tests the number of modes, and ``d - 1`` cores of a train or matrices of a Khatri-Rao DRM, with its other
    limits.  Every other caller declines a KhatriRaoDRM: its sketches of trains, CP and Tucker tensors run on the generic
    driver."""
    # (plain tests, no generator expressions: this runs on every public sketch call)
    if type(right_drm) not in kinds or not right_drm.transpose:
        return False
    if need_left and (type(left_drm) not in kinds or left_drm.transpose):
        return False
    drms = (left_drm, right_drm) if need_left else (right_drm,)
    d = len(shape)
    shape = tuple(shape)
    for m in drms:
        if cores and (d < 2 or len(m.cores) != d - 1):
            return False
    if not sliced_ok:
        for m in drms:
            if tuple(m.rank_min) != (0,) * (d - 1) or tuple(m.rank_max) != tuple(m.true_rank):
                return False
    for m in drms:
        if tuple(m.shape) != shape:
            if mismatch_raises:
                raise ValueError(f"Shape {drms[0].shape} of DRM doesn't match tensor's shape {shape}")
            return False
    return True


# ------------------------------------------------------------------ kernel or composition
# Where a path has both a kernel and a composition from ``contract`` calls, its entry takes ``route=``: None is the path's
# cost rule (``cp_fused.chain_route_ms``, ``operator_product.route_ms``, ``hadamard_product.route_ms``, ``hadamard_gram.close_route_ms``, ``operator_gram.close_route_ms``, ``tensor_gram._gram_route_ms``,
# ``sparse_fused.chain_route_ms``), ``"composed"`` never
# calls the library entry, ``"kernel"`` calls it and lets its ``TtskUnsupported`` propagate, so that a test or a benchmark
# knows which code it ran.  ``forced`` sets the route of every call made without the keyword.
ROUTES = (None, "kernel", "composed")
_forced: Optional[str] = None


def _valid(route: Optional[str]) -> Optional[str]:
    if route not in ROUTES:
        raise ValueError(f"route {route!r}: 'kernel', 'composed' or None")
    return route


@contextlib.contextmanager
def forced(route: Optional[str]):
    """Every routed call inside the block that names no route of its own takes ``route``."""
    global _forced
    saved, _forced = _forced, _valid(route)
    try:
        yield
    finally:
        _forced = saved


def resolve(route: Optional[str]) -> Optional[str]:
    """the route a call was given, or else the one ``forced`` has set, or else None"""
    return _forced if _valid(route) is None else route


def taken(route: Optional[str], kernel_ms: float, composed_ms: float) -> str:
    """the route of a call: the resolved ``route``, or under None what the path's cost rule expects to be faster (a caller
    whose rule costs something evaluates it under None only)"""
    return route or ("composed" if composed_ms < kernel_ms else "kernel")
