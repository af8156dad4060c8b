"""The layout of the tensor modules: ``tensor`` (the classes) and the device passes ``tensor_gather``, ``tensor_dense``,
``tensor_gram``, which import the classes from it while it reaches them only from inside its methods.  Needs neither
a GPU nor the built library."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = ("tensor_gather", "tensor_dense", "tensor_gram")

ALL = [
    "ALL_DRM", "DenseGaussianDRM", "SparseGaussianDRM", "SparseSignDRM", "TensorTrainDRM",
    "SketchedTensorTrain", "assemble_sketched_tt", "blocked_stream_sketch", "hmt_sketch",
    "orthogonal_sketch", "orthogonal_sketch_batch", "hmt_sketch_batch", "stream_sketch", "stream_sketch_batch", "to_tt_batch", "SketchContainer", "SketchMethod", "general_sketch",
    "CPTensor", "DenseTensor", "SparseTensor", "Tensor", "TensorSum", "TensorTrain", "TuckerTensor",
    "tt_svd", "tt_gram", "cp_gram", "OperatorProduct", "HadamardProduct", "hadamard_round",
]


@pytest.mark.parametrize("module", ("tensor",) + PASSES)
def test_each_module_imports_first(module):
    """Every one of the four as the first ``tt_sketch_amd`` import of a fresh interpreter: no import cycle."""
    run = subprocess.run([sys.executable, "-c", f"import tt_sketch_amd.{module}"], cwd=ROOT,
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr


def test_no_pass_can_reach_host():
    import importlib
    for name in PASSES:
        assert not hasattr(importlib.import_module(f"tt_sketch_amd.{name}"), "_host"), name


def test_public_names():
    import tt_sketch_amd as tsa
    from tt_sketch_amd import tensor_gram
    assert tsa.tt_gram is tensor_gram.tt_gram
    assert tsa.cp_gram is tensor_gram.cp_gram
    assert tsa.__all__ == ALL


def test_core_list_mixin_is_shared():
    from tt_sketch_amd import CPTensor, TensorTrain
    for name in ("dev_cores", "prepare_device", "resident", "__getitem__", "__setitem__", "gather_dev", "support_error"):
        assert getattr(TensorTrain, name) is getattr(CPTensor, name), name
    assert TensorTrain.prepare_device is TensorTrain.dev_cores
