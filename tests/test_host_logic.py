"""CPU tests: host-side logic of tt_sketch_amd and the C-ABI surface (no compute calls)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tt_sketch_amd import _native as nat
from tt_sketch_amd.device import _view_strides
from tt_sketch_amd.utils import dematricize, matricize, process_tt_rank, trim_ranks


def test_library_exports_every_declared_symbol():
    lib = nat.lib()                      # raises if a symbol of include/ttsk.h is missing
    names = nat.declared_symbols()
    assert len(names) >= 35
    for n in names:
        assert hasattr(lib, n), n


def test_rank_processing():
    assert process_tt_rank(3, (4, 5, 6), trim=False) == (3, 3)
    assert process_tt_rank((2, 9), (4, 5, 6), trim=False) == (2, 9)
    with pytest.raises(ValueError):
        process_tt_rank((2, 3, 4), (4, 5, 6), trim=False)
    assert trim_ranks((4, 5, 6), (100, 100)) == (4, 6)
    assert trim_ranks((2, 2, 2, 2), (9, 9, 9)) == (2, 4, 2)
    assert trim_ranks((10, 10, 10), (3, 50)) == (3, 10)
    assert process_tt_rank(100, (5, 6, 7, 8), trim=True) == (5, 30, 8)


def test_matricize_roundtrip():
    A = np.arange(2 * 3 * 4 * 5.0).reshape(2, 3, 4, 5)
    for mode in range(4):
        M = matricize(A, mode)
        assert M.shape == (A.shape[mode], A.size // A.shape[mode])
        assert np.array_equal(dematricize(M, mode, A.shape), A)
    assert matricize(A, range(2), mat_shape=True).shape == (6, 20)
    assert matricize(A, range(2)).shape == (2, 3, 20)


def test_view_strides_rule():
    assert _view_strides((3, 4, 5), (20, 5, 1), (12, 5)) == (5, 1)
    assert _view_strides((3, 4, 5), (1, 3, 12), (12, 5)) is None
    assert _view_strides((1, 7, 4), (1, 1, 7), (7, 4)) == (1, 7)
    assert _view_strides((6, 5), (5, 1), (2, 3, 5)) == (15, 5, 1)


def test_drm_bookkeeping_matches_reference_conventions():
    from tt_sketch_amd.drm_base import DRM
    d = DRM((3, 4, 5), (6, 7, 8, 9), transpose=True, seed=12,
            rank_min=(1, 0, 2), rank_max=(3, 4, 5), true_rank=(3, 4, 5))
    assert d.rank_min == (2, 0, 1) and d.rank_max == (5, 4, 3) and d.rank == (3, 4, 2)
    assert d.true_rank == (5, 4, 3)
    t = d.T
    assert t.transpose is False and t.rank == (2, 4, 3) and t.rank_min == (1, 0, 2)
    assert DRM(3, (4, 5), False, seed=2**32 + 5).seed == (2**32 + 5) % (2**32 - 1)


def test_container_arithmetic_and_packing():
    from tt_sketch_amd import SketchContainer
    rng = np.random.default_rng(0)
    a = SketchContainer.zero((4, 5, 6), (2, 3), (3, 4))
    b = SketchContainer([rng.standard_normal(p.shape) for p in a.Psi_cores],
                        [rng.standard_normal(o.shape) for o in a.Omega_mats])
    c = (b + b) * 0.5 - b / 1.0
    assert all(np.allclose(x, 0) for x in c.Psi_cores + c.Omega_mats)
    assert b.left_rank == (2, 3) and b.right_rank == (3, 4) and b.shape == (4, 5, 6)
    t = b.T
    assert t.left_rank == (4, 3) and t.right_rank == (3, 2)
    buf = b.pack()
    assert buf.size == sum(x.size for x in b.Psi_cores + b.Omega_mats)
    r = a.unpack(buf)
    assert all(np.array_equal(x, y) for x, y in zip(r.Psi_cores + r.Omega_mats,
                                                     b.Psi_cores + b.Omega_mats))


def test_no_cpu_fallback_without_gpu():
    """On a box without a GPU every compute entry point must raise, never fall back."""
    import tt_sketch_amd as tsa
    lib = nat.lib()
    if lib.ttsk_init(0) == 0:
        pytest.skip("a GPU is present")
    X = tsa.TensorTrain.random((4, 5, 6), 2, seed=1)
    with pytest.raises(nat.TtskError):
        tsa.stream_sketch(X, 2, 3, seed=1)


def test_read_tns(tmp_path):
    """FROSTT text format (reference scripts/frostt.py:51-65): 1-based indices, value last."""
    import gzip
    from tt_sketch_amd.io import read_tns
    text = "# comment\n1 2 3 0.5\n4 1 2 -1.25\n\n2 2 2 3e-2\n"
    p = tmp_path / "t.tns"
    p.write_text(text)
    T = read_tns(str(p))
    assert T.shape == (4, 2, 3) and T.indices.shape == (3, 3)
    assert np.array_equal(T.indices, np.array([[0, 3, 1], [1, 0, 1], [2, 1, 1]]))
    assert np.allclose(T.entries, [0.5, -1.25, 0.03])
    g = tmp_path / "t.tns.gz"
    with gzip.open(g, "wb") as f:
        f.write(text.encode())
    T2 = read_tns(str(g), shape=(5, 5, 5))
    assert T2.shape == (5, 5, 5) and np.array_equal(T2.indices, T.indices)
    with pytest.raises(ValueError):
        read_tns(str(p), shape=(2, 2, 2))
    bad = tmp_path / "bad.tns"
    bad.write_text("1 2 3 0.5\n1 2 0.5\n")
    with pytest.raises(ValueError):
        read_tns(str(bad))
    zero = tmp_path / "zero.tns"
    zero.write_text("0 1 1 1.0\n")
    with pytest.raises(ValueError):
        read_tns(str(zero))


def test_pool_reuse_is_stream_ordered():
    """device.py hands a released buffer out again only to the same stream, or after every stream that
    may still be touching it has been drained (cross-stream reuse)."""
    from tt_sketch_amd import device
    saved = (set(nat._dirty), list(nat._stream_gen))
    saved_join = dict(nat._joined_into)
    try:
        nat._dirty.clear()
        nat._joined_into.clear()
        nat._mark("ttsk_axpby", (None, None, 1.0, 1.0, 0, 0))        # work on stream 0 only
        tag0 = nat.dirty_snapshot()
        assert set(tag0) == {0}
        assert device._reusable(tag0, 0) and not device._reusable(tag0, 3)
        nat._mark("ttsk_gemm", (None, None, None, None, None, 3))    # a multi-stream region opens
        nat._mark("ttsk_tt_sketch", (None,) * 14 + (4,))             # forks a helper on stream 5, joined back into 4
        assert nat._dirty >= {0, 3, 4, 5}
        tag = nat.dirty_snapshot()
        assert set(tag) == {0, 3, 4}                                 # the joined helper counts as its caller's stream
        assert not any(device._reusable(tag, s) for s in range(nat.NUM_STREAMS))
        nat._stream_gen[3] += 1                                      # as ttsk_sync(3) does
        nat._dirty.discard(3)
        assert not device._reusable(tag, 0)
        for s in range(nat.NUM_STREAMS):                             # as ttsk_sync(-1) does
            nat._stream_gen[s] += 1
        nat._dirty.clear()
        assert all(device._reusable(tag, s) for s in range(nat.NUM_STREAMS))
        assert device._size_class(100) == 256 and device._size_class(9 << 20) == 10 << 20
    finally:
        nat._dirty.clear()
        nat._dirty.update(saved[0])
        nat._stream_gen[:] = saved[1]
        nat._joined_into.clear()
        nat._joined_into.update(saved_join)


def test_helper_stream_of_a_one_call_sketch_is_drained_with_its_caller():
    """ttsk_tt_sketch* fork stream + 1 and join it back; a blocking read / sync of the CALLER's stream must
    release buffers tagged with the helper too (they used to wait for a device-wide sync), but not if something else
    was queued on the helper directly."""
    from tt_sketch_amd import _native as nat
    saved = (set(nat._dirty), list(nat._stream_gen), dict(nat._joined_into))
    try:
        nat._dirty.clear(); nat._joined_into.clear()
        nat._mark("ttsk_tt_sketch_batch", (1, 2, 3, 0))          # last argument: stream 0 -> helper 1
        assert nat._dirty == {0, 1}
        tag = nat.dirty_snapshot()
        nat._drained(0)                                          # what ttsk_d2h(..., 0) / ttsk_sync(0) do
        assert nat._dirty == set() and all(nat.drained_since(s, g) for s, g in tag.items())
        nat._mark("ttsk_tt_sketch", (0,))
        nat._mark("ttsk_gemm", (1,))                             # independent work on the helper stream
        tag = nat.dirty_snapshot()
        nat._drained(0)
        assert nat._dirty == {1} and not nat.drained_since(1, tag[1])
    finally:
        nat._dirty.clear(); nat._dirty.update(saved[0])
        nat._stream_gen[:] = saved[1]
        nat._joined_into.clear(); nat._joined_into.update(saved[2])


# ------------------------------------------------------------------ _native.ENTRY_POINTS against include/ttsk.h
_C_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64,
              "double": ctypes.c_double, "float": ctypes.c_float}
_C_RETURNS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "const char *": ctypes.c_char_p}
# entry points that end in `int stream` and neither queue work on it nor drain it
_STREAM_LAST_WITHOUT_ROLE = {
    "ttsk_graph_begin": "opens a capture: nothing runs on the stream until ttsk_graph_launch, which is marked",
}


def _header_text():
    with open(nat.HEADER_PATH) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def _header_declarations():
    """{name: (return type, [(type, name, is pointer), ...])} of every function include/ttsk.h declares."""
    out = {}
    for ret, name, params in re.findall(r"^[ \t]*((?:const\s+)?\w+\s*\*?)\s*(ttsk_\w+)\s*\(([^()]*)\)\s*;", _header_text(), flags=re.M):
        plist = []
        for p in ([] if params.strip() in ("", "void") else params.split(",")):
            words = p.replace("*", " * ").split()
            pname = words.pop()
            plist.append((" ".join(w for w in words if w != "const"), pname, "*" in words))
        out[name] = (" ".join(ret.replace("*", " *").split()), plist)
    return out


def _is_pointer_type(t) -> bool:
    return t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer)


def _ends_in_stream(params) -> bool:
    return bool(params) and params[-1][:2] == ("int", "stream")


def _roles_missing(has_role) -> list:
    """Functions of the header that end in `int stream` for which ``has_role(name)`` is false, the stated exceptions aside."""
    return sorted(name for name, (_, params) in _header_declarations().items()
                  if _ends_in_stream(params) and not has_role(name) and name not in _STREAM_LAST_WITHOUT_ROLE)


def test_entry_point_table_matches_the_header_types():
    decls = _header_declarations()
    assert sorted(decls) == nat.declared_symbols() == sorted(nat.ENTRY_POINTS)
    for name, (ret, params) in decls.items():
        e = nat.ENTRY_POINTS[name]
        assert e.restype is _C_RETURNS[ret], name
        assert len(e.argtypes) == len(params), name
        for i, ((ctype, pname, is_ptr), t) in enumerate(zip(params, e.argtypes)):
            assert _is_pointer_type(t) == is_ptr, (name, i, pname)
            if not is_ptr:
                assert t is _C_SCALARS[ctype], (name, i, pname)


def test_entry_point_table_matches_the_header_constants():
    text = _header_text()
    assert nat.NUM_STREAMS == int(re.search(r"#define\s+TTSK_NUM_STREAMS\s+(\d+)", text).group(1))
    status = {k: int(v) for k, v in re.findall(r"\b(TTSK_ERR_\w+)\s*=\s*(-?\d+)", text)}
    mine = {k: v for k, v in vars(nat).items() if k.startswith("TTSK_ERR_")}
    assert mine and all(status[k] == v for k, v in mine.items())


def test_every_stream_argument_has_a_role():
    """A queued entry point that is not marked leaves its stream out of the tag of a released buffer: the pool of
    device.py would hand the buffer to another stream while the kernel still reads it."""
    decls = _header_declarations()
    queueing = (nat.QUEUE, nat.FORK_NEXT, nat.FORK_ALL)
    assert _roles_missing(lambda name: nat.ENTRY_POINTS[name].role is not None) == []
    assert set(_STREAM_LAST_WITHOUT_ROLE) <= set(decls)
    for name, e in nat.ENTRY_POINTS.items():
        params = decls[name][1]
        assert e.role in queueing + (nat.DRAIN_FIRST, nat.DRAIN_LAST, None), name
        if e.role in queueing or e.role == nat.DRAIN_LAST:
            assert _ends_in_stream(params), name
        if e.role == nat.DRAIN_FIRST:
            assert params[0][:2] == ("int", "stream"), name


def test_mark_records_the_streams_of_every_queueing_entry_point():
    saved = (set(nat._dirty), list(nat._stream_gen), dict(nat._joined_into))
    try:
        for name, e in nat.ENTRY_POINTS.items():
            nat._dirty.clear(); nat._joined_into.clear()
            nat._mark(name, (None,) * (len(e.argtypes) - 1) + (3,))
            want = {nat.QUEUE: {3}, nat.FORK_NEXT: {3, 4}, nat.FORK_ALL: set(range(nat.NUM_STREAMS))}.get(e.role, set())
            assert nat._dirty == want, name
    finally:
        nat._dirty.clear(); nat._dirty.update(saved[0])
        nat._stream_gen[:] = saved[1]
        nat._joined_into.clear(); nat._joined_into.update(saved[2])


def _rdv_worker(rank, world, directory, out):
    from tt_sketch_amd.rendezvous import FileRendezvous
    r = FileRendezvous(rank, world, directory=directory, timeout=30)
    got = r.broadcast(b"\x01" * 128 if rank == 0 else None)
    parts = r.allgather(bytes([rank]) * 3)
    r.barrier()
    r.close()
    out.put((rank, got == b"\x01" * 128, parts == [bytes([k]) * 3 for k in range(world)]))


def test_file_rendezvous_carries_the_id_between_processes(tmp_path):
    """The torch-free exchange of the 128-byte RCCL id (bench.py, RcclComm.from_env)."""
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rdv_worker, args=(r, 3, str(tmp_path / "rdv"), q)) for r in range(3)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=60) for _ in procs)
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    assert res == [(0, True, True), (1, True, True), (2, True, True)]


def test_file_rendezvous_ignores_the_leftovers_of_a_crashed_launch(tmp_path):
    """a directory that still holds an earlier launch's files (crashed before close(), or a fixed
    TTSK_RDV_DIR): the new launch must neither read the stale NCCL id nor a stale gather piece, and the directory is
    gone after a clean close."""
    import multiprocessing as mp
    import os
    d = tmp_path / "rdv"
    d.mkdir()
    # what a launch of the old naming scheme and a crashed launch of the new one leave behind
    (d / "000001_bcast.0").write_bytes(b"\x07" * 128)
    (d / "000002_gather.1").write_bytes(b"stale")
    (d / "hello.0").write_bytes(b"deadbeefdeadbeef")
    (d / "hello.1").write_bytes(b"0123456789abcdef")
    (d / "hello.2").write_bytes(b"fedcba9876543210")
    (d / "session").write_bytes(b"aaaaaaaaaaaaaaaa deadbeefdeadbeef 0123456789abcdef fedcba9876543210")
    (d / "ack.1").write_bytes(b"aaaaaaaaaaaaaaaa deadbeefdeadbeef 0123456789abcdef fedcba9876543210")
    (d / "aaaaaaaaaaaaaaaa_000001_bcast.0").write_bytes(b"\x09" * 128)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rdv_worker, args=(r, 3, str(d), q)) for r in range(3)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=60) for _ in procs)
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    assert res == [(0, True, True), (1, True, True), (2, True, True)]
    assert not os.path.exists(d)              # the last rank out removed it, leftovers included


def test_failed_comm_init_leaves_the_process_exit_clean():
    """ttsk_comm_init with a bad rank / without a device returns an error code, leaves no
    communicator behind (destroy is a no-op, init can be called again) and the interpreter exits 0
    (round 1: the only N = 2 run died in `double free or corruption` after a failed init)."""
    import subprocess
    import sys
    code = r"""
import ctypes, sys
sys.path.insert(0, %r)
from tt_sketch_amd import _native as nat
lib = nat.lib()
uid = (ctypes.c_char * 128)()
rcs = [lib.ttsk_comm_init(uid, 5, 2), lib.ttsk_comm_init(uid, -1, 2), lib.ttsk_comm_init(None, 0, 1)]
assert all(rc != 0 for rc in rcs), rcs
assert lib.ttsk_comm_destroy() == 0
assert lib.ttsk_comm_allreduce_sum(None, 4, 0) != 0          # no communicator: an error, not a crash
assert lib.ttsk_comm_init(uid, 7, 3) != 0 and lib.ttsk_comm_destroy() == 0
print("clean")
""" % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    assert "clean" in out.stdout


def test_test_tensor_generators():
    """hilbert_tensor / sqrt_tensor (reference utils.py:20-39) from their definitions, incl. the swapped first two
    modes of sqrt_tensor (np.meshgrid's 'xy' default in the reference)."""
    from tt_sketch_amd import utils
    H = utils.hilbert_tensor(3, 4)
    i, j, k = np.ogrid[:4, :4, :4]
    assert H.shape == (4, 4, 4) and np.array_equal(H, 1.0 / (i + j + k + 1.0))
    S = utils.sqrt_tensor((3, 4, 5), a=0.5, b=3)
    assert S.shape == (4, 3, 5) and abs(np.linalg.norm(S) - 1) < 1e-14
    t = [np.linspace(0.5, 3, n) for n in (4, 3, 5)]
    want = np.sqrt(np.abs(t[0][:, None, None] + t[1][None, :, None] + t[2][None, None, :]))
    assert np.allclose(S, want / np.linalg.norm(want), rtol=1e-15, atol=0)
    assert utils.sqrt_tensor((7,)).shape == (7,)


def test_public_names_of_the_reference_are_present():
    """The reference's public names on and around the path (modules sketch, sketch_dispatch, drm, drm_base, tensor,
    utils, sketch_container, tt_svd, tt_gmres; listed from its sources) exist under the same module paths."""
    import importlib
    expected = {
        "sketch": ["stream_sketch", "orthogonal_sketch", "hmt_sketch", "blocked_stream_sketch", "assemble_sketched_tt",
                   "SketchedTensorTrain"],
        "sketch_dispatch": ["general_sketch", "SketchMethod", "get_sketch_method", "orth_step", "OrthogTTDRM", "sum_sketch",
                            "sketch_omega_sum", "sketch_psi_sum", "OMEGA_METHODS", "PSI_METHODS",
                            "DRM_SKETCH_METHOD_DISPATCH"],
        "sketch_container": ["SketchContainer"],
        "drm": ["ALL_DRM", "DenseGaussianDRM", "SparseGaussianDRM", "SparseSignDRM", "TensorTrainDRM"],
        "drm.fast_lazy_gaussian": ["hash_int_c", "_inds_to_rand_double", "inds_to_normal", "inds_to_sparse_sign"],
        "drm_base": ["DRM", "CanSlice", "CanIncreaseRank", "handle_transpose"],
        "tensor": ["Tensor", "DenseTensor", "SparseTensor", "TensorTrain", "CPTensor", "TuckerTensor", "TensorSum"],
        "utils": ["hilbert_tensor", "sqrt_tensor", "power_decay_tensor", "matricize", "dematricize", "right_mul_pinv",
                  "left_mul_pinv", "projector", "trim_ranks", "process_tt_rank", "random_normal"],
        "tt_svd": ["tt_svd"],
        "tt_gmres": ["TTLinearMap", "MPO", "TTPrecond", "TTLinearMapSum", "round_tt_sum", "tt_sum_gmres"],
        "sketching_methods.abstract_methods": ["CansketchSparse", "CansketchTT", "CansketchCP", "CansketchDense",
                                               "CanSketchTucker"],
    }
    for mod, names in expected.items():
        m = importlib.import_module("tt_sketch_amd." + mod)
        missing = [n for n in names if not hasattr(m, n)]
        assert not missing, (mod, missing)
    from tt_sketch_amd.sketch import SketchedTensorTrain
    for attr in ("left_rank", "right_rank", "Psi_cores", "Omega_mats", "C_cores", "T", "to_tt", "to_numpy", "increase_rank",
                 "error", "dense"):
        assert hasattr(SketchedTensorTrain, attr), attr


def test_shard_bounds_cover_everything():
    from tt_sketch_amd.distributed import shard_bounds
    for n in (0, 1, 5, 32, 33):
        for world in (1, 2, 3, 8):
            spans = [shard_bounds(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1


def test_sparse_one_pass_path_declines_a_mode_beyond_its_sort_key():
    """The mode-order sort key of the one-pass sparse path holds the mode index in 24 bits (ttsk_sparse_mode_order): a
    longer mode is declined BEFORE anything touches the device, so that the panel path takes over."""
    from tt_sketch_amd import SparseGaussianDRM, SparseTensor, sparse_fused
    from tt_sketch_amd.sketch_dispatch import SketchMethod
    shape = (5, (1 << 24) + 1, 4)
    idx = np.array([[0, 1], [3, (1 << 24)], [2, 1]])
    X = SparseTensor(shape, idx, np.array([1.0, -2.0]))
    left = SparseGaussianDRM((2, 2), shape, transpose=False, seed=1)
    right = SparseGaussianDRM((3, 3), shape, transpose=True, seed=2)
    assert sparse_fused.try_sparse_gauss_sketch(X, left, right, SketchMethod.streaming) is None


def test_every_launch_goes_through_the_one_checked_helper():
    """csrc/common.h launch() is the library's only kernel launch and runtime.hip's registry its only dynamic-LDS set-up:
    a kernel added with a local idiom (its own hipFuncSetAttribute, a per-function once-flag) fails here."""
    import glob
    import re
    csrc = os.path.join(os.path.dirname(nat.__file__), "csrc")
    src = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))}
    assert len(src) > 40
    where = lambda pat: sorted(f for f, s in src.items() if re.search(pat, s))
    assert where(r"\bhipLaunchKernelGGL\b") == ["common.h"]
    assert where(r"\bhipFuncSetAttribute\b") == ["runtime.hip"]
    assert where(r"\bPerInit\b") == []
    assert where(r"static\s+bool\s+attr_done") == []
    assert where(r"\bTTSK_LAUNCH_CHECK\b") == []


def test_each_solver_decision_has_one_definition():
    """common.h's builders are the only place a ttsk_gemm_desc is filled (gemm_plan.h holds one as a launch argument), the
    normal-equations pseudo-inverse is one list of stages (no TTSK_PB macros per entry point), the sign reconstruction of one
    matrix is the batched kernel's, and linalg.hip is split by solver."""
    import glob
    import re
    csrc = os.path.join(os.path.dirname(nat.__file__), "csrc")
    src = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))}
    where = lambda pat: sorted(f for f, s in src.items() if re.search(pat, s))
    assert where(r"\bttsk_gemm_desc\s+\w+\s*(\{\s*\}|;)") == ["common.h", "gemm_plan.h"]
    assert where(r"\bTTSK_PB\b") == []
    assert where(r"\bqr_signs_kernel\b") == []
    assert "linalg.hip" not in src and {"jacobi.hip", "householder.hip", "cholesky.hip", "pinv.hip"} <= set(src)


def test_each_path_decision_has_one_definition():
    """paths.py is the only place that asks whether a DRM is a rank slice or validates a route; the module switch of
    tt_gram is gone; and no fused module imports SketchMethod inside a function (sketch_dispatch and they no longer import
    each other for it)."""
    import glob
    import re
    import tt_sketch_amd
    from tt_sketch_amd import paths, sketch_dispatch
    pkg = os.path.dirname(nat.__file__)
    src = {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(pkg, "*.py"))}
    where = lambda pat: sorted(f for f, s in src.items() if re.search(pat, s))
    # "is this a rank slice": rank_min compared with the zeros, rank_max with true_rank
    slice_test = r"rank_min\)?\s*[!=]=|rank_max\)?\s*[!=]=\s*(tuple\()?[\w.]*true_rank"
    assert re.search(slice_test, "tuple(m.rank_min) != (0,) * (d - 1)") and re.search(slice_test, "m.rank_max == m.true_rank")
    assert where(slice_test) == ["paths.py"]
    assert where(r"'kernel', 'composed' or None") == ["paths.py"]
    assert where(r"_GRAM_ROUTE") == []
    for f in ("tt_fused.py", "cp_fused.py", "operator_fused.py", "sparse_fused.py"):
        assert not re.search(r"^[ \t]+from [.\w]+ import .*\bSketchMethod\b", src[f], re.M), f
        assert re.search(r"^from \.paths import .*\bSketchMethod\b", src[f], re.M), f
    assert sketch_dispatch.SketchMethod is paths.SketchMethod is tt_sketch_amd.SketchMethod
    imported = set(re.findall(r"^\s*from \.(\w+)", src["paths.py"], re.M))
    for names in re.findall(r"^\s*from \. import (.+)$", src["paths.py"], re.M):
        imported |= {n.split()[0] for n in names.split(",")}
    assert not imported & {"sketch_dispatch", "sketch", "tt_fused", "cp_fused", "operator_fused", "sparse_fused"}, imported


def _outside_lab_blocks(text):
    """text with every line inside `#ifdef TTSK_LAB` ... (`#else` | `#endif`) blanked: what the shipped library compiles."""
    import re
    out, stack = [], []                  # one entry per open #if: True while inside the lab branch of a TTSK_LAB test
    for line in text.splitlines():
        d = line.strip()
        if re.match(r"#\s*if", d):
            stack.append(bool(re.match(r"#\s*(ifdef\s+TTSK_LAB\b|if\s+defined\s*\(?\s*TTSK_LAB\b)", d)))
        elif re.match(r"#\s*(else|elif)", d) and stack:
            stack[-1] = False
        elif re.match(r"#\s*endif", d) and stack:
            stack.pop()
        out.append("" if any(stack) else line)
    return "\n".join(out)


def test_shipped_library_reads_no_ab_switches():
    """The A/B switches of libttsk were folded to their defaults: outside the lab build (-DTTSK_LAB) the only environment
    variables csrc/ reads are TTSK_SINGLE_STREAM (bench.py's roofline pass) and TTSK_GEMM_TRACE (prints only)."""
    import glob
    import re
    csrc = os.path.join(os.path.dirname(nat.__file__), "csrc")
    calls, named = [], []
    for p in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")):
        text = _outside_lab_blocks(open(p).read())
        calls += re.findall(r"\bgetenv\s*\(", text)
        named += re.findall(r"\bgetenv\s*\(\s*\"(\w+)\"\s*\)", text)
    assert len(named) == len(calls) >= 2          # every read names its variable literally
    assert set(named) == {"TTSK_SINGLE_STREAM", "TTSK_GEMM_TRACE"}, sorted(set(named))


def test_sparse_pass_configurations_reach_every_instantiation():
    """tests/test_gpu_sparse_pass.py runs the configurations of tests/sparse_cases.py; sparse_cases.instantiation restates how
    sg_plan (csrc/sparse_plan.h) chooses among the seven instantiations of sg_pass_kernel (csrc/sparse_pass.h;
    tests/test_sparse_plan.py holds the restatement against the plan).  Every one of them is
    reached, and the configurations the design document names for each land where it says."""
    from tests import sparse_cases as sc
    reached = {}
    for cfg in sc.CONFIGS:
        reached.setdefault(sc.instantiation(cfg), []).append(cfg.name)
    assert set(reached) == set(sc.INSTANTIATIONS), sorted(reached)
    by_name = {cfg.name: sc.instantiation(cfg) for cfg in sc.CONFIGS}
    assert len(by_name) == len(sc.CONFIGS)             # the names are the test ids: no two alike
    assert by_name["t16-16-16-both-left"] == (1, 0, 32)
    assert by_name["t16-32-16-both-left"] == (2, 0, 32) and by_name["sign32-B-nnz1"] == (2, 0, 32)      # NT = 2 from the sign row alone
    assert by_name["t20-20-20-both-left"] == (2, 1, 32) and by_name["t17-4-9-both-right"] == (2, 1, 32)
    assert by_name["t5-21-1-both-left"] == (2, 2, 32) and by_name["t24-24-24-both-noC"] == (2, 2, 32)
    assert by_name["t32-32-8-both-left"] == (2, 0, 16) and by_name["t32-32-32-both-right"] == (2, 0, 16)
    assert by_name["normal20"] == (2, 1, 16)
    assert by_name["t24-24-24-both-left"] == (2, 2, 16)
    # (32, 32, 8) is just over the threshold of the 16-record tile: one table column pair less keeps 32
    assert sc.instantiation(sc.table_config((32, 32, 6), "both", "left")) == (2, 0, 32)
