"""ctypes binding of libttsk.so (the C ABI declared in include/ttsk.h).

The product path has no CPU fallback: if the HIP library is missing or no
device is present every compute entry point raises.
"""
import ctypes
import os
import re
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_uint64, c_void_p
from typing import NamedTuple, Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TTSK_LIB") or os.path.join(_HERE, "libttsk.so")      # TTSK_LIB: another build of the library (A/B runs)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "ttsk.h")

TTSK_ERR_ARG = -2
TTSK_ERR_UNSUPPORTED = -3
NUM_STREAMS = 8


class TtskError(RuntimeError):
    """A HIP / RCCL level failure inside libttsk."""


class TtskUnsupported(TtskError):
    """The fused kernel does not cover this shape (caller composes from ttsk_gemm)."""


class GemmDesc(Structure):
    _fields_ = [(n, c_int64) for n in
                ("batch", "M", "N", "Ko", "Ki", "a_b", "a_m", "a_ko", "a_ki",
                 "b_b", "b_ko", "b_ki", "b_n", "c_b", "c_m", "c_n")] + [
        ("alpha", c_double), ("accumulate", c_int), ("split_k", c_int)]


_lib = None


def declared_symbols():
    """Every function name include/ttsk.h declares."""
    with open(HEADER_PATH) as f:
        text = f.read()
    return sorted(set(re.findall(r"\b(ttsk_[a-z0-9_]+)\s*\(", text)))


# Stream role of an entry point: what a call does to the library streams, which is what the buffer pool of device.py
# needs to know to hand a released buffer out again (dirty_snapshot / drained_since below).
QUEUE = "queue"              # queues work on the library stream given as the LAST argument
FORK_NEXT = "queue, +1"      # the same, and forks a helper on stream + 1 that is joined back before the call returns
FORK_ALL = "queue, all"      # the same, and forks every other library stream, all joined back
DRAIN_FIRST = "drain first"  # returns only after the stream given as the FIRST argument has drained (negative: all of them)
DRAIN_LAST = "drain last"    # the same for the stream given as the last argument
_QUEUEING = (QUEUE, FORK_NEXT, FORK_ALL)


class Entry(NamedTuple):
    argtypes: list
    role: Optional[str] = None     # None: queues no work
    restype: type = c_int          # a ttsk_status unless stated


P, I, S, I64, U64 = c_void_p, c_int, c_size_t, c_int64, c_uint64
_CHAIN = [I, I, I, I, I, I, POINTER(P), I64, POINTER(P), I64, I64, I64, I64, P]       # ttsk_chain_step*: up to E
_MODE_STREAM = [P, I64, P, S, POINTER(I), POINTER(U64), I, POINTER(I), POINTER(U64), I, I, P, P, P, P, P, I]
_GAUSS_PASS = [P, P, P, P, S, I64, P, P, P, I, P, P, I]
# Every function of include/ttsk.h, one line each: argument types, stream role, return type.  This is the only place an
# entry point is described; tests/test_host_logic.py holds it against the header.
ENTRY_POINTS = {
    "ttsk_init": Entry([I]),
    "ttsk_shutdown": Entry([]),
    "ttsk_last_error": Entry([], restype=c_char_p),
    "ttsk_device_info": Entry([c_char_p, S, POINTER(I), POINTER(S)]),
    "ttsk_malloc": Entry([POINTER(P), S]),
    "ttsk_free": Entry([P]),
    "ttsk_memset": Entry([P, I, S, I], QUEUE),
    "ttsk_h2d": Entry([P, P, S, I], DRAIN_LAST),
    "ttsk_d2h": Entry([P, P, S, I], DRAIN_LAST),
    "ttsk_d2d": Entry([P, P, S, I], QUEUE),
    "ttsk_sync": Entry([I], DRAIN_FIRST),
    "ttsk_stream_wait": Entry([I, I]),
    "ttsk_timer_start": Entry([I], QUEUE),
    "ttsk_timer_stop": Entry([I, POINTER(c_float)]),
    "ttsk_graph_begin": Entry([I]),
    "ttsk_graph_end": Entry([I, POINTER(P)]),
    "ttsk_graph_launch": Entry([P, I], QUEUE),
    "ttsk_graph_free": Entry([P]),
    "ttsk_gemm": Entry([POINTER(GemmDesc), P, P, P, P, I], QUEUE),
    "ttsk_copy_strided": Entry([P, P, I, POINTER(I64), POINTER(I64), POINTER(I64), I], QUEUE),
    "ttsk_axpby": Entry([P, P, c_double, c_double, S, I], QUEUE),
    "ttsk_sum_slices": Entry([P, P, I, S, S, I, I], QUEUE),
    "ttsk_tt_sketch": Entry([I] + [POINTER(I64)] * 8 + [POINTER(P)] * 3 + [P, I, I], FORK_NEXT),
    "ttsk_tt_sketch_batch": Entry([I, I] + [POINTER(I64)] * 8 + [POINTER(P)] * 3 + [P, I64, I, I], FORK_NEXT),
    "ttsk_tt_sketch_sum": Entry([I, I] + [POINTER(I64)] * 8 + [POINTER(P)] * 3 + [P, I, I], FORK_NEXT),
    "ttsk_tt_sketch_split": Entry([I, I, I]),
    "ttsk_chain_step": Entry(_CHAIN + [POINTER(P), POINTER(P), I], QUEUE),
    "ttsk_chain_step_wide": Entry(_CHAIN + [POINTER(P), POINTER(P), I], QUEUE),
    "ttsk_chain_step_sum": Entry(_CHAIN + [P, I64, I64, I64, POINTER(P), I], QUEUE),
    "ttsk_psi_stream": Entry([I, I, I, I, POINTER(P), I64, POINTER(P), I64, POINTER(P), I64, I, I], QUEUE),
    "ttsk_psi_stream_sum": Entry([I, I, I, I, P, I64, I64, P, I64, I64, P, I64, I, I], QUEUE),
    "ttsk_drm_pack": Entry([P, I, I, I, I], DRAIN_LAST),
    "ttsk_drm_unpack": Entry([P]),
    "ttsk_dense_left_pass": Entry([P, I64, I64, I64, I64, I64, I, P, P, P, P, P, P, P, P, I], QUEUE),
    "ttsk_tt_sketch_size": Entry([I] + [POINTER(I64)] * 5, restype=I64),
    "ttsk_prof_enable": Entry([I]),
    "ttsk_mfma_f64_peak_probe": Entry([POINTER(c_double)]),
    "ttsk_ndtri_rate_probe": Entry([POINTER(c_double)]),
    "ttsk_prof_read": Entry([I, POINTER(I64), POINTER(c_double), POINTER(c_double)]),
    "ttsk_prof_kernel_name": Entry([I, c_char_p, S]),
    "ttsk_hash_u64": Entry([P, S]),
    "ttsk_inds_to_rand_double": Entry([P, P, I, S, I, I, U64, P]),
    "ttsk_inds_to_normal": Entry([P, P, I, S, I, I, U64, P]),
    "ttsk_inds_to_sparse_sign": Entry([P, P, I, S, I, I, I, I, U64, P]),
    "ttsk_sparse_normal_dev": Entry([P, I64, POINTER(I), POINTER(U64), I, S, I, I, U64, P, I], QUEUE),
    "ttsk_sparse_normal_table": Entry([POINTER(U64), I, I, I, U64, P, I], QUEUE),
    "ttsk_sparse_sign_dev": Entry([P, I64, POINTER(I), POINTER(U64), I, S, I, I, I, I, U64, P, I], QUEUE),
    "ttsk_sparse_sign_table": Entry([POINTER(U64), I, I, I, I, I, U64, P, I], QUEUE),
    "ttsk_fill_normal": Entry([P, S, U64, c_double, I], QUEUE),
    "ttsk_fill_normal_many": Entry([I, POINTER(P), POINTER(S), POINTER(U64), POINTER(c_double), I], QUEUE),
    "ttsk_gauss_lazy_left": Entry([U64, I64, I64, I64, P, I64, I64, P, I64, I], QUEUE),
    "ttsk_gauss_lazy_right": Entry([U64, I64, I64, I64, P, I64, I64, P, I64, I], QUEUE),
    "ttsk_sparse_ttdrm_step": Entry([P, I64, P, I64, I64, P, S, P, I], QUEUE),
    "ttsk_kr_rows": Entry([P, I64, P, I64, I64, P, I], QUEUE),
    "ttsk_kr_step": Entry([P, P, I64, I64, P, S, P, I], QUEUE),
    "ttsk_sparse_densedrm_gather": Entry([P, I64, I64, P, I64, POINTER(I), POINTER(I64), I, S, P, I], QUEUE),
    "ttsk_sparse_psi": Entry([P, P, P, S, P, I64, P, I64, I64, P, I], QUEUE),
    "ttsk_tt_gather": Entry([POINTER(P), POINTER(I64), POINTER(I64), I, P, I64, POINTER(I), S, P, P, P, I], QUEUE),
    "ttsk_cp_gather": Entry([POINTER(P), I64, POINTER(I64), I, P, I64, POINTER(I), S, P, P, P, I], QUEUE),
    "ttsk_tucker_gather": Entry([P, POINTER(P), POINTER(I64), POINTER(I64), I, P, I64, POINTER(I), S, P, P, P, I], QUEUE),
    "ttsk_sparse_key_index": Entry([POINTER(I64), I, P, I64, POINTER(I), S, P, I, P, P, P, I], QUEUE),
    "ttsk_sparse_join": Entry([P, P, P, S, I, POINTER(I64), I, P, I64, POINTER(I), S, P, P, P, I], QUEUE),
    "ttsk_dense_join": Entry([P, POINTER(I64), I, P, I64, POINTER(I), S, P, P, P, I], QUEUE),
    "ttsk_sparse_join_layout": Entry([S, S, I, POINTER(I64)]),
    "ttsk_tt_gram": Entry([POINTER(P), POINTER(I64), I, POINTER(P), POINTER(I64), I, POINTER(I64), I, P, I], QUEUE),
    "ttsk_gram_round_bonds": Entry([POINTER(P), POINTER(P), POINTER(I64), POINTER(I64), I, c_double, POINTER(P), POINTER(P), POINTER(P), P, I], QUEUE),
    "ttsk_op_apply": Entry([I, POINTER(P), POINTER(P), POINTER(P), POINTER(I64), POINTER(I64), I64, P, I64, I], QUEUE),
    "ttsk_hadamard_apply": Entry([P, P, P, POINTER(I64), POINTER(I64), P, I64, I64, I], QUEUE),
    "ttsk_hadamard_close": Entry([P, P, P, POINTER(I64), POINTER(I64), P, I, P, I64, I], QUEUE),
    "ttsk_hadamard_close_layout": Entry([POINTER(I64), POINTER(I64)]),
    "ttsk_op_close": Entry([P, P, P, POINTER(I64), POINTER(I64), P, I, P, I64, I], QUEUE),
    "ttsk_op_close_layout": Entry([POINTER(I64), POINTER(I64)]),
    "ttsk_op_close_batch": Entry([I, POINTER(P), POINTER(P), POINTER(P), POINTER(I64), POINTER(I64), POINTER(I64), POINTER(P), I, P, I64, I], QUEUE),
    "ttsk_op_close_batch_layout": Entry([I, POINTER(I64), POINTER(I64)]),
    "ttsk_cp_chain_step": Entry([P, I64, P, I64, I64, P, P, I64, I64, I64, I64, I64, I], QUEUE),
    "ttsk_cp_psi_omega": Entry([P, I64, P, I64, P, I64, I64, P, P, I64, I64, P, I64, I64, I64, I64, I], QUEUE),
    "ttsk_cp_gram": Entry([POINTER(P), POINTER(I64), I64, POINTER(P), POINTER(I64), I64, POINTER(I64), I, I, P, I], QUEUE),
    "ttsk_sum": Entry([P, S, P, I], QUEUE),
    "ttsk_tt_dense_stats": Entry([P, I64, P, I64, I64, P, P, P, I], QUEUE),
    "ttsk_tt_dense_stats_ld": Entry([P, I64, P, I64, I64, P, I64, P, I64, P, I, I], QUEUE),
    "ttsk_sumsq": Entry([P, S, P, I], QUEUE),
    "ttsk_sparse_flat_mult": Entry([POINTER(U64), I, POINTER(U64)]),
    "ttsk_sparse_mode_order": Entry([P, I64, S, POINTER(I), POINTER(U64), I, I, I64, P, I], QUEUE),
    "ttsk_sparse_mode_stream": Entry(_MODE_STREAM, QUEUE),
    "ttsk_sparse_mode_stream_u32": Entry(_MODE_STREAM, QUEUE),
    "ttsk_sparse_gauss_pass": Entry(_GAUSS_PASS, QUEUE),
    "ttsk_sparse_gauss_pass_u32": Entry(_GAUSS_PASS, QUEUE),
    "ttsk_sparse_sort_mode": Entry([P, S, I64, P, I], QUEUE),
    "ttsk_pinv": Entry([P, I64, I64, c_double, P, POINTER(I), I], QUEUE),
    "ttsk_pinv_begin": Entry([P, I64, I64, c_double, P, I], QUEUE),
    "ttsk_pinv_end": Entry([P, I64, I64, c_double, P, POINTER(I), I], QUEUE),
    "ttsk_svd_small": Entry([P, I64, I64, P, P, P, I], QUEUE),
    "ttsk_triu": Entry([P, I64, I64, I], QUEUE),
    "ttsk_qr_thin": Entry([P, I64, I64, I], QUEUE),
    "ttsk_orth_step": Entry([P, I64, I64, P, I64, P, I], QUEUE),
    "ttsk_pinv_batch_deferred": Entry([I, POINTER(P), I64, I64, POINTER(P), I], QUEUE),
    "ttsk_orth_step_pinv": Entry([P, I64, I64, P, I64, P, I], QUEUE),
    "ttsk_deferred_status": Entry([I, POINTER(I)], DRAIN_FIRST),
    "ttsk_tt_orth_sketch": Entry([I] + [POINTER(I64)] * 4 + [POINTER(P)] * 5 + [I], FORK_NEXT),
    "ttsk_tt_orth_sketch_batch": Entry([I, I] + [POINTER(I64)] * 4 + [POINTER(P)] * 5 + [P, I], FORK_ALL),
    "ttsk_dense_first_pass": Entry([P, I64, I64, I64, P, I64, P, I64, P, P, I], QUEUE),
    "ttsk_pinv_batch": Entry([I, POINTER(P), I64, I64, POINTER(P), I], QUEUE),
    "ttsk_tt_assemble": Entry([I] + [POINTER(I64)] * 3 + [POINTER(P)] * 4 + [I, I], FORK_ALL),
    "ttsk_tt_assemble_batch": Entry([I, I] + [POINTER(I64)] * 3 + [POINTER(P)] * 4 + [I, I], QUEUE),
    "ttsk_comm_unique_id": Entry([P]),
    "ttsk_comm_init": Entry([P, I, I]),
    "ttsk_comm_allreduce_sum": Entry([P, S, I], QUEUE),
    "ttsk_comm_reduce_sum": Entry([P, S, I, I], QUEUE),
    "ttsk_comm_allgather": Entry([P, P, S, I], QUEUE),
    "ttsk_comm_allreduce_max": Entry([P, S, I], QUEUE),
    "ttsk_comm_destroy": Entry([]),
}
del P, I, S, I64, U64


def ptr_array(arrays):
    """Host array of the device addresses of ``arrays`` (the `const double *const *` arguments)."""
    return (c_void_p * len(arrays))(*[a.ptr for a in arrays])


def i64_array(values):
    return (c_int64 * len(values))(*[int(v) for v in values])


def _bind(lib):
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    if missing:
        raise TtskError(f"{LIB_PATH} does not export {missing}")
    for name, e in ENTRY_POINTS.items():
        fn = getattr(lib, name)
        fn.argtypes = e.argtypes
        fn.restype = e.restype


def lib():
    """Loads libttsk.so (no device needed) and checks the exported symbol set."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise TtskError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`; "
                "tt_sketch_amd has no CPU fallback")
        handle = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
        _bind(handle)
        _lib = handle
    return _lib


def check(rc):
    if rc == 0:
        return
    msg = lib().ttsk_last_error().decode(errors="replace")
    if rc == TTSK_ERR_ARG:
        raise ValueError(msg)
    if rc == TTSK_ERR_UNSUPPORTED:
        raise TtskUnsupported(msg)
    raise TtskError(msg)


_sync_epoch = 0
# Which library streams have had work queued since they were last drained, and how often each has
# been drained: device.py tags a released buffer with this so that it is handed out again only to a
# user on the same stream, or after the streams that may still be touching it have been synchronised.
_stream_gen = [0] * NUM_STREAMS
_dirty = set()


def sync_epoch() -> int:
    """Number of device-wide synchronisations so far."""
    return _sync_epoch


def dirty_snapshot() -> dict:
    """{stream: drain generation} of every stream with work queued since its last drain.  A helper stream whose work
    was joined back into its caller's stream (the one-call TT sketches) counts as that stream: whatever is queued there
    later is ordered behind the helper's work too, so a buffer released now may go straight to a user on the caller's
    stream (every temporary of a loop of one-call sketches used to miss the pool and cost a hipMalloc)."""
    out = {}
    for s in _dirty:
        t = _joined_into.get(s, s)
        out[t] = _stream_gen[t]
    return out


def drained_since(stream: int, gen: int) -> bool:
    return _stream_gen[stream] > gen


# helper stream -> the stream its work was joined back into (the one-call TT sketches fork stream + 1 and join it
# before they return): draining the caller's stream then covers the helper too, unless something else was queued on
# the helper directly in the meantime
_joined_into = {}


def _mark(name, args):
    e = ENTRY_POINTS.get(name)
    if e is not None and e.role in _QUEUEING:
        s = int(args[-1])
        if 0 <= s < NUM_STREAMS:
            _dirty.add(s)
            _joined_into.pop(s, None)          # direct work on s: it is no longer merely a joined helper
            helpers = ((s + 1) % NUM_STREAMS,) if e.role == FORK_NEXT else \
                (tuple(h for h in range(NUM_STREAMS) if h != s) if e.role == FORK_ALL else ())
            for h in helpers:
                if h not in _dirty or _joined_into.get(h) == s:
                    _joined_into[h] = s
                _dirty.add(h)


def _drained(s):
    _stream_gen[s] += 1
    _dirty.discard(s)
    _joined_into.pop(s, None)
    for h, into in list(_joined_into.items()):
        if into == s:                          # everything the helper had in flight was ordered before this drain
            _stream_gen[h] += 1
            _dirty.discard(h)
            del _joined_into[h]


def call(name, *args):
    global _sync_epoch
    _mark(name, args)                      # before the call: a failing call may have queued part of its work
    check(getattr(lib(), name)(*args))
    role = ENTRY_POINTS[name].role
    if role in (DRAIN_FIRST, DRAIN_LAST):
        s = int(args[0 if role == DRAIN_FIRST else -1])
        if s < 0:                          # ttsk_sync(-1): every stream
            _sync_epoch += 1
            for i in range(NUM_STREAMS):
                _stream_gen[i] += 1
            _dirty.clear()
            _joined_into.clear()
        elif s < NUM_STREAMS:
            _drained(s)
