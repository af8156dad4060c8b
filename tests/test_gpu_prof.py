"""The per-launch device timer (csrc/prof.h: ttsk_prof_enable / ttsk_prof_read / ttsk_prof_kernel_name) over every launcher
that brackets its kernel.

Each scenario of SCENARIOS runs one or a few calls with profiling on and reads all twelve classes: the kernel name kept
(that of the class's largest launch), the number of bracketed launches and the summed work.  EXPECTED holds what the same
scenario code gave on an MI355X at commit dedb75d ("One table for the C entry points; DevArray is a ctypes argument"),
the last one with the timer inside tt_fused.hip and the names decoded there from integer codes.  bench.py keys
profiles/*_traffic.json by these names and writes them into its record, so names and counts are compared exactly, and so
is the work: it is host arithmetic on the shapes.  A class that EXPECTED does not list must stay at ("", 0, 0.0).

The shapes are the small cases of the parity tests that reach each family (test_gpu_parity.py, test_gpu_dense_pass.py,
test_gpu_ndtri_edges.py, test_gpu_dense_error.py); the values computed are checked there, not here.

No launcher opens a bracket inside another one (the sampler and sparse scopes, the span of dense_pass.hip and the chain
steps hold plain launches only), so the nesting case queues calls on two streams alternately and counts the brackets.
"""
import ctypes

import numpy as np
import pytest

from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

NCLS = 12
V = ctypes.c_void_p


def read_classes():
    """{class: (kernel name, launches, work)} of every class with a launch or a name"""
    from tt_sketch_amd import _native as nat
    out = {}
    for c in range(NCLS):
        n, work = ctypes.c_int64(-1), ctypes.c_double(-1.0)
        name = ctypes.create_string_buffer(96)
        nat.call("ttsk_prof_read", c, ctypes.byref(n), None, ctypes.byref(work))
        nat.call("ttsk_prof_kernel_name", c, name, ctypes.c_size_t(len(name)))
        if n.value or work.value or name.value:
            out[c] = (name.value.decode(), n.value, work.value)
    return out


def profile(run, on=True):
    from tt_sketch_amd import _native as nat
    nat.call("ttsk_prof_enable", 1)
    if not on:
        nat.call("ttsk_prof_enable", 0)
    try:
        run()
        nat.call("ttsk_sync", -1)
        return read_classes()
    finally:
        nat.call("ttsk_prof_enable", 0)


# ------------------------------------------------------------------------------------------------------------ the calls
def chain_step(entry, case, stream=0):
    """ttsk_chain_step / _wide / _sum on random operands; case = (nb, n, K1, A, A2, J, right-chain strides?, T)"""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray, as_dev
    nb, n, K1, A, A2, J, right, wt = case
    rng = np.random.default_rng(7)
    shp, strides = ((J, n, K1), (n * K1, K1, 1)) if right else ((K1, n, J), (1, J, n * J))
    dW = [as_dev(rng.standard_normal((K1, A))) for _ in range(nb)]
    dX = [as_dev(rng.standard_normal(shp)) for _ in range(nb)]
    dE = as_dev(rng.standard_normal((A, n, A2)))
    dO = [DevArray.zeros((J, A2)) for _ in range(nb)]
    arr = lambda xs: (V * nb)(*[x.ptr for x in xs])
    head = (nb, n, K1, A, A2, J, arr(dW), A, arr(dX), strides[0], strides[1], strides[2], J * n * K1, V(dE.ptr))
    if entry == "ttsk_chain_step_sum":           # wt: 0 = no T, 1 = interleaved over the terms, 2 = per term
        dT, t_b, t_ld = None, 0, 0
        if wt == 1:
            dT, t_b, t_ld = DevArray.zeros((A, n, nb, J)), J, nb * J
        elif wt == 2:
            dT, t_b, t_ld = DevArray.zeros((nb, A, n, J)), A * n * J, J
        nat.call(entry, *head, None if dT is None else V(dT.ptr), t_b, t_ld, 0 if dT is None else dT.size, arr(dO), stream)
    else:
        dT = [DevArray.zeros((A, n, J)) for _ in range(nb)] if wt else None
        nat.call(entry, *head, arr(dT) if wt else None, arr(dO), stream)
    return dW, dX, dE, dO, dT                    # alive until the caller has synchronised


def sketch_tt(tsa):
    tt = tsa.TensorTrain.random((64, 64, 64, 64), 20, seed=1)
    return tsa.stream_sketch(tt, 50, 100, seed=2)                                      # Psi: stream_small_kernel


def sketch_sum(tsa):
    terms = [tsa.TensorTrain.random((70, 66, 68, 40), (52, 57, 49), seed=20 + i) for i in range(3)]
    return tsa.stream_sketch(tsa.TensorSum(terms), (26, 28, 30), (54, 58, 70), seed=6)  # Psi: stream_small_sum_kernel


def dense_passes(tsa):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray, as_dev
    rng = np.random.default_rng(3)
    n0, Q, T, ll, r = 32, 8, 16, 20, 40
    Xd, Cd, Pd = as_dev(rng.standard_normal((n0, Q, T))), as_dev(rng.standard_normal((n0, ll))), as_dev(rng.standard_normal((Q, r)))
    Z, U = DevArray.empty((ll, Q, T)), DevArray.empty((n0, r, T))
    nat.call("ttsk_dense_first_pass", V(Xd.ptr), n0, Q, T, V(Cd.ptr), ll, V(Pd.ptr), r, V(Z.ptr), V(U.ptr), 0)
    n0, n1, n2, n3, n4, l = 8, 3, 8, 8, 64, 20
    C = n3 * n4
    ins = [as_dev(rng.standard_normal(s)) for s in ((n0, n1, n2, n3, n4), (l, n0), (l, n1, n0), (l, n2, n1, n0), (l, n3, n2, n0 * n1))]
    outs = [DevArray.empty(s) for s in ((l, n1 * n2 * C), (l, n2 * C), (l, C), (l, C))]
    nat.call("ttsk_dense_left_pass", V(ins[0].ptr), n0, n1, n2, C, n4, l, *[V(a.ptr) for a in ins[1:]], *[V(z.ptr) for z in outs], 0)
    rows_longk(tsa)


def rows_longk(tsa):
    """the right-hand product of a dense sketch with a Gaussian DRM matrix: rows_longk_kernel behind ttsk_gemm"""
    return gemm("bq,mq->bm", (20, 4096), (40, 4096))


def samplers(tsa):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    ns = [3 * 2048 + 5, 0, 257]
    outs = [DevArray.empty((max(n, 1),)) for n in ns]
    nat.call("ttsk_fill_normal_many", 3, (V * 3)(*[o.ptr for o in outs]), (ctypes.c_size_t * 3)(*ns), (ctypes.c_uint64 * 3)(5, 6, 7),
             (ctypes.c_double * 3)(1.0, 0.25, 1.0), 0)
    tab = DevArray.empty((300, 17))
    nat.call("ttsk_sparse_normal_table", (ctypes.c_uint64 * 2)(20, 15), 2, 0, 17, ctypes.c_uint64(11), V(tab.ptr), 0)
    nat.call("ttsk_sync", -1)


def sparse_normal_dev(tsa):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    # ttsk_sparse_normal_dev: many rows over few prefixes (every prefix sampled once, rows copied out), then row by row
    rng = np.random.default_rng(5)
    rows = []
    for shape, N, w in (((5, 6), 1000, 8), ((50, 60, 70), 1003, 26)):
        idx = DevArray.from_host(np.stack([rng.integers(0, n, N) for n in shape]).astype(np.int64))
        rows.append((idx, DevArray.empty((N, w))))
        nat.call("ttsk_sparse_normal_dev", V(idx.ptr), N, None, (ctypes.c_uint64 * len(shape))(*shape), len(shape), ctypes.c_size_t(N),
                 3, 3 + w, ctypes.c_uint64(99), V(rows[-1][1].ptr), 0)
    nat.call("ttsk_sync", -1)


def sparse_passes(tsa):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    N, n, l, r = 1000, 7, 10, 15
    rng = np.random.default_rng(N + n)
    idx = rng.integers(0, n, N).astype(np.int64)
    d_idx, d_val = DevArray.from_host(idx), DevArray.from_host(rng.standard_normal(N))
    d_perm = DevArray.from_host(np.argsort(idx, kind="stable").astype(np.int64))
    d_L, d_R = DevArray.from_host(rng.standard_normal((N, l))), DevArray.from_host(rng.standard_normal((N, r)))
    out = DevArray.zeros((l, n, r))
    nat.call("ttsk_sparse_psi", V(d_val.ptr), V(d_idx.ptr), V(d_perm.ptr), ctypes.c_size_t(N), V(d_L.ptr), l, V(d_R.ptr), r, n,
             V(out.ptr), 0)
    sparse_gauss_pass(tsa)


def sparse_gauss_pass(tsa):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    from tt_sketch_amd.sparse_fused import _Factor
    rng = np.random.default_rng(13)
    # one fused pass: no left factor, the right one sampled in the pass from the suffix index, one nonzero per slice
    N, w = 600, 17
    fr = DevArray.from_host(rng.integers(0, 1 << 40, N).astype(np.uint64))
    jj = DevArray.from_host(np.arange(N, dtype=np.int32).view(np.int64))
    val, psi = DevArray.from_host(np.ones(N)), DevArray.zeros((1, N, w))
    B = _Factor(2, w, 3, 1, 0, 12345, None, 0, 0)
    nat.call("ttsk_sparse_gauss_pass", None, V(fr.ptr), V(jj.ptr), V(val.ptr), ctypes.c_size_t(N), N, None, ctypes.byref(B), None, 0,
             V(psi.ptr), None, 0)
    nat.call("ttsk_sync", -1)


def dense_stats(tsa, streams=(0,), with_stats=True):
    """ttsk_tt_dense_stats (`with_stats`) and ttsk_sumsq, once per entry of `streams`"""
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    rng = np.random.default_rng(9)
    M, N, rho = 17, 65, 3
    dL, dR, dx = (DevArray.from_host(rng.standard_normal(s)) for s in ((M, rho), (rho, N), (M, N)))
    keep = []
    for s in streams:
        out, stats, ss = DevArray.empty((M, N), stream=s), DevArray.empty((4,), stream=s), DevArray.empty((1,), stream=s)
        keep += [out, stats, ss]
        if with_stats:
            nat.call("ttsk_tt_dense_stats", V(dL.ptr), M, V(dR.ptr), N, rho, V(dx.ptr), V(out.ptr), V(stats.ptr), s)
        nat.call("ttsk_sumsq", V(dx.ptr), ctypes.c_size_t(M * N), V(ss.ptr), s)
    nat.call("ttsk_sync", -1)


def gemm(spec, a_shape, b_shape):
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import as_dev, contract
    rng = np.random.default_rng(1)
    out = contract(spec, as_dev(rng.standard_normal(a_shape)), as_dev(rng.standard_normal(b_shape)))
    nat.call("ttsk_sync", -1)
    return out


SCENARIOS = {
    "a_chain_step": lambda tsa: chain_step("ttsk_chain_step", (2, 20, 64, 22, 22, 30, True, True)),
    "b_chain_step_wide": lambda tsa: chain_step("ttsk_chain_step_wide", (2, 9, 37, 33, 47, 29, False, True)),
    "c_chain_step_sum": lambda tsa: chain_step("ttsk_chain_step_sum", (9, 11, 12, 30, 22, 9, False, 2)),
    "d_sketch_tt": sketch_tt,
    "d_sketch_sum": sketch_sum,
    # each class keeps the name of its largest launch: the smaller launches of e .. h once more on their own
    "e_dense_passes": dense_passes,
    "e_rows_longk": rows_longk,
    "f_samplers": samplers,
    "f_sparse_normal_dev": sparse_normal_dev,
    "g_sparse_passes": sparse_passes,
    "g_sparse_gauss_pass": sparse_gauss_pass,
    "h_dense_stats": dense_stats,
    "h_sumsq": lambda tsa: dense_stats(tsa, with_stats=False),
    # the families behind ttsk_gemm, one call each (class 11 keeps one name): the names the launchers of gemm.hip, small.hip
    # and skinny.hip format
    "i_gemm_tiles": lambda tsa: gemm("mk,kn->mn", (600, 200), (200, 520)),
    "i_gemm_small": lambda tsa: gemm("mk,kn->mn", (20, 30), (30, 25)),
    "i_gemm_skinny_s": lambda tsa: gemm("mk,kn->mn", (5, 128), (128, 3000)),
    "i_gemm_skinny_r": lambda tsa: gemm("km,kn->mn", (8192, 40), (8192, 64)),
}

# recorded at the commit named above: ttsk_prof_kernel_name, launches and work of ttsk_prof_read per class
EXPECTED = {
 'a_chain_step': {11: ('chain_step_kernel<1, 2, 1, 2, 5, true, 1, 2, 5>', 1, 4540800.0)},
 'b_chain_step_wide': {11: ('chain_wide_kernel<2, 2, 3, 0, true, 5, true>', 1, 2893968.0)},
 'c_chain_step_sum': {11: ('chain_sum_kernel<5, 5, NA, true>', 1, 1817640.0)},
 'd_sketch_sum': {1: ('chain_wide_kernel<2, 2, 4, 0, false, 5, true>', 2, 306758736.0),
                  3: ('chain_step_kernel<2, 0, 2, 0, 5, true, 1, 2, 5>', 2, 95650272.0),
                  4: ('stream_small_sum_kernel<1, 1, 5, 5>', 2, 73222896.0),
                  5: ('small_gemm_kernel', 7, 4534056.0)},
 'd_sketch_tt': {0: ('gemm_f64_kernel<1, 4, 4, 1, false, true>', 2, 10240000.0),
                 1: ('skinny_r_kernel<7, 2, 4>', 2, 51200000.0),
                 2: ('gemm_f64_kernel<1, 4, 4, 1, false, false>', 2, 5120000.0),
                 3: ('gemm_f64_kernel<1, 4, 2, 1, false, false>', 2, 12800000.0),
                 4: ('stream_small_kernel<6, 1, 5, 5>', 1, 25600000.0),
                 5: ('small_gemm_kernel', 5, 1368000.0)},
 'e_dense_passes': {8: ('dense_pass', 1, 0.0), 11: ('dense_left_pass_kernel', 2, 22282240.0)},
 'e_rows_longk': {11: ('rows_longk_kernel', 1, 6553600.0)},
 'f_samplers': {6: ('sample_rows_kernel (prefix table)', 1, 5100.0)},
 'f_sparse_normal_dev': {6: ('sample_rows_kernel / expand_rows_kernel', 2, 34078.0)},
 'g_sparse_gauss_pass': {7: ('sg_pass_kernel', 1, 16800.0)},
 'g_sparse_passes': {7: ('sparse_psi_mfma_kernel', 2, 240800.0)},
 'h_dense_stats': {9: ('tt_dense_stats_kernel', 2, 8840.0)},
 'h_sumsq': {9: ('sumsq_kernel', 1, 2210.0)},      # read off that commit's tt_dense_stats.hip (one bracket, 2 n), not recorded
 'i_gemm_skinny_r': {11: ('skinny_r_kernel<4, 3, 4>', 1, 41943040.0)},
 'i_gemm_skinny_s': {11: ('skinny_s_kernel<1, 0, 4, 2>', 1, 3840000.0)},
 'i_gemm_small': {11: ('small_gemm_kernel', 1, 30000.0)},
 'i_gemm_tiles': {11: ('gemm_f64_kernel<2, 2, 2, 2, true, false>', 1, 124800000.0)},
}


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_names_launches_and_work_as_before_the_move(tsa, name):
    got = profile(lambda: SCENARIOS[name](tsa))
    print(f"[prof] {name}: {got!r}")
    assert got == EXPECTED[name]


def test_scenarios_reach_the_kernels_they_are_meant_for():
    """the recorded table itself: every launcher that formats a name is in it"""
    names = {name for rec in EXPECTED.values() for name, _, _ in rec.values()}
    for prefix in ("chain_step_kernel<", "chain_wide_kernel<", "chain_sum_kernel<", "stream_small_kernel<", "stream_small_sum_kernel<",
                   "dense_pass", "dense_left_pass_kernel", "rows_longk_kernel", "sample_rows_kernel / expand_rows_kernel",
                   "sample_rows_kernel (prefix table)", "sparse_psi_mfma_kernel", "sg_pass_kernel", "tt_dense_stats_kernel", "sumsq_kernel",
                   "gemm_f64_kernel<", "small_gemm_kernel", "skinny_s_kernel<", "skinny_r_kernel<"):
        assert any(n.startswith(prefix) for n in names), prefix
    assert set(EXPECTED["d_sketch_tt"]) >= {0, 1, 2, 3, 4, 5}           # the TT pipeline classes: ProfClass scoping
    assert EXPECTED["h_dense_stats"][9][1] == 2                         # ttsk_tt_dense_stats + ttsk_sumsq


def test_brackets_on_two_streams_queued_alternately(tsa):
    """Two streams, the calls queued alternately and nothing synchronised in between: every bracket times its own record, so
    class 9 counts one launch per bracket opened (two per stream visit) and sums their work."""
    visits = (0, 1, 0, 1, 0, 1)
    got = profile(lambda: dense_stats(tsa, streams=visits))
    one = EXPECTED["h_dense_stats"][9]
    assert got == {9: (one[0], 2 * len(visits), one[2] * len(visits))}


def test_profiling_off_records_nothing(tsa):
    assert profile(lambda: chain_step("ttsk_chain_step", (2, 20, 64, 22, 22, 30, True, True)), on=False) == {}
    assert profile(lambda: dense_stats(tsa), on=False) == {}
