"""The host-side plans of the GEMM family (csrc/gemm_plan.h, plain C++): tests/gemm_plan_driver.cpp, compiled with the host
compiler, prints every non-pointer field of what gemm_route, rows_longk_plan, skinny_r_plan, skinny_s_plan, small_gemm_plan,
gemm_tile_plan and r_reduce_plan decide, and that is checked here -- before any kernel reads it.

(a) tests/golden/gemm_plan_cases.json holds, for a list of calls, what the launchers of the commit before gemm_plan.h decided
    (recorded from that commit's own gemm.hip / skinny.hip / small.hip / dense_right_pass.hip, compiled for the host and
    linked against stubs that print what they are handed): the family, and for it the kernel-argument struct, the
    instantiation, grid, block, LDS, scratch bytes, the arguments, kernel and grid of the slab sum, the profiling bracket's
    name and work, or the error and its message.  The list is the family table of tests/gemm_families_ref.py and the edge list
    below -- the smallest shapes on either side of every branch and refusal -- at 256 and at 20 compute units.  The plans must
    give the same, field by field.
(b) On every accepted plan of that list, the invariants the kernels rely on.
(c) The family table on the CPU: every case's descriptor, built as tests/test_gpu_gemm_families.py builds it, goes through
    gemm_route at 256 compute units; the route must be the case's family and every branch tag the kernel name does not show
    must follow from the plan's fields.
(d) The fall-back inside ttsk_gemm's loop over the slice groups of a batched long contraction is not reached: over a sweep of
    descriptors and alignments, the first group is accepted and so is every later one, or the whole batch goes to the tiles."""
import hashlib
import itertools
import json
import os
import re

import pytest

from tests import gemm_families_ref as fam
from tests.host_driver import ROOT, compile_driver, run_driver

DRIVER = os.path.join(ROOT, "tests", "gemm_plan_driver.cpp")
FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_plan_cases.json")

LIM32 = (1 << 32) - 64
LDS_MAX = 160 * 1024
N_CU = (256, 20)
BASE = {"A": 0x7F1000000000, "B": 0x7F2000000000, "C": 0x7F3000000000}      # device buffers are at least 256-byte aligned
DESC_KEYS = ("batch", "M", "N", "Ko", "Ki", "a_b", "a_m", "a_ko", "a_ki", "b_b", "b_ko", "b_ki", "b_n", "c_b", "c_m", "c_n")


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------------------ calls
def call(kind="route", alpha=1.0, acc=0, split_k=0, ks=0, off=(0, 0, 0), nb=1, tab=(0, 0, 0), **d):
    """One line of the driver's input, without id and n_cu; `off`: elements from the aligned bases of A, B, C; `tab`: elements
    between the problems of a pointer table."""
    assert set(d) == set(DESC_KEYS), sorted(set(DESC_KEYS) ^ set(d))
    return dict(kind=kind, d=d, alpha=float(alpha), acc=acc, split_k=split_k, ks=ks, nb=nb, tab=tuple(tab),
                ptr=tuple(BASE[x] + 8 * o for x, o in zip("ABC", off)))


def line(id, n_cu, c):
    if c["kind"] == "reduce":
        return "%s reduce %d %s" % (id, n_cu, " ".join(str(x) for x in c["v"]))
    v = [n_cu] + [c["d"][k] for k in DESC_KEYS] + [c["acc"], c["split_k"], c["ks"], *c["ptr"], c["nb"], *c["tab"]]
    return "%s %s %s %r" % (id, c["kind"], " ".join(str(int(x)) for x in v), c["alpha"])


def nn(M, N, K, batch=1, **kw):
    """A[m, k], B[k, n], C[m, n], all row-major"""
    d = dict(batch=batch, M=M, N=N, Ko=1, Ki=K, a_b=M * K, a_m=K, a_ko=0, a_ki=1, b_b=K * N, b_ko=0, b_ki=N, b_n=1, c_b=M * N, c_m=N, c_n=1)
    return _over(d, kw)


def tn(M, N, K, batch=1, **kw):
    """A stored [k, m], B [k, n]: m and n contiguous (the long-K chain shape)"""
    d = dict(batch=batch, M=M, N=N, Ko=1, Ki=K, a_b=M * K, a_m=1, a_ko=0, a_ki=M, b_b=K * N, b_ko=0, b_ki=N, b_n=1, c_b=M * N, c_m=N, c_n=1)
    return _over(d, kw)


def nt(M, N, K, batch=1, **kw):
    """A[m, k], B stored [n, k]: k contiguous on both sides (rows against rows)"""
    d = dict(batch=batch, M=M, N=N, Ko=1, Ki=K, a_b=M * K, a_m=K, a_ko=0, a_ki=1, b_b=K * N, b_ko=0, b_ki=1, b_n=K, c_b=M * N, c_m=N, c_n=1)
    return _over(d, kw)


def _over(d, kw):
    opts = {k: kw.pop(k) for k in list(kw) if k not in DESC_KEYS}
    d.update(kw)
    return call(**opts, **d)


def koki(M, N, Ko, Ki, gap=0, **kw):
    """m / n contiguous, two-level kappa: ko slices `gap` rows further apart than Ki rows (gap = 0 merges)"""
    return tn(M, N, Ki, Ko=Ko, a_ko=(Ki + gap) * M, b_ko=(Ki + gap) * N, **kw)


def reduce_call(chunks, M, N, m_tiles, nprob, Mtot, c_m, c_n, slab_off=0, c_off=0, c_tab=0):
    return dict(kind="reduce", v=(chunks, M, N, m_tiles, nprob, Mtot, c_m, c_n, 4096 + 8 * slab_off, BASE["C"] + 8 * c_off, c_tab))


def edge_calls():
    """The smallest shapes on either side of every branch and refusal of the route and the six plans."""
    e = {}
    # ---- the route: argument checks, empty, K == 0, k_scale keeps every shape on the tiles, the batched long contraction
    e["rt-neg"] = nn(-1, 4, 8)
    e["rt-batch-cb0"] = nn(8, 8, 8, batch=2, c_b=0)
    e["rt-batch1-cb0"] = nn(8, 8, 8, c_b=0)
    e["rt-empty-b"], e["rt-empty-m"], e["rt-empty-n"] = nn(4, 4, 8, batch=0), nn(0, 4, 8), nn(4, 0, 8)
    e["rt-k0"], e["rt-k0-acc"], e["rt-k0-ko"] = nn(4, 5, 0), nn(4, 5, 0, acc=1), nn(4, 5, 3, Ko=0)
    e["rt-ks-rows"], e["rt-ks-r"] = nt(64, 16, 4096, ks=1), tn(64, 32, 4096, ks=1)
    e["rt-ks-s"], e["rt-ks-small"], e["rt-ks-lb"] = nn(5, 3000, 128, ks=1), nn(37, 53, 29, ks=1), tn(8, 4, 32768, batch=2, a_b=0, ks=1)
    e["rt-lb-k32767"], e["rt-lb-k32768"] = tn(8, 4, 32767, batch=2, a_b=0), tn(8, 4, 32768, batch=2, a_b=0)
    e["rt-lb-33"], e["rt-lb-65-odd"] = tn(8, 4, 32768, batch=33, a_b=0), tn(7, 5, 33001, batch=65)
    e["rt-lb-big"] = tn(200, 300, 32768, batch=3)                 # both sides > 128: the first group is refused, tiles
    e["rt-lb-koki"] = koki(8, 4, 64, 600, gap=3, batch=2)
    e["rt-splits-65535"], e["rt-splits-65536"] = nn(8, 8, 8, batch=65535, ks=1), nn(8, 8, 8, batch=65536, ks=1)
    e["rt-splits-x"] = nn(8, 8, 4096, batch=100, split_k=656, ks=1)
    # ---- rows_longk_plan
    for N in (1, 33, 48, 49):
        e["rl-n%d" % N] = nt(130, N, 4096)
    e["rl-k4032"], e["rl-k4160"], e["rl-k4100"] = nt(64, 16, 4032), nt(64, 16, 4160), nt(64, 16, 4100)
    e["rl-srow-odd"], e["rl-brow-odd"] = nt(64, 16, 4096, a_m=4097), nt(64, 16, 4096, b_n=4097)
    e["rl-srow-short"], e["rl-brow-short"] = nt(64, 16, 4096, a_m=4094), nt(2, 16, 4096, b_n=4094)
    e["rl-offa"], e["rl-offb"], e["rl-offc"] = nt(64, 16, 4096, off=(1, 0, 0)), nt(64, 16, 4096, off=(0, 1, 0)), nt(64, 16, 4096, off=(0, 0, 1))
    e["rl-cn2"], e["rl-cm-odd"] = nt(64, 16, 4096, c_n=2, c_m=40), nt(64, 16, 4096, c_m=17)
    e["rl-rows1"], e["rl-rows65"], e["rl-rows-many"] = nt(1, 16, 8192), nt(65, 16, 4096), nt(64 * 600, 16, 4096)
    e["rl-nrb-2p20"], e["rl-nrb-over"] = nt(64 << 20, 16, 4096), nt((64 << 20) + 1, 2, 4096)
    e["rl-k-long"], e["rl-koki-merge"] = nt(64, 40, 1 << 24), nt(64, 16, 1024, Ko=4, a_ko=1024, b_ko=1024)
    e["rl-acc"] = nt(130, 48, 4160, alpha=-0.5, acc=1)
    # ---- skinny_r_plan
    e["sr-k4095"], e["sr-k4096"], e["sr-k4097"] = tn(64, 32, 4095), tn(64, 32, 4096), tn(64, 32, 4097)
    e["sr-both-129"], e["sr-128-129"], e["sr-129-128"] = tn(129, 129, 4096), tn(128, 129, 4096), tn(129, 128, 4096)
    e["sr-ki3"], e["sr-ki4"] = koki(64, 32, 2000, 3, gap=1), koki(64, 32, 1500, 4, gap=1)
    e["sr-neg"] = tn(64, 32, 4096, a_ki=-64)
    e["sr-oddm"], e["sr-oddn"], e["sr-oddki"] = tn(33, 64, 6000), tn(64, 33, 6000), tn(64, 16, 4200, a_ki=65)
    e["sr-offa"], e["sr-offb"] = tn(64, 32, 4096, off=(1, 0, 0)), tn(64, 32, 4096, off=(0, 1, 0))
    e["sr-swap-eq"], e["sr-swap"] = tn(64, 64, 4096), tn(32, 96, 5000, alpha=-3.0, acc=1)
    e["sr-gk"], e["sr-gk-kodd"], e["sr-gk-amodd"] = nt(100, 20, 4100), nt(100, 20, 4101), nt(100, 20, 4100, a_m=4101)
    e["sr-gk-off"], e["sr-gk-koki"] = nt(100, 20, 4100, off=(0, 1, 0)), nt(100, 20, 1025, Ko=4, a_ko=1030, b_ko=1030)
    e["sr-row-reach"], e["sr-row-over"] = nt(64, 49, 4096, a_m=17895696), nt(64, 49, 4096, a_m=17895698)
    e["sr-mtiles-60000"], e["sr-mtiles-60001"] = tn(128 * 60000, 8, 4096), tn(128 * 60000 + 1, 8, 4096)
    e["sr-tile-129"], e["sr-tile-300"] = tn(129, 20, 4096), tn(300, 20, 4097)
    e["sr-ko-uniform"], e["sr-ko-gap"] = koki(48, 40, 4, 1100), koki(34, 50, 9, 600, gap=50)
    e["sr-span-halve"], e["sr-span-out"] = tn(64, 32, 4096, a_ki=1 << 21), tn(64, 32, 4096, a_ki=1 << 23)
    e["sr-span-64"] = tn(64, 32, 1 << 20, a_ki=4000000)
    e["sr-reach-a"], e["sr-reach-ok"] = koki(64, 32, 8, 600, gap=1 << 20), koki(64, 32, 8, 600, gap=1 << 19)
    for nmt, nnt in ((1, 1), (4, 3), (4, 4), (5, 1), (6, 2), (5, 3), (7, 1), (7, 2), (8, 1), (8, 8)):
        e["sr-%dx%d" % (nmt, nnt)] = tn(16 * nmt, 16 * nnt - 2, 4160)
    e["sr-ct"] = tn(80, 6, 4608, c_m=1, c_n=84, alpha=-0.5, acc=1)
    e["sr-c-off"], e["sr-c-odd"] = tn(64, 32, 4096, off=(0, 0, 1)), tn(64, 32, 4096, c_m=33)
    # ---- skinny_s_plan
    e["ss-k128"], e["ss-k129"], e["ss-k1"] = nn(5, 3000, 128), nn(5, 3000, 129), nn(32, 2500, 1, a_m=0, b_ki=0)
    e["ss-k124-p128"], e["ss-k125-p128"], e["ss-k128-p112"] = nn(128, 3000, 124), nn(128, 3000, 125), nn(112, 3000, 128)
    e["ss-n2047"], e["ss-n2048"], e["ss-m129"] = nn(5, 2047, 64), nn(5, 2048, 64), nn(129, 4000, 64)
    e["ss-b-small"], e["ss-both"], e["ss-both-b"] = nn(4001, 20, 77), nn(100, 2100, 100), nn(2100, 100, 100)
    e["ss-batch-shared"], e["ss-batch-own"] = nn(24, 700, 20, batch=3, a_b=0), nn(24, 700, 20, batch=3)
    e["ss-batch-b-shared"], e["ss-batch-cneg"] = nn(700, 24, 20, batch=3, b_b=0), nn(24, 700, 20, batch=3, a_b=0, c_b=-24 * 700)
    e["ss-neg"], e["ss-koki"] = nn(5, 3000, 64, b_ki=-3000), nn(5, 3000, 16, Ko=4, a_ko=20, b_ko=3000 * 20)
    e["ss-j-max"], e["ss-j-over"] = nn(4, (1 << 31) - 257, 1), nn(4, (1 << 31) - 256, 1)
    e["ss-span-s"], e["ss-wext"], e["ss-big"] = nn(3000, 5, 64, a_m=1 << 25), nn(128, 3000, 8, a_m=1, a_ki=1 << 22), nn(5, 1 << 26, 8, b_n=8, b_ki=1)
    for P in (1, 4, 5, 8, 9, 16, 20, 24, 25, 127):
        e["ss-p%d" % P] = nn(P, 4000, 60)
    for K in (13, 16, 17, 20, 21, 77):
        e["ss-ring-k%d" % K] = nn(2300, 40, K)
    for N in (2048, 16 * 4 * 256, 16 * 5 * 256, 16 * 8 * 256 + 16, 16 * 8 * 1000):
        e["ss-mode-n%d" % N] = nn(100, N, 100)
        e["ss-mode8-n%d" % N] = nn(16, N, 32)
    # ---- small_gemm_plan
    e["sm-1"], e["sm-k1024"], e["sm-k1025"] = nn(37, 53, 29), nn(20, 21, 1024), nn(20, 21, 1025)
    e["sm-512"], e["sm-513"], e["sm-flop"], e["sm-flop-over"] = nn(512, 512, 91), nn(513, 20, 30), nn(512, 512, 91), nn(512, 512, 92)
    e["sm-batch32"], e["sm-batch33"], e["sm-batch-neg"] = nn(10, 14, 12, batch=32), nn(10, 14, 12, batch=33), nn(10, 14, 12, batch=3, a_b=-120)
    e["sm-neg"], e["sm-extent"], e["sm-koki"] = nn(10, 14, 12, c_n=-1), nn(10, 14, 12, a_m=1 << 27), nn(10, 14, 6, Ko=2, a_ko=7, b_ko=100)
    for K in (127, 128, 255, 256, 511, 512):
        e["sm-ksplit-k%d" % K] = nn(20, 21, K)
    # ---- gemm_tile_plan (k_scale keeps the small shapes on the tiles)
    for M in (16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128):
        e["g-f1-m%d" % M] = nn(M, 700, 300, ks=1)
        e["g-f2-n%d" % M] = nn(700, M, 300, ks=1)
    e["g-f0-129"], e["g-f1-128-128"], e["g-f2-129-128"] = nn(129, 129, 300), nn(128, 128, 40, ks=1), nn(129, 128, 300)
    e["g-auto-k127"], e["g-auto-k128"], e["g-auto-k1023"], e["g-auto-k1024"] = (nn(200, 200, K) for K in (127, 128, 1023, 1024))
    e["g-auto-191"], e["g-auto-192"], e["g-auto-cap"] = nn(64 * 191, 64, 2000, ks=1), nn(64 * 192, 64, 2000, ks=1), nn(40, 40, 1 << 20, ks=1)
    e["g-split1"], e["g-split3"], e["g-split-big"] = nn(200, 200, 2000, split_k=1), nn(201, 203, 1999, split_k=3), nn(600, 200, 40, split_k=5)
    e["g-nt"], e["g-tn"], e["g-tt"] = nt(300, 300, 500), tn(300, 300, 500), tn(300, 300, 500, b_ki=1, b_n=500)
    e["g-vec-offa"], e["g-vec-offb"], e["g-vec-oddk"] = nn(300, 300, 500, off=(1, 0, 0)), nn(300, 300, 500, off=(0, 1, 0)), nt(300, 300, 501)
    e["g-vec-oddm"], e["g-vec-oddlda"], e["g-vec-oddb"] = tn(301, 300, 500), nn(300, 300, 500, a_m=501), nn(300, 300, 64, batch=3, a_b=300 * 64 + 1)
    e["g-koki"], e["g-koki-odd"], e["g-koki-small"] = koki(300, 300, 4, 64, gap=2), nt(300, 300, 63, Ko=4, a_ko=64, b_ko=64), koki(300, 300, 40, 8, gap=2)
    e["g-neg"], e["g-span"], e["g-span-ok"] = nn(300, 300, 64, a_m=-64), nn(300, 300, 64, a_m=1 << 22), nn(300, 300, 64, a_m=1 << 21)
    e["g-batch-ct"], e["g-batch40"] = nn(600, 130, 50, batch=3, c_m=1, c_n=604, alpha=2.0, acc=1), nn(300, 40, 64, batch=40)
    # ---- pointer tables (gemm_each): nb problems of one shape
    e["b-r-2"], e["b-r-32"], e["b-r-33"] = (tn(100, 100, 6400, kind="batch", nb=nb, tab=(1 << 20, 1 << 20, 1 << 14)) for nb in (2, 32, 33))
    e["b-r-odd-tab"], e["b-r-0"] = tn(100, 100, 6400, kind="batch", nb=4, tab=(1 << 20, (1 << 20) + 1, 1 << 14)), tn(100, 100, 6400, kind="batch", nb=0)
    e["b-r-c-tab-odd"] = tn(100, 100, 6400, kind="batch", nb=4, tab=(1 << 20, 1 << 20, (1 << 14) + 1))
    e["b-s-32"], e["b-s-batch"] = nn(100, 6400, 100, kind="batch", nb=32, tab=(1 << 14, 1 << 20, 1 << 20)), nn(24, 700, 20, batch=3, a_b=0, kind="batch", nb=5, tab=(1 << 14, 1 << 20, 1 << 20))
    e["b-sm-8"], e["b-sm-batch"], e["b-none"] = nn(37, 53, 29, kind="batch", nb=8, tab=(4096, 4096, 4096)), nn(37, 53, 29, batch=2, kind="batch", nb=2, tab=(4096, 4096, 4096)), nn(600, 600, 600, kind="batch", nb=2, tab=(1 << 20, 1 << 20, 1 << 20))
    # ---- r_reduce_plan as the chain step and the dense left pass call it
    e["rr-scalar-cn"], e["rr-scalar-n"], e["rr-scalar-cm"] = reduce_call(64, 64, 32, 1, 1, 64, 1, 64), reduce_call(64, 64, 33, 1, 1, 64, 33, 1), reduce_call(64, 64, 32, 1, 1, 64, 33, 1)
    e["rr-scalar-slab"], e["rr-scalar-c"] = reduce_call(64, 64, 32, 1, 1, 64, 32, 1, slab_off=1), reduce_call(64, 64, 32, 1, 4, 64, 32, 1, c_tab=2049)
    e["rr-pair-c63"], e["rr-wide-c64"] = reduce_call(63, 128, 64, 1, 1, 128, 64, 1), reduce_call(64, 128, 64, 1, 1, 128, 64, 1)
    e["rr-pair-g63"], e["rr-wide-g64"] = reduce_call(64, 126, 64, 1, 1, 126, 64, 1), reduce_call(64, 127, 64, 1, 1, 127, 64, 1)
    e["rr-wide-gy"] = reduce_call(200, 16, 16, 8, 8, 128, 16, 1, c_tab=4096)
    return e


# ------------------------------------------------------------------------------------------------------------ the family table
class _Buf:
    def __init__(self, ptr):
        self.ptr = ptr


def family_call(case, monkeypatch):
    """The call ttsk_gemm gets for a case of the family table, built as tests/test_gpu_gemm_families.py builds it: the same
    lowering of device.contract or the same GemmDesc, the views PRE + off elements into buffers of their own."""
    import tt_sketch_amd.device as dev
    from tt_sketch_amd import _native as nat

    def desc_call(d, A, B, C):
        return call(alpha=d.alpha, acc=d.accumulate, split_k=d.split_k, ks=int(case.ks), off=(A, B, C), **{k: getattr(d, k) for k in DESC_KEYS})

    off = {x: fam.PRE + v.off for x, v in (("A", case.A), ("B", case.B), ("C", case.C))}
    if case.via == "desc":
        d = nat.GemmDesc()
        d.batch, d.M, d.Ko, d.Ki = case.A.shape
        d.N = case.B.shape[3]
        d.a_b, d.a_m, d.a_ko, d.a_ki = case.A.strides
        d.b_b, d.b_ko, d.b_ki, d.b_n = case.B.strides
        d.c_b, d.c_m, d.c_n = case.C.strides
        d.alpha, d.accumulate, d.split_k = float(case.alpha), int(case.acc), int(case.split_k)
        return desc_call(d, off["A"], off["B"], off["C"])
    got = []

    def fake(name, *args):
        assert name == "ttsk_gemm", name          # a contraction that had to copy an operand first would not be the table's case
        got.append(desc_call(args[0]._obj, *((a.ptr - BASE[x]) // 8 for x, a in zip("ABC", args[1:4]))))

    monkeypatch.setattr(nat, "call", fake)
    view = lambda x, v: dev.DevArray(_Buf(BASE[x]), off[x], v.shape, v.strides)
    dev.contract(case.spec, view("A", case.A), view("B", case.B), out=view("C", case.C), alpha=case.alpha, accumulate=bool(case.acc), split_k=case.split_k)
    assert len(got) == 1
    return got[0]


def all_calls(monkeypatch):
    """[(id, n_cu, call)]: the family table and the edge list at both device sizes"""
    todo = []
    for n_cu in N_CU:
        for c in fam.CASES:
            todo.append(("fam-%s@%d" % (c.id, n_cu), n_cu, family_call(c, monkeypatch)))
        todo += [("%s@%d" % (id, n_cu), n_cu, k) for id, k in edge_calls().items()]
    return todo


# ------------------------------------------------------------------------------------------------------------ the driver
def parse(text):
    """{id: (fields the parent's launchers showed, the plan's own intermediate decisions, message)}"""
    res = {}
    for ln in text.splitlines():
        head, msg = ln.split(" |", 1)
        head, _, own = head.partition(" ;; ")
        w = head.split()
        res[w[0]] = (dict(kv.split("=", 1) for kv in w[1:]), dict(kv.split("=", 1) for kv in own.split()), msg.strip())
    return res


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "gemm_plan", DRIVER)

    def run(lines):
        f = exe.parent / "cases.txt"
        f.write_text("\n".join(lines) + "\n")
        return run_driver(exe, [f])

    return run


@pytest.fixture(scope="module")
def monkeymodule():
    mp = pytest.MonkeyPatch()
    yield mp
    mp.undo()


@pytest.fixture(scope="module")
def listed(driver, monkeymodule):
    todo = all_calls(monkeymodule)
    monkeymodule.undo()
    return todo, parse(driver([line(*t) for t in todo]))


# ------------------------------------------------------------------------------------------------------------ (a)
def call_digest(text):
    return hashlib.sha1(text.encode()).hexdigest()[:10]


def fixture_rows(todo, shown_of):
    """The fixture's layout: the field names of each kind of answer once, then per call one row
    [id, digest of the call's line, kind of answer, the values in the order of the names, message]; kind "=" where the answer at
    20 compute units is the one at 256."""
    fields, rows = {}, []
    for t in todo:
        shown, msg = shown_of(t[0])
        if t[0].endswith("@20") and shown_of(t[0][:-2] + "256") == (shown, msg):
            rows.append([t[0], call_digest(line(*t)), "=", [], ""])
            continue
        kind = "%s/%d" % (shown.get("route", shown.get("fam", "reduce" if "rc" not in shown else "error")), len(shown))
        assert fields.setdefault(kind, list(shown)) == list(shown), (t[0], kind)
        rows.append([t[0], call_digest(line(*t)), kind, list(shown.values()), msg])
    return fields, rows


def test_plans_equal_the_parents_decisions(listed):
    todo, plans = listed
    with open(FIXTURE) as f:
        fixture = json.load(f)
    golden = {id: (digest, dict(zip(fixture["fields"][kind], values)), msg) for id, digest, kind, values, msg in fixture["rows"] if kind != "="}
    golden.update({id: (digest,) + golden[id[:-2] + "256"][1:] for id, digest, kind, _, _ in fixture["rows"] if kind == "="})
    assert [t[0] for t in todo] == [r[0] for r in fixture["rows"]] and all(call_digest(line(*t)) == golden[t[0]][0] for t in todo), \
        "the list of calls changed: the fixture holds the parent's answers to its own list"
    assert len(todo) == len(plans) == len(golden) and len(todo) > 500
    fams = {}
    for id, _, _ in todo:
        shown, _, msg = plans[id]
        _, want, want_msg = golden[id]
        assert shown == want and msg == want_msg, (id, {k: (shown.get(k), want.get(k)) for k in set(shown) | set(want) if shown.get(k) != want.get(k)}, msg)
        fams[shown.get("route", shown.get("fam", "reduce"))] = fams.get(shown.get("route", shown.get("fam", "reduce")), 0) + 1
    print("plans equal to the parent's decisions:", len(todo), fams)
    assert {"empty", "k0", "rows_longk", "skinny_r", "skinny_s", "small", "longk_batch", "tiles", "none", "reduce"} <= set(fams)
    assert any(plans[id][0].get("rc") == "-2" for id, _, _ in todo)


# ------------------------------------------------------------------------------------------------------------ (b)
def _aligned(c, x, n=1):
    """every problem's base of operand x (0, 1, 2: A, B, C) is 16-byte aligned"""
    step = c["tab"][x] if c["kind"] == "batch" else c["d"][("a_b", "b_b", "c_b")[x]]
    return all((c["ptr"][x] + 8 * b * step) % 16 == 0 for b in range(n))


def check_reduce(f, c_aligned, big_rows=False):
    chunks, M, N, m_tiles, nprob, Mtot, c_m, c_n = (int(x) for x in f["red"].split(",")[:8])
    variant, (gx, gy), block = int(f["rvariant"]), (int(x) for x in f["rgrid"].split(",")), int(f["rblock"])
    assert f["redC"] == "a" and gy == nprob * m_tiles and Mtot <= m_tiles * M
    assert gy <= 65535 or big_rows, "the second grid dimension"
    if variant:          # two consecutive n per lane: 16-byte loads and stores
        assert c_n == 1 and N % 2 == 0 and c_m % 2 == 0 and c_aligned
        lanes = 64 if variant == 2 else 16
        assert block == 16 * lanes and gx == cdiv(M * N // 2, lanes) and (variant == 1 or chunks >= 64)
    else:
        assert block == 256 and gx == cdiv(M * N, 16)
    return chunks, M, N, m_tiles, nprob


def check_skinny_r(c, f, own, n_cu):
    g = lambda k: int(f[k])
    d, nb = c["d"], g("nb")
    K, chunk, chunks, M, N, m_tiles = g("K"), g("chunk"), g("chunks"), g("M"), g("N"), g("m_tiles")
    nsub = int(own["nsub"])
    assert chunk % 8 == 0 and chunks == cdiv(K, chunk) and K >= 4096
    # at least 64 -- but for one corner the launcher always had and the plan keeps: where the 32-bit span of a chunk forces
    # halvings, the last one may go from under 128 to under 64 (sr-span-halve at 20 compute units: 208 -> 104 -> 56, row stride
    # 2^21).  The kernel masks by the chunk's length and takes any multiple of 8; the chunk before the halving did not fit.
    span = lambda ch: max(((16 * x if int(f["a_gen"]) else 144) + (ch + 64) * ki) * 8 for x, ki in ((int(f["a_m"]), int(f["a_ki"])), (int(f["b_n"]), int(f["b_ki"]))))
    assert chunk >= 64 or (g("rebase") and 32 <= chunk and span(2 * chunk - 8) >= LIM32), chunk
    assert g("grid") == nb * m_tiles * chunks <= (1 << 27) and g("block") == 512 and nb * m_tiles <= 60000
    assert g("scratch") == 8 * g("grid") * nsub * M * N + 64 and nsub == (8 if cdiv(M, 16) * cdiv(N, 16) <= 12 else 1)
    assert f["name"] == "skinny_r_kernel<%d,%d,4>" % (cdiv(M, 16), cdiv(N, 16)) and g("unit") == (0 if M <= 64 else 1 if M <= 96 else 2 if M <= 112 else 3)
    assert 1 <= N <= 128 and 1 <= M <= 128 and cdiv(N, 16) <= cdiv(g("Mtot"), 16) and m_tiles == cdiv(g("Mtot"), 128)
    swap = int(own["swap"])
    assert (f["tabA"], f["tabB"]) == (("b", "a") if swap else ("a", "b")) and f["slab"] == "0"
    a_gen, a_m, b_n, a_ki, b_ki, a_ko, b_ko = g("a_gen"), g("a_m"), g("b_n"), g("a_ki"), g("b_ki"), g("a_ko"), g("b_ko")
    assert a_gen == g("b_gen") and 15 * a_m * 8 < 1 << 31 and 15 * b_n * 8 < 1 << 31
    ali = _aligned(c, 0, nb) and _aligned(c, 1, nb)
    if a_gen == 0:       # pairs of rows by 16-byte loads
        assert a_m == b_n == 1 and not (g("Mtot") | N | a_ki | b_ki | a_ko | b_ko) & 1 and ali
    if a_gen == 2:       # pairs of kappa by 16-byte loads
        assert a_ki == b_ki == 1 and not (K | a_m | b_n) & 1 and ali and g("rebase")
    if g("rebase"):      # 32-bit offsets span one chunk and one row tile
        assert g("Ki") == K
        for gen, xs, ki in ((a_gen, a_m, a_ki), (a_gen, b_n, b_ki)):
            assert ((16 * xs if gen else 144) + (chunk + 64) * ki) * 8 < LIM32
    else:                # ... or the whole operand with the kappa walk past its end
        Ko, Ki = d["Ko"], d["Ki"]
        assert g("Ki") == Ki and Ko * Ki == K
        assert ((16 * a_m if a_gen else g("Mtot") + 144) + (Ko + 1) * a_ko + (Ki + 64) * a_ki) * 8 < LIM32
        assert ((16 * b_n if a_gen else 144) + (Ko + 1) * b_ko + (Ki + 64) * b_ki) * 8 < LIM32
    rc = check_reduce(f, _aligned(c, 2, nb))
    assert rc == (chunks * nsub, M, N, m_tiles, nb)


def check_skinny_s(c, f, own, n_cu):
    g = lambda k: int(f[k])
    npt, spt, dring, strips = (int(x) for x in re.match(r"skinny_s_kernel<(\d+),(\d+),(\d+),(\d+)>", f["name"]).groups())
    P, K, nb = g("P"), g("K"), g("nb")
    kb = cdiv(K, 4)
    ldw = 16 * npt if (16 * npt) % 32 == 16 else 16 * npt + 16
    assert npt == cdiv(P, 16) <= 8 and 1 <= K <= 128 and dring in (4, 5) and strips == ((P % 16 + 3) // 4 if 0 < P % 16 <= 8 else 0)
    assert g("lds") == cdiv(kb, dring) * dring * 4 * ldw * 8 <= LDS_MAX and cdiv(kb, dring) * dring <= cdiv(kb, 9 - dring) * (9 - dring)
    nrb = cdiv(g("J"), 16) if g("U") == 1 else g("U") * cdiv(g("V"), 16)
    assert g("groups") == cdiv(nrb, (4, 5, 8)[spt]) and 1 <= g("wpp") <= g("groups") and g("grid") == g("wpp") * nb and g("block") == 512
    assert g("J") == g("U") * g("V") < (1 << 31) - 256 and g("tvl") == 4 and g("nbv") == cdiv(g("V"), 16)
    assert (f["tabW"], f["tabS"]) == (("a", "b") if int(own["a_small"]) else ("b", "a")) and f["tabC"] == "a"
    assert (16 * g("s_j") + 4 * g("s_k")) * 8 < LIM32 and (16 * g("c_j") + 16 * g("c_m")) * 8 < LIM32 and g("w_extent") * 8 < 1 << 31
    if not g("big"):
        rows = g("J") if g("U") == 1 else g("V")
        assert ((g("U") + 4) * g("s_u") + (g("V") + 96) * g("s_j") + (K + 24) * g("s_k")) * 8 < LIM32
        assert ((g("U") + 4) * g("c_u") + (rows + 96) * g("c_j") + 144 * g("c_m")) * 8 < LIM32


def check_small(c, f, own, n_cu):
    g = lambda k: int(f[k])
    ksplit = int(own["ksplit"])
    assert g("grid") == g("nb") * g("tiles_m") * g("tiles_n") and g("block") == 64 * ksplit <= 512 and 1 <= g("nb") <= 32
    assert (g("tiles_m"), g("tiles_n")) == (cdiv(g("M"), 16), cdiv(g("N"), 32)) and g("K") <= 1024 and max(g("M"), g("N")) <= 512
    assert ksplit == (8 if g("K") >= 512 else 4 if g("K") >= 256 else 2 if g("K") >= 128 else 1)
    assert (g("a_extent") + 64 * g("a_k")) * 8 < LIM32 and (g("b_extent") + 64 * g("b_k")) * 8 < LIM32 and g("c_extent") * 8 < LIM32
    assert (f["tabA"], f["tabB"], f["tabC"]) == ("a", "a", "a") and f["name"] == "small_gemm_kernel"


def check_rows(c, f, own, n_cu):
    g = lambda k: int(f[k])
    K, N, nrb, nkc = g("K"), g("N"), g("nrb"), g("nkc")
    assert K % 64 == 0 and K >= 4096 and 1 <= N <= 48 and nrb == cdiv(g("rows"), 64) <= 1 << 20 and 1 <= nkc <= max(1, K // 64 // 8)
    assert g("grid") == nrb * nkc < 1 << 30 and g("block") == 512 and g("lds") == 2 * (64 + 48) * 64 * 8 <= LDS_MAX
    assert g("scratch") == 8 * nrb * nkc * 64 * N + 64 and not (g("s_row") | g("b_row")) & 1 and min(g("s_row"), g("b_row")) >= K
    assert _aligned(c, 0) and _aligned(c, 1) and (f["S"], f["B"], f["slab"]) == ("1", "1", "0")
    # rows_longk_plan takes up to 2^20 blocks of 64 rows, as its launcher always did, but the slab sum puts the blocks on the
    # grid's second dimension: beyond 65535 blocks (4.2 M rows of at least 32 KB) that launch is refused with an error.  Known
    # and kept: the plans decide what the launchers decided.
    assert check_reduce(f, _aligned(c, 2), big_rows=nrb > 65535) == (nkc, 64, N, nrb, 1)


def check_tiles(c, f, own, n_cu):
    g = lambda k: int(f[k])
    dd = [[int(x) for x in part.split(",")] for part in f["d"].split("|")[:4]]
    (batch, M, N, Ko, Ki), (a_b, a_m, a_ko, a_ki), (b_b, b_ko, b_ki, b_n), _ = dd
    K, kchunk, splits, bm, bn = Ko * Ki, g("kchunk"), g("splits"), g("bm"), g("bn")
    wm, wn, tm, tn, ak, bk = re.match(r"gemm_f64_kernel<(\d),(\d),(\d),(\d),(\w+),(\w+)>", f["name"]).groups()
    ak, bk = ak == "true", bk == "true"
    assert (bm, bn) == (16 * int(wm) * int(tm), 16 * int(wn) * int(tn)) and int(wm) * int(wn) == 4 and f["ptrs"] == "1" and f["partial"] == "0"
    assert kchunk % 32 == 0 and kchunk > 0 and splits == cdiv(K, kchunk)
    gx, gy, gz = (int(x) for x in f["grid"].split(","))
    assert (gx, gy, gz) == (cdiv(N, bn), cdiv(M, bm), batch * splits) and gz <= 65535
    # (the row tiles are the grid's second dimension: more than 65535 of them -- over a million rows -- and the launch is refused
    # with an error, as it always was; the plans decide what the launchers decided)
    assert gy <= 65535 or M > 16 * 65535
    tiles_m, tiles_n = gy * bm // 16, gx * bn // 16
    assert g("scratch") == (8 * batch * splits * tiles_m * tiles_n * 256 + 64 if splits > 1 else 0)
    if splits > 1:
        assert f["sred"] == "%d,%d,%d,%d" % (min(4096, batch * tiles_m * tiles_n * 4), tiles_m, tiles_n, int(wm) == 4)
    ld = lambda bx, kf: bx * 34 if kf else 32 * (bx if bx % 32 == 16 else bx + 16)
    assert g("lds") == 8 * (ld(bm, ak) + ld(bn, bk)) <= LDS_MAX
    even = lambda *v: not any(x & 1 for x in v)
    for vec, kf, x, xs, ko, bs, X, al in ((g("avec"), ak, a_m, a_ki, a_ko, a_b, M, _aligned(c, 0)), (g("bvec"), bk, b_n, b_ki, b_ko, b_b, N, _aligned(c, 1))):
        if vec:           # 16-byte loads: even strides, whole pairs inside the extents, aligned base
            assert al and even(ko, bs) and (even(x, K) and xs == 1 and (Ko == 1 or even(Ki)) if kf else x == 1 and even(xs, X))
    if g("fast_ok"):
        assert min(a_m, a_ki, a_ko, b_n, b_ki, b_ko) >= 0
        assert (bm * a_m + Ko * a_ko + (Ki + 32) * a_ki) * 8 < 1 << 31 and (bn * b_n + Ko * b_ko + (Ki + 32) * b_ki) * 8 < 1 << 31


CHECKS = {"skinny_r": check_skinny_r, "skinny_s": check_skinny_s, "small": check_small, "rows_longk": check_rows, "tiles": check_tiles}


def test_accepted_plans_hold_what_the_kernels_rely_on(listed):
    todo, plans = listed
    n = {}
    for id, n_cu, c in todo:
        f, own, _ = plans[id]
        if f.get("fam") in CHECKS:
            try:
                CHECKS[f["fam"]](c, f, own, n_cu)
            except AssertionError as e:
                raise AssertionError((id, f, own)) from e
            n[f["fam"]] = n.get(f["fam"], 0) + 1
    print("plans checked:", n)
    assert set(n) == set(CHECKS) and min(n.values()) >= 30


# ------------------------------------------------------------------------------------------------------------ (c)
REDUCE_TAGS = ("red:scalar", "red:paired", "red:paired_wide")
# the tags of a case that only its plan shows (the others state the shape, or follow from the kernel name)
PLAN_TAG = re.compile(r"sr:(swap|noswap|pair|gen_\w+|gk|rebase|ko_nonuniform|nsub\d|chunks_ragged|ragged_tile)$|ss:(a_small|b_small|ring\d|str\d|batch_shared)$|"
                      r"lb:|g:(autosplit|split\w+)$|red:")


def plan_tags(case, c, f, own):
    """the branch tags of the family table that follow from the plan's fields"""
    t = set()
    fam_ = f.get("fam")
    if fam_ == "skinny_r" and f["route"] == "skinny_r":
        g = lambda k: int(f[k])
        t.add("sr:swap" if own["swap"] == "1" else "sr:noswap")
        if g("a_gen") == 0:
            t.add("sr:pair")
        if g("a_gen") == 2:
            t.add("sr:gk")
        if g("a_gen") == 1:
            pair_a, pair_b = own["a_pair"] == "1", own["b_pair"] == "1"
            d = c["d"]
            if not _aligned(c, 0) or not _aligned(c, 1):
                t.add("sr:gen_off8")
            elif (d["M"] & 1 and not pair_a and d["a_m"] == 1) or (d["N"] & 1 and not pair_b and d["b_n"] == 1):
                t.add("sr:gen_oddM")
            elif (d["a_m"] == 1 and not pair_a) or (d["b_n"] == 1 and not pair_b):
                t.add("sr:gen_oddstride")
        if g("rebase"):
            t.add("sr:rebase")              # one stride walks kappa: per-workgroup origins
        if not g("rebase"):
            t.add("sr:ko_nonuniform")
        t.add("sr:nsub%s" % own["nsub"])
        if g("K") % g("chunk"):
            t.add("sr:chunks_ragged")
        if g("Mtot") % 128 and g("m_tiles") > 1:
            t.add("sr:ragged_tile")
    if fam_ == "skinny_s":
        t.add("ss:a_small" if own["a_small"] == "1" else "ss:b_small")
        m = re.match(r"skinny_s_kernel<\d+,\d+,(\d+),(\d+)>", f["name"])
        t |= {"ss:ring" + m.group(1), "ss:str" + m.group(2)}
        if int(f["U"]) > 1:
            t.add("ss:batch_shared")
    if f.get("route") == "longk_batch":
        batch = c["d"]["batch"]
        t |= {"lb:%d" % (batch if batch <= 32 else 33), "lb:acc" if c["acc"] else "lb:noacc"}
    if fam_ == "tiles":
        if c["split_k"] == 0 and int(f["splits"]) > 1:
            t.add("g:autosplit")
        if c["split_k"]:
            t.add("g:split%d" % c["split_k"] if c["split_k"] <= 3 else "g:split_big")
    if "rvariant" in f:
        t.add(REDUCE_TAGS[int(f["rvariant"])])
    return t


def test_family_table_reaches_its_families_and_tags_on_the_cpu(driver, monkeymodule):
    calls = {c.id: family_call(c, monkeymodule) for c in fam.CASES}
    monkeymodule.undo()
    plans = parse(driver([line(id, 256, k) for id, k in calls.items()]))
    seen = set()
    for case in fam.CASES:
        k = calls[case.id]
        f, own, msg = plans[case.id]
        assert f["rc"] == "0", (case.id, msg)
        # the route is the case's family, with its number of bracketed launches
        want_l = case.launches if case.launches is not None else (0 if case.fam is None else 1)
        assert int(f["launches"]) == want_l and f["fallback"] == "0", (case.id, f["route"], f["launches"])
        if case.fam is None:
            assert f["route"] in ("empty", "k0"), (case.id, f["route"])
            continue
        name = f["name"].replace(",", ", ")
        assert re.match(case.fam, name), (case.id, name, case.fam)
        assert {"rows_longk": "rows_longk", "skinny_r": "skinny_r", "longk_batch": "batched long-K", "skinny_s": "skinny_s", "small": "small_gemm",
                "tiles": "gemm_f64"}[f["route"]] == fam._family(case), (case.id, f["route"])
        # a case states the branches it is there for, not every one it takes: each stated tag must be derived.  Within a group of
        # alternatives (swap / noswap, pair / gen_* / gk, nsub1 / nsub8, ring4 / ring5, ...) the plan yields exactly one, so a
        # stated tag the plan contradicts fails here.
        got = plan_tags(case, k, f, own)
        want = {t for t in case.tags if PLAN_TAG.match(t)}
        assert want <= got, (case.id, sorted(want - got))
        seen |= got
    assert set(REDUCE_TAGS) <= seen, sorted(set(REDUCE_TAGS) - seen)
    need = {t for ts in fam.REQUIRED.values() for t in ts if PLAN_TAG.match(t)}
    assert need <= seen, sorted(need - seen)


# ------------------------------------------------------------------------------------------------------------ (d)
def test_no_slice_group_is_refused_after_the_first(driver):
    """ttsk_gemm's loop over the groups of SK_MAXB slices of a batched long contraction falls back to the tiles when a group is
    refused after earlier ones ran.  skinny_r_plan refuses by the descriptor, which the groups share, or by limits that grow with
    the group's size, and the first group is the largest; the alignment of a slice only picks the operand variant."""
    lines, n, batch_of = [], 0, {}
    shapes = ((8, 4), (7, 5), (130, 4), (40, 130), (128, 128), (129, 130))
    for K, layout, (M, N), batch, n_cu, off, share in itertools.product(
            (32768, 32769, 33000, 1 << 16, 1 << 20, 1 << 26), (tn, nt), shapes, (2, 3, 31, 32, 33, 64, 65, 200), (20, 64, 256),
            ((0, 0, 0), (1, 0, 0), (0, 1, 1)), (0, 1, 2)):
        kw = {}
        if share == 0:
            kw["a_b"] = 0                        # A shared by the batch
        elif share == 2:
            kw["a_b"], kw["b_b"], kw["c_b"] = M * K + 1, K * N + 3, M * N + 1      # slices of alternating alignment
        lines.append(line("s%d" % n, n_cu, layout(M, N, K, batch=batch, off=off, **kw)))
        batch_of["s%d" % n] = batch
        n += 1
    kinds = {}
    for id, (f, _, _) in parse(driver(lines)).items():
        assert f["rc"] == "0" and f["fallback"] == "0", (id, f)
        assert f["route"] in ("longk_batch", "tiles"), (id, f["route"])
        if f["route"] == "longk_batch":
            assert int(f["launches"]) == cdiv(batch_of[id], 32), (id, f["launches"])
        kinds[f["route"]] = kinds.get(f["route"], 0) + 1
    print("slice-group sweep:", n, kinds)
    assert n > 15000 and min(kinds.get("longk_batch", 0), kinds.get("tiles", 0)) > 1000
