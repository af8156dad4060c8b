"""Reference, guarded operands and case table for the two Psi product kernels of csrc/stream_small.h --
stream_small_kernel (ttsk_psi_stream) and stream_small_sum_kernel (ttsk_psi_stream_sum).  Plain module, no GPU:
tests/test_psi_plan.py runs the table through the host plans (csrc/psi_plan.h) and tests the checker on seeded defects,
tests/test_gpu_psi_edges.py runs every case on the device.

    ss:   C_b[j, a] (+)= sum_c S_b[j, c] W_b[c, a]                 nb problems, one C each
    sss:  C[j, a]   (+)= sum_b sum_c S_b[j, c] W_b[c, a]           nb terms into one C

A case is (id, kind, nb, J, K1, A, opts).  The kernels refuse J < 1024, so 1024 rows is the smallest case there is.
Options: s_pad / w_pad / c_pad (row strides s_j = K1 + s_pad, w_c = A + w_pad, c_j = A + c_pad), acc (accumulate into a
prior C), s_gap / w_gap (sum kernel: s_b = J s_j + s_gap, w_b = K1 w_c + w_gap), nan_gap (the doubles between two terms of S
hold NaN: see below), refuse (the plan must refuse the call), and raw overrides s_j / w_c / c_j / s_b of a refusal.

Buffers.  Every device buffer has PRE = POST = 64 guard elements around it.  C and its guards start as the sentinel -1/3
(finite, no multiple of 1/2: an unwritten element fails the integer pass, a stray store changes a guard); with acc the
J x A window holds the prior values, the row padding stays sentinel.  W: everything outside the K1 x A views -- columns
A .. w_c - 1, the gap between terms, four more rows behind the last view, the guards -- is NaN: the kernels load W masked,
and one unmasked element makes a column of C NaN.  S: everything outside the J x K1 views is 1e300: the kernels read a row on
to whole runs of k-blocks against exact zeros (0 * 1e300 == 0), a read that meets a nonzero partner is off by hundreds of
orders of magnitude.  nan_gap: the s_gap doubles between two terms are NaN instead, and ONLY they.  csrc/stream_small.h
documents that the last row of every term but the last reads them when K1 is not a whole run of k-blocks, so the expected
result is: row J - 1 of C all NaN, every other row as the truth says.  (The driver zeroes that double before it launches.)

Integer pass: S, W hold integers in [-3, 3], a prior C integers in [-100, 100]; every partial sum is below 9 nb K1 + 100 <
2^53, so the fp64 result is exact in any order: C must EQUAL the int64 einsum (signed zeros are not told apart).
Gaussian pass: standard normal operands, truth in np.longdouble,
    |C - ref| <= C_BOUND (m + 2) 2^-53 (sum |s| |w| + |prior|),   m = K1 (ss) or nb K1 (sss), plus 1 with acc
with C_BOUND = 2 (tests/chain_step_ref.py): any order of the m additions is within gamma_m of the magnitude sum up to
second-order terms.  Then the Frobenius ratio against 1e-12."""
from collections import namedtuple

import numpy as np

from tests.edge_kit import C_BOUND, LD, PAD, SENT, assert_guards, assert_untouched, bounded, exact, sentinel_buffer, strided  # noqa: F401

PRE = POST = 64
FROB = 1e-12
KINDS = {"ss": "ttsk_psi_stream", "sss": "ttsk_psi_stream_sum"}
BUDGET = 5e8            # multiply-adds of a case: about 3 s of long-double arithmetic on one core
W_MORE = 4              # rows of NaN behind the last W view

Case = namedtuple("Case", "id kind nb J K1 A opts")
SS_STRUCTURES = [(nf, st) for nf in range(1, 8) for st in range(3) if nf + (1 if st else 0) <= 7]
SSS_STRUCTURES = [(nf, st) for nf in range(1, 4) for st in range(3)]


# ------------------------------------------------------------------------------------------------ the table
def plain_cases():
    P = lambda id, nb=1, J=1024, K1=8, A=20, **o: Case("p-" + id, "ss", nb, J, K1, A, o)
    # every instantiation: one chunk of exactly 16 nf + 4 str columns; K1 = 7 runs of 5 k-blocks, K1 = 81 runs of 25
    c = [P("s%d%d-K%d" % (nf, st, K1), K1=K1, A=16 * nf + 4 * st) for nf, st in SS_STRUCTURES for K1 in (7, 81)]
    c += [P("A%d" % A, A=A) for A in (9, 12, 17, 21, 24, 25, 112, 113, 130, 1792)]      # narrowest; 1, 5, 8, 9 past a tile; one / two chunks; short last chunk; widest
    c += [P("K%d" % K1, K1=K1) for K1 in (1, 3, 4, 5, 20, 21, 80, 100, 101)] + [P("K600-A64", K1=600, A=64)]
    c += [P("J%d" % J, J=J) for J in (1025, 1039, 1041)]
    c += [P("nb2", nb=2), P("nb32", nb=32), P("nb32-wrap", nb=32, J=1107), P("nb5-A130", nb=5, A=130, J=1041), P("nb32-A130", nb=32, A=130)]
    c += [P("pads", s_pad=3, w_pad=5, c_pad=7), P("acc", acc=1), P("pads-acc", nb=2, J=1025, K1=5, A=17, s_pad=3, w_pad=5, c_pad=7, acc=1),
          P("A113-pads-acc", A=113, K1=21, J=1039, s_pad=1, w_pad=2, c_pad=3, acc=1)]
    return c


def sum_cases():
    S = lambda id, nb=2, J=1024, K1=8, A=32, **o: Case("s-" + id, "sss", nb, J, K1, A, o)
    # every instantiation.  One full tile and its strips: two chunks of a narrow A (a third chunk would be under 16 columns).  Wider
    # structures: the chunks stop growing at 16 where a 17th no longer fits the chip in one round, J = 2049 on 256 compute units.
    small = {(1, 0): 32, (1, 1): 40, (1, 2): 45}
    c = []
    for nf, st in SSS_STRUCTURES:
        for K1 in (7, 81):
            if (nf, st) in small:
                c.append(S("s%d%d-K%d" % (nf, st, K1), K1=K1, A=small[(nf, st)]))
            else:
                c.append(S("s%d%d-K%d" % (nf, st, K1), K1=K1, J=2049, A=16 * (16 * nf + 4 * st) - (3 if K1 == 7 else 0)))
    c += [S("A%d" % A, A=A) for A in (17, 33, 47, 48, 64, 113, 128, 896)]
    c += [S("K%d" % K1, K1=K1) for K1 in (1, 3, 4, 5, 20, 21, 80, 100, 101, 380)]
    c += [S("J%d" % J, J=J) for J in (1025, 1039, 1041)] + [S("J1025-A128", J=1025, A=128)]
    c += [S("nb3", nb=3, K1=5, A=17), S("nb8", nb=8, K1=21)]
    c += [S("pads", s_pad=3, w_pad=5, c_pad=7), S("gaps", nb=3, s_gap=5, w_gap=3), S("acc", acc=1),
          S("pads-acc", nb=3, J=1025, K1=5, A=33, s_pad=3, w_pad=5, c_pad=7, s_gap=9, w_gap=11, acc=1)]
    c += [S("nangap-K49", nb=3, J=1025, K1=49, A=33, s_gap=1, nan_gap=1), S("nangap-K97", nb=3, K1=97, A=40, s_gap=1, nan_gap=1, acc=1)]
    return c


def refusals():
    """the far side of each cover limit: the plan must refuse, nothing may be written"""
    R = lambda id, kind, nb=2, J=1024, K1=8, A=32, **o: Case("x-" + id, kind, nb, J, K1, A, dict(o, refuse=1))
    return [R("p-J1023", "ss", J=1023), R("p-A8", "ss", A=8), R("p-A1793", "ss", A=1793), R("p-nb0", "ss", nb=0), R("p-nb33", "ss", nb=33),
            R("p-sj", "ss", s_pad=-1), R("p-wc", "ss", w_pad=-1), R("p-cj", "ss", c_pad=-1),
            R("s-J1023", "sss", J=1023), R("s-A16", "sss", A=16), R("s-A897", "sss", A=897), R("s-nb1", "sss", nb=1), R("s-K381", "sss", K1=381),
            R("s-sj", "sss", s_pad=-1), R("s-wc", "sss", w_pad=-1), R("s-cj", "sss", c_pad=-1), R("s-sb", "sss", s_b=-1)]


def all_cases():
    return plain_cases() + sum_cases()


OPTIONS = {"ss": ("s_pad", "w_pad", "c_pad", "acc"), "sss": ("s_pad", "w_pad", "c_pad", "acc", "s_gap", "w_gap", "nan_gap")}

# the values of each plan field the table must reach (256 compute units)
BRANCHES = {"ss": {"unr": "5 25", "nac": "1 2 16", "wpp": "4 8 9", "short": "0 1"},
            "sss": {"unr": "5 25", "nac": "2 3 4 8 16", "xcd_map": "0 1", "short": "0 1"}}


def geometry(c):
    o = c.opts
    g = dict(s_j=o.get("s_j", c.K1 + o.get("s_pad", 0)), w_c=o.get("w_c", c.A + o.get("w_pad", 0)), c_j=o.get("c_j", c.A + o.get("c_pad", 0)))
    g["s_alloc"], g["w_alloc"], g["c_alloc"] = max(g["s_j"], c.K1), max(g["w_c"], c.A), max(g["c_j"], c.A)      # a refused stride still gets a sane buffer
    g["s_b"] = o.get("s_b", c.J * g["s_alloc"] + o.get("s_gap", 0)) if c.kind == "sss" else 0
    g["w_b"] = c.K1 * g["w_alloc"] + o.get("w_gap", 0) if c.kind == "sss" else 0
    return g


def plan_call(c):
    """the case as a call of tests/test_psi_plan.py's driver"""
    g = geometry(c)
    return [c.kind, c.nb, c.J, c.K1, c.A, g["s_j"], g["w_c"], g["c_j"], g["s_b"], g["w_b"], int(bool(c.opts.get("acc"))), 0]


def plan_calls():
    return [(c.id, plan_call(c)) for c in all_cases() + refusals()]


def tags_of_plan(kind, f):
    """the tag string of a plan record (the driver's fields): `short` = the last column chunk is narrower than the others"""
    A, nac, ac = int(f["a.A"]), int(f["a.nac"]), int(f["a.ac"])
    short = 1 if nac > 1 and A - (nac - 1) * ac < ac else 0
    geo = "wpp=%s" % f["a.wpp"] if kind == "ss" else "groups=%s xcd_map=%s" % (f["a.groups"], f["a.xcd_map"])
    return "nf=%s str=%s unr=%s nac=%d ac=%d short=%d %s" % (f["nf"], f["str"], f["unr"], nac, ac, short, geo)


def expected_name(c):
    t = dict(kv.split("=") for kv in TAGS[c.id].split())
    return "stream_small%s_kernel<%s, %s, 5, %s>" % ("_sum" if c.kind == "sss" else "", t["nf"], t["str"], t["unr"])


def macs(c):
    return c.nb * c.J * c.K1 * c.A


# What each accepted case is meant to reach: the plan's fields at 256 compute units (tests/test_psi_plan.py asserts every one
# of them against psi_stream_plan / psi_stream_sum_plan).
TAGS = {
    "p-s10-K7": "nf=1 str=0 unr=5 nac=1 ac=16 short=0 wpp=8",
    "p-s10-K81": "nf=1 str=0 unr=25 nac=1 ac=16 short=0 wpp=8",
    "p-s11-K7": "nf=1 str=1 unr=5 nac=1 ac=20 short=0 wpp=8",
    "p-s11-K81": "nf=1 str=1 unr=25 nac=1 ac=20 short=0 wpp=8",
    "p-s12-K7": "nf=1 str=2 unr=5 nac=1 ac=24 short=0 wpp=8",
    "p-s12-K81": "nf=1 str=2 unr=25 nac=1 ac=24 short=0 wpp=8",
    "p-s20-K7": "nf=2 str=0 unr=5 nac=1 ac=32 short=0 wpp=8",
    "p-s20-K81": "nf=2 str=0 unr=25 nac=1 ac=32 short=0 wpp=8",
    "p-s21-K7": "nf=2 str=1 unr=5 nac=1 ac=36 short=0 wpp=8",
    "p-s21-K81": "nf=2 str=1 unr=25 nac=1 ac=36 short=0 wpp=8",
    "p-s22-K7": "nf=2 str=2 unr=5 nac=1 ac=40 short=0 wpp=8",
    "p-s22-K81": "nf=2 str=2 unr=25 nac=1 ac=40 short=0 wpp=8",
    "p-s30-K7": "nf=3 str=0 unr=5 nac=1 ac=48 short=0 wpp=8",
    "p-s30-K81": "nf=3 str=0 unr=25 nac=1 ac=48 short=0 wpp=8",
    "p-s31-K7": "nf=3 str=1 unr=5 nac=1 ac=52 short=0 wpp=8",
    "p-s31-K81": "nf=3 str=1 unr=25 nac=1 ac=52 short=0 wpp=8",
    "p-s32-K7": "nf=3 str=2 unr=5 nac=1 ac=56 short=0 wpp=8",
    "p-s32-K81": "nf=3 str=2 unr=25 nac=1 ac=56 short=0 wpp=8",
    "p-s40-K7": "nf=4 str=0 unr=5 nac=1 ac=64 short=0 wpp=8",
    "p-s40-K81": "nf=4 str=0 unr=25 nac=1 ac=64 short=0 wpp=8",
    "p-s41-K7": "nf=4 str=1 unr=5 nac=1 ac=68 short=0 wpp=8",
    "p-s41-K81": "nf=4 str=1 unr=25 nac=1 ac=68 short=0 wpp=8",
    "p-s42-K7": "nf=4 str=2 unr=5 nac=1 ac=72 short=0 wpp=8",
    "p-s42-K81": "nf=4 str=2 unr=25 nac=1 ac=72 short=0 wpp=8",
    "p-s50-K7": "nf=5 str=0 unr=5 nac=1 ac=80 short=0 wpp=8",
    "p-s50-K81": "nf=5 str=0 unr=25 nac=1 ac=80 short=0 wpp=8",
    "p-s51-K7": "nf=5 str=1 unr=5 nac=1 ac=84 short=0 wpp=8",
    "p-s51-K81": "nf=5 str=1 unr=25 nac=1 ac=84 short=0 wpp=8",
    "p-s52-K7": "nf=5 str=2 unr=5 nac=1 ac=88 short=0 wpp=8",
    "p-s52-K81": "nf=5 str=2 unr=25 nac=1 ac=88 short=0 wpp=8",
    "p-s60-K7": "nf=6 str=0 unr=5 nac=1 ac=96 short=0 wpp=8",
    "p-s60-K81": "nf=6 str=0 unr=25 nac=1 ac=96 short=0 wpp=8",
    "p-s61-K7": "nf=6 str=1 unr=5 nac=1 ac=100 short=0 wpp=8",
    "p-s61-K81": "nf=6 str=1 unr=25 nac=1 ac=100 short=0 wpp=8",
    "p-s62-K7": "nf=6 str=2 unr=5 nac=1 ac=104 short=0 wpp=8",
    "p-s62-K81": "nf=6 str=2 unr=25 nac=1 ac=104 short=0 wpp=8",
    "p-s70-K7": "nf=7 str=0 unr=5 nac=1 ac=112 short=0 wpp=8",
    "p-s70-K81": "nf=7 str=0 unr=25 nac=1 ac=112 short=0 wpp=8",
    "p-A9": "nf=1 str=0 unr=5 nac=1 ac=9 short=0 wpp=8",
    "p-A12": "nf=1 str=0 unr=5 nac=1 ac=12 short=0 wpp=8",
    "p-A17": "nf=1 str=1 unr=5 nac=1 ac=17 short=0 wpp=8",
    "p-A21": "nf=1 str=2 unr=5 nac=1 ac=21 short=0 wpp=8",
    "p-A24": "nf=1 str=2 unr=5 nac=1 ac=24 short=0 wpp=8",
    "p-A25": "nf=2 str=0 unr=5 nac=1 ac=25 short=0 wpp=8",
    "p-A112": "nf=7 str=0 unr=5 nac=1 ac=112 short=0 wpp=8",
    "p-A113": "nf=4 str=0 unr=5 nac=2 ac=60 short=1 wpp=8",
    "p-A130": "nf=4 str=1 unr=5 nac=2 ac=68 short=1 wpp=8",
    "p-A1792": "nf=7 str=0 unr=5 nac=16 ac=112 short=0 wpp=8",
    "p-K1": "nf=1 str=1 unr=5 nac=1 ac=20 short=0 wpp=8",
    "p-K3": "nf=1 str=1 unr=5 nac=1 ac=20 short=0 wpp=8",
    "p-K4": "nf=1 str=1 unr=5 nac=1 ac=20 short=0 wpp=8",
    "p-K5": "nf=1 str=1 unr=5 nac=1 ac=20 short=0 wpp=8",
    "p-K20": "nf=1 str=1 unr=5 nac=1 ac=20 short=0 wpp=8",
    "p-K21": "nf=1 str=1 unr=5 nac=1 ac=20 short=0 wpp=8",
    "p-K80": "nf=1 str=1 unr=5 nac=1 ac=20 short=0 wpp=8",
    "p-K100": "nf=1 str=1 unr=25 nac=1 ac=20 short=0 wpp=8",
    "p-K101": "nf=1 str=1 unr=5 nac=1 ac=20 short=0 wpp=8",
    "p-K600-A64": "nf=2 str=0 unr=25 nac=2 ac=32 short=0 wpp=8",
    "p-J1025": "nf=1 str=1 unr=5 nac=1 ac=20 short=0 wpp=9",
    "p-J1039": "nf=1 str=1 unr=5 nac=1 ac=20 short=0 wpp=9",
    "p-J1041": "nf=1 str=1 unr=5 nac=1 ac=20 short=0 wpp=9",
    "p-nb2": "nf=1 str=1 unr=5 nac=1 ac=20 short=0 wpp=8",
    "p-nb32": "nf=1 str=1 unr=5 nac=1 ac=20 short=0 wpp=8",
    "p-nb32-wrap": "nf=1 str=1 unr=5 nac=1 ac=20 short=0 wpp=8",
    "p-nb5-A130": "nf=4 str=1 unr=5 nac=2 ac=68 short=1 wpp=9",
    "p-nb32-A130": "nf=4 str=1 unr=5 nac=2 ac=68 short=1 wpp=4",
    "p-pads": "nf=1 str=1 unr=5 nac=1 ac=20 short=0 wpp=8",
    "p-acc": "nf=1 str=1 unr=5 nac=1 ac=20 short=0 wpp=8",
    "p-pads-acc": "nf=1 str=1 unr=5 nac=1 ac=17 short=0 wpp=9",
    "p-A113-pads-acc": "nf=4 str=0 unr=5 nac=2 ac=60 short=1 wpp=9",
    "s-s10-K7": "nf=1 str=0 unr=5 nac=2 ac=16 short=0 groups=8 xcd_map=1",
    "s-s10-K81": "nf=1 str=0 unr=25 nac=2 ac=16 short=0 groups=8 xcd_map=1",
    "s-s11-K7": "nf=1 str=1 unr=5 nac=2 ac=20 short=0 groups=8 xcd_map=1",
    "s-s11-K81": "nf=1 str=1 unr=25 nac=2 ac=20 short=0 groups=8 xcd_map=1",
    "s-s12-K7": "nf=1 str=2 unr=5 nac=2 ac=24 short=1 groups=8 xcd_map=1",
    "s-s12-K81": "nf=1 str=2 unr=25 nac=2 ac=24 short=1 groups=8 xcd_map=1",
    "s-s20-K7": "nf=2 str=0 unr=5 nac=16 ac=32 short=1 groups=17 xcd_map=1",
    "s-s20-K81": "nf=2 str=0 unr=25 nac=16 ac=32 short=0 groups=17 xcd_map=1",
    "s-s21-K7": "nf=2 str=1 unr=5 nac=16 ac=36 short=1 groups=17 xcd_map=1",
    "s-s21-K81": "nf=2 str=1 unr=25 nac=16 ac=36 short=0 groups=17 xcd_map=1",
    "s-s22-K7": "nf=2 str=2 unr=5 nac=16 ac=40 short=1 groups=17 xcd_map=1",
    "s-s22-K81": "nf=2 str=2 unr=25 nac=16 ac=40 short=0 groups=17 xcd_map=1",
    "s-s30-K7": "nf=3 str=0 unr=5 nac=16 ac=48 short=1 groups=17 xcd_map=1",
    "s-s30-K81": "nf=3 str=0 unr=25 nac=16 ac=48 short=0 groups=17 xcd_map=1",
    "s-s31-K7": "nf=3 str=1 unr=5 nac=16 ac=52 short=1 groups=17 xcd_map=1",
    "s-s31-K81": "nf=3 str=1 unr=25 nac=16 ac=52 short=0 groups=17 xcd_map=1",
    "s-s32-K7": "nf=3 str=2 unr=5 nac=16 ac=56 short=1 groups=17 xcd_map=1",
    "s-s32-K81": "nf=3 str=2 unr=25 nac=16 ac=56 short=0 groups=17 xcd_map=1",
    "s-A17": "nf=1 str=0 unr=5 nac=2 ac=12 short=1 groups=8 xcd_map=1",
    "s-A33": "nf=1 str=1 unr=5 nac=2 ac=20 short=1 groups=8 xcd_map=1",
    "s-A47": "nf=1 str=0 unr=5 nac=3 ac=16 short=1 groups=8 xcd_map=1",
    "s-A48": "nf=1 str=0 unr=5 nac=3 ac=16 short=0 groups=8 xcd_map=1",
    "s-A64": "nf=1 str=0 unr=5 nac=4 ac=16 short=0 groups=8 xcd_map=1",
    "s-A113": "nf=1 str=1 unr=5 nac=6 ac=20 short=1 groups=8 xcd_map=1",
    "s-A128": "nf=1 str=0 unr=5 nac=8 ac=16 short=0 groups=8 xcd_map=1",
    "s-A896": "nf=2 str=0 unr=5 nac=32 ac=28 short=0 groups=8 xcd_map=1",
    "s-K1": "nf=1 str=0 unr=5 nac=2 ac=16 short=0 groups=8 xcd_map=1",
    "s-K3": "nf=1 str=0 unr=5 nac=2 ac=16 short=0 groups=8 xcd_map=1",
    "s-K4": "nf=1 str=0 unr=5 nac=2 ac=16 short=0 groups=8 xcd_map=1",
    "s-K5": "nf=1 str=0 unr=5 nac=2 ac=16 short=0 groups=8 xcd_map=1",
    "s-K20": "nf=1 str=0 unr=5 nac=2 ac=16 short=0 groups=8 xcd_map=1",
    "s-K21": "nf=1 str=0 unr=5 nac=2 ac=16 short=0 groups=8 xcd_map=1",
    "s-K80": "nf=1 str=0 unr=5 nac=2 ac=16 short=0 groups=8 xcd_map=1",
    "s-K100": "nf=1 str=0 unr=25 nac=2 ac=16 short=0 groups=8 xcd_map=1",
    "s-K101": "nf=1 str=0 unr=5 nac=2 ac=16 short=0 groups=8 xcd_map=1",
    "s-K380": "nf=1 str=0 unr=5 nac=2 ac=16 short=0 groups=8 xcd_map=1",
    "s-J1025": "nf=1 str=0 unr=5 nac=2 ac=16 short=0 groups=9 xcd_map=0",
    "s-J1039": "nf=1 str=0 unr=5 nac=2 ac=16 short=0 groups=9 xcd_map=0",
    "s-J1041": "nf=1 str=0 unr=5 nac=2 ac=16 short=0 groups=9 xcd_map=0",
    "s-J1025-A128": "nf=1 str=0 unr=5 nac=8 ac=16 short=0 groups=9 xcd_map=1",
    "s-nb3": "nf=1 str=0 unr=5 nac=2 ac=12 short=1 groups=8 xcd_map=1",
    "s-nb8": "nf=1 str=0 unr=5 nac=2 ac=16 short=0 groups=8 xcd_map=1",
    "s-pads": "nf=1 str=0 unr=5 nac=2 ac=16 short=0 groups=8 xcd_map=1",
    "s-gaps": "nf=1 str=0 unr=5 nac=2 ac=16 short=0 groups=8 xcd_map=1",
    "s-acc": "nf=1 str=0 unr=5 nac=2 ac=16 short=0 groups=8 xcd_map=1",
    "s-pads-acc": "nf=1 str=1 unr=5 nac=2 ac=20 short=1 groups=9 xcd_map=0",
    "s-nangap-K49": "nf=1 str=1 unr=5 nac=2 ac=20 short=1 groups=9 xcd_map=0",
    "s-nangap-K97": "nf=1 str=1 unr=25 nac=2 ac=20 short=0 groups=8 xcd_map=1",
}


# ------------------------------------------------------------------------------------------------ values and truth
def values(c, integer, seed):
    """([S_b] (J x K1), [W_b] (K1 x A), [prior C] or None): one prior per result"""
    rng = np.random.default_rng(seed)
    nres = c.nb if c.kind == "ss" else 1
    if integer:
        S = [rng.integers(-3, 4, (c.J, c.K1)).astype(np.float64) for _ in range(c.nb)]
        W = [rng.integers(-3, 4, (c.K1, c.A)).astype(np.float64) for _ in range(c.nb)]
        prior = [rng.integers(-100, 101, (c.J, c.A)).astype(np.float64) for _ in range(nres)]
    else:
        S = [rng.standard_normal((c.J, c.K1)) for _ in range(c.nb)]
        W = [rng.standard_normal((c.K1, c.A)) for _ in range(c.nb)]
        prior = [rng.standard_normal((c.J, c.A)) for _ in range(nres)]
    return S, W, (prior if c.opts.get("acc") else None)


def _terms(c):
    """the (S, W) index lists that meet in each result"""
    return [[b] for b in range(c.nb)] if c.kind == "ss" else [list(range(c.nb))]


def truth(c, vals, integer):
    """Per result: integer pass -- the int64 einsum as float64 (exact).  Gaussian pass -- the long-double result as a pair of
    doubles hi + lo and the element-wise bound.  Computed once per (case, pass) and shared by every call of it."""
    S, W, prior = vals
    hi, lo, tol = [], [], []
    for r, bs in enumerate(_terms(c)):
        if integer:
            t = sum(S[b].astype(np.int64) @ W[b].astype(np.int64) for b in bs)
            if prior is not None:
                t = t + prior[r].astype(np.int64)
            assert 9 * len(bs) * c.K1 + 100 < 2 ** 53
            hi.append(t.astype(np.float64)); lo.append(None); tol.append(None)
            continue
        t = sum(S[b].astype(LD) @ W[b].astype(LD) for b in bs)
        mag = sum(np.abs(S[b]) @ np.abs(W[b]) for b in bs)
        m = len(bs) * c.K1
        if prior is not None:
            t, mag, m = t + prior[r].astype(LD), mag + np.abs(prior[r]), m + 1
        h = t.astype(np.float64)
        hi.append(h); lo.append((t - h.astype(LD)).astype(np.float64)); tol.append(C_BOUND * (m + 2) * 2.0 ** -53 * mag)
    return dict(C=hi, C_lo=lo, C_tol=tol)


# ------------------------------------------------------------------------------------------------ buffers
def operands(c, vals):
    """host images of the S and W buffers, guards included: ([S buffers], [W buffers]); every base sits at PRE.  ss: one
    buffer per problem, sss: one buffer holding all terms"""
    g = geometry(c)
    S, W, _ = vals
    sj, wc = g["s_alloc"], g["w_alloc"]
    if c.kind == "ss":
        hS, hW = [], []
        for b in range(c.nb):
            s = np.full(PRE + c.J * sj + POST, PAD)
            strided(s, PRE, (c.J, c.K1), (sj, 1))[...] = S[b]
            w = np.full(PRE + (c.K1 + W_MORE) * wc + POST, np.nan)
            strided(w, PRE, (c.K1, c.A), (wc, 1))[...] = W[b]
            hS.append(s); hW.append(w)
        return hS, hW
    sb, wb = max(g["s_b"], 0), g["w_b"]
    s = np.full(PRE + (c.nb - 1) * sb + c.J * sj + POST, PAD)
    w = np.full(PRE + (c.nb - 1) * wb + (c.K1 + W_MORE) * wc + POST, np.nan)
    if c.opts.get("nan_gap"):
        for b in range(c.nb - 1):
            s[PRE + b * sb + c.J * sj:PRE + (b + 1) * sb] = np.nan
    for b in range(c.nb):
        strided(s, PRE + b * sb, (c.J, c.K1), (sj, 1))[...] = S[b]
        strided(w, PRE + b * wb, (c.K1, c.A), (wc, 1))[...] = W[b]
    return [s], [w]


def c_views(c, bufs):
    g = geometry(c)
    return [strided(x, PRE, (c.J, c.A), (g["c_alloc"], 1)) for x in bufs]


def sentinels(c, vals=None):
    """host images of the C buffers before a call: the sentinel everywhere, the prior values in the window of an accumulating call"""
    g = geometry(c)
    nres = max(c.nb, 1) if c.kind == "ss" else 1
    out = [sentinel_buffer(c.J * g["c_alloc"], PRE, POST) for _ in range(min(nres, 33))]
    if vals is not None and vals[2] is not None:
        for v, p in zip(c_views(c, out), vals[2]):
            v[...] = p
    return out


# ------------------------------------------------------------------------------------------------ the checks
def check_guards(c, out, what):
    """every element of the C buffers outside the J x A windows still holds the sentinel"""
    g = geometry(c)
    for b, o in enumerate(out):
        assert_guards(o, [(PRE, (c.J, c.A), (g["c_alloc"], 1))], "%s C[%d]" % (what, b))


def check_untouched(c, out, what):
    """a refused call: nothing written at all"""
    assert_untouched(out, what + " C")


def check_results(c, out, tr, integer, what=""):
    """The C buffers of one call (host images after it) against the truth `tr` of truth(); guards included.  Returns the largest
    |err| / bound (Gaussian pass; 0 in the integer pass, where nothing but equality passes).  A nan_gap case: row J - 1 must be
    NaN in every column, the rows above are checked as usual."""
    what = "%s %s (%s pass)" % (what, c.id, "integer" if integer else "Gaussian")
    check_guards(c, out, what)
    worst = 0.0
    rows = c.J - 1 if c.opts.get("nan_gap") else c.J
    for r, got in enumerate(c_views(c, out)):
        if rows < c.J:
            assert np.isnan(got[rows:, :]).all(), "%s: row %d of C[%d] is not NaN throughout: the gap behind a term was not read as documented" % (what, rows, r)
        if integer:
            exact(got[:rows], tr["C"][r][:rows], "%s C[%d]" % (what, r))
        else:
            worst = max(worst, bounded(got[:rows], tr["C"][r][:rows], tr["C_lo"][r][:rows], tr["C_tol"][r][:rows], "%s C[%d]" % (what, r), FROB))
    return worst


def float64_result(c, vals):
    """what a correct kernel may return (the finite result also of a nan_gap case): float64 products in guarded buffers"""
    S, W, prior = vals
    out = sentinels(c, vals)
    for r, (v, bs) in enumerate(zip(c_views(c, out), _terms(c))):
        t = sum(S[b] @ W[b] for b in bs)
        v[...] = t + prior[r] if prior is not None else t
    return out
