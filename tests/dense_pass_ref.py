"""Reference, guarded operands and case tables for the two passes over a dense tensor -- dense_pass_kernel
(ttsk_dense_first_pass) and dense_left_pass_kernel (ttsk_dense_left_pass).  Plain module, no GPU:
tests/test_dense_pass_cover.py runs the tables through the host plans (csrc/dense_pass_plan.h) and tests the checker on
seeded defects, tests/test_gpu_dense_pass_edges.py runs every case on the device.

First pass (dense_sketch.py:7-52 with the matrices of tensor_train_drm.py:109-122), a case is (n0, Q, T, ll, r):
    Z[p', q, t] = sum_b C[b, p'] X[b, q, t]                U[b, p, t] = sum_q P[q, p] X[b, q, t]
Left pass (the matrices of dense_gaussian_drm.py:77-80), a case is (n0, n1, n2, n3, n4, l), X (n0, n1, n2, n3, n4):
    Z_mu = A_mu X^{<mu+1>}, mu = 0, 1, 2             E3[a, i3, i4] = sum_{i0 i1 i2} A_3[a, (i0, i1, i2, i3)] X[i0, i1, i2, i3, i4]
(E3 still holds i3: Z_3 is its sum over i3, the caller's; every element of E3 is compared here, not that sum).

Buffers.  Every array sits in a buffer of its own with PRE = POST = 64 guard elements around it, all of them the sentinel
-1/3 (finite, no multiple of 1/2).  The outputs are the sentinel throughout before a call: an unwritten element fails the
integer pass, a stray store changes a guard.  The guards of an operand are what a read beyond it meets: -1/3 times an
integer is no integer.  Option uoff / coff: U / C start that many elements into their buffers (8 bytes off a 16-byte
boundary: accepted); xoff / poff / zoff: the same for X / P / Z (refused).

Integer pass: every operand holds integers in [-4, 4]; a partial sum is at most 16 K < 2^53, so the fp64 result is exact
in any order -- q chunks, slabs, blocks of rows included: the results must EQUAL the int64 einsum.
Gaussian pass: standard normal operands, truth in np.longdouble, every element within
    |got - ref| <= C_BOUND (K + 3) 2^-53 (|A| |B|)_ij,     C_BOUND = 2 (the argument of tests/test_gpu_gemm_families.py),
K the number of products of that element: n0 for Z, Q for U, n0 / n0 n1 / n0 n1 n2 / n0 n1 n2 for Z_0, Z_1, Z_2, E3 --
chunked and slab sums are another order of the same terms.  (The magnitude products are formed in float64: sums of
non-negative terms, right to a few 2^-53 of themselves, which moves the bound by less than 1e-13 of itself.)  Then the
Frobenius ratio against 1e-13, as that file has it.

Poison.  Both entry points keep partial sums in the library's grow-only scratch.  Before a case the GPU test calls the same
entry point on POISON_FIRST / POISON_LEFT with X scaled by 2^500: finite results, and scratch that now holds huge values
wherever the case may read what it did not write itself.  For that the poison call must itself write a huge value to
every element of its scratch: the cover test shows that in the poison plans every q chunk owns a tile, every slot of
the slab is a column of U in use and every row of the partial Z a row in use (left pass: l = 20, every row of the slabs),
and that no case needs more scratch than its poison shape (a larger request would be served from fresh memory)."""
from collections import namedtuple

import numpy as np

from tests.edge_kit import C_BOUND, LD, SENT, assert_guards, assert_untouched, bounded, exact, guarded, sentinel_buffer  # noqa: F401

PRE = POST = 64
FROB = 1e-13
ENTRY = {"first": "ttsk_dense_first_pass", "left": "ttsk_dense_left_pass"}

First = namedtuple("First", "id n0 Q T ll r opts")
Left = namedtuple("Left", "id n0 n1 n2 n3 n4 l opts")
First.kind = "first"
Left.kind = "left"


# ------------------------------------------------------------------------------------------------ the tables
def first_cases():
    F = lambda id, n0=64, Q=16, T=16, ll=20, r=40, **o: First("d-" + id, n0, Q, T, ll, r, o)
    # whole blocks of 64 rows: the rank edges r = 40 | 41 .. 44 | 45 .. 48 | 49 .. 64, ll = 20 | 21 .. 24 | 25 .. 32
    c = [F("r%d" % r, r=r) for r in (1, 33, 39, 40, 41, 43, 44, 45, 47, 48, 49, 57, 64)]
    c += [F("l%d" % ll, ll=ll) for ll in (1, 17, 21, 24, 25, 32)]
    c += [F("l%d-r%d" % lr, ll=lr[0], r=lr[1]) for lr in ((1, 1), (24, 44), (24, 48), (25, 48), (24, 49), (25, 49), (32, 64),
                                                         (1, 45), (1, 64), (25, 1), (32, 1), (29, 57), (21, 45), (17, 33))]
    # blocks of 32 rows
    c += [F("n32-l%d-r%d" % lr, n0=32, ll=lr[0], r=lr[1]) for lr in ((20, 40), (21, 40), (32, 39), (20, 41), (20, 47), (21, 48), (20, 49),
                                                                    (32, 64), (32, 63), (1, 1), (17, 33))]
    # blocks of rows: one and several, of 32 and of 64; a split over several blocks; the longest first mode
    c += [F("n96", n0=96), F("n96-l21-r49", n0=96, ll=21, r=49), F("n128", n0=128), F("n128-l25-r49", n0=128, ll=25, r=49),
          F("n128-l21-r41", n0=128, ll=21, r=41), F("n4096", n0=4096, Q=8)]
    # q ranges: seven empty chunks; nine tiles in eight chunks; three tiles per chunk, walked from a rotated start; chunks
    # as the grid wants them (not capped by the tiles)
    c += [F("Q8", Q=8), F("n32-Q8", n0=32, Q=8), F("Q72-T272", n0=32, Q=72, T=272), F("Q192-T272", n0=32, Q=192, T=272),
          F("Q512-T64", n0=32, Q=512, T=64), F("Q192-T272-l25-r49", n0=64, Q=192, T=272, ll=25, r=49)]
    # t ranges: three (no power of two in the block-id decode), more than 32, and many blocks of rows times t ranges
    c += [F("T48", T=48), F("n32-T48", n0=32, T=48), F("T528", n0=32, Q=8, T=528), F("n96-T48", n0=96, T=48, Q=24),
          F("n1376-T96", n0=1376, Q=8, T=96)]
    # U and C 8 bytes off a 16-byte boundary
    c += [F("off8", uoff=1, coff=1), F("off8-l25-r49", ll=25, r=49, uoff=1, coff=1), F("n96-off8-r41", n0=96, r=41, uoff=1, coff=1)]
    return c


def first_refusals():
    R = lambda id, n0=32, Q=16, T=16, ll=20, r=40, **o: First("x-" + id, n0, Q, T, ll, r, dict(o, refuse=1))
    return [R("n48", n0=48), R("n4128", n0=4128), R("T24", T=24), R("Q10", Q=10), R("l33", ll=33), R("r65", r=65),
            R("QT27", Q=1 << 11, T=1 << 16, dummy=1), R("partials", n0=64 * 40, Q=8 * 1024, T=128, dummy=1, msg="partial"),
            R("xoff8", xoff=1), R("poff8", poff=1), R("zoff8", zoff=1)]


def left_cases():
    L = lambda id, n0, n1, n2, n3, n4, l, **o: Left("e-" + id, n0, n1, n2, n3, n4, l, o)
    return [L("l1", 4, 1, 1, 8, 64, 1), L("l16", 12, 2, 3, 8, 128, 16), L("l17", 4, 2, 8, 2, 256, 17), L("l20", 12, 3, 16, 1, 512, 20),
            L("n4-64-ct2", 8, 2, 3, 16, 64, 20), L("xcd-ct2", 4, 1, 8, 4, 256, 7), L("n4-512-ct2", 8, 1, 16, 2, 512, 17),
            L("n1-5", 4, 5, 1, 4, 128, 20), L("kb3", 12, 1, 3, 8, 64, 16)]


def left_refusals():
    R = lambda id, n0=8, n1=2, n2=2, n3=8, n4=64, l=8, **o: Left("x-" + id, n0, n1, n2, n3, n4, l, dict(o, refuse=1))
    return [R("n6", n0=6), R("C500", n3=10, n4=50), R("n4-32", n3=16, n4=32), R("n4-48", n3=32, n4=48), R("l21", l=21),
            R("n2-big", n2=(1 << 16) + 1, dummy=1)]


def all_cases():
    return first_cases() + left_cases()


def refusals():
    return first_refusals() + left_refusals()


# First pass: Q / 8 = 8 tiles for its 8 q chunks and r = 64 = 16 TP, ll = 32 = 16 ZT -- the kernel stores its accumulators
# whether or not its chunk had a tile, so only a shape in which every chunk has one, and every accumulator column a column
# of P, leaves no zero in the slab.  43 blocks of rows: the partial Z as well.
POISON_FIRST = First("poison-first", 1376, 64, 96, 32, 64, {})
POISON_LEFT = Left("poison-left", 4, 1, 16, 2, 512, 20, {})


def _t(inst, kind, rows, pc, zr, grid="nt=1 nqc=8 cap=1 wide=- lens=0+1 rot=0"):
    """first pass; the default grid is that of Q = T = 16 with one block of rows: one t range, two tiles for eight chunks"""
    return "inst=%s kind=%s rows=%s pc=%s zr=%s %s" % (inst, kind, rows, pc, zr, grid)


_NB = "nt=1 nqc=8 cap=1 wide=0 lens=0+1 rot=0"          # the same with several blocks of rows
# What each accepted case is meant to reach: fields of the plan (tests/test_dense_pass_cover.py compares them with what
# dense_first_plan / dense_left_plan decide; tags_of_plan() below says how a plan is written as a tag string).
TAGS = {
    "d-r1": _t("8.2.2.1.1", "plain", "64x1", "1", "20"),
    "d-r33": _t("8.2.2.1.1", "plain", "64x1", "33", "20"),
    "d-r39": _t("8.2.2.1.1", "plain", "64x1", "39", "20"),
    "d-r40": _t("8.2.2.1.1", "plain", "64x1", "40", "20"),
    "d-r41": _t("8.2.3.1.2", "one", "64x1", "41", "20"),
    "d-r43": _t("8.2.3.1.2", "one", "64x1", "43", "20"),
    "d-r44": _t("8.2.3.1.2", "one", "64x1", "44", "20"),
    "d-r45": _t("8.1.2.0.3", "split", "64x1", "24+21", "12+8"),
    "d-r47": _t("8.1.2.0.3", "split", "64x1", "24+23", "12+8"),
    "d-r48": _t("8.1.2.0.3", "split", "64x1", "24+24", "12+8"),
    "d-r49": _t("8.2.0.0.3", "split", "64x1", "28+21", "12+8"),
    "d-r57": _t("8.2.0.0.3", "split", "64x1", "32+25", "12+8"),
    "d-r64": _t("8.2.0.0.3", "split", "64x1", "32+32", "12+8"),
    "d-l1": _t("8.2.2.1.1", "plain", "64x1", "40", "1"),
    "d-l17": _t("8.2.2.1.1", "plain", "64x1", "40", "17"),
    "d-l21": _t("8.2.3.1.2", "one", "64x1", "40", "21"),
    "d-l24": _t("8.2.3.1.2", "one", "64x1", "40", "24"),
    "d-l25": _t("8.1.2.1.0", "split", "64x1", "20+20", "16+9"),
    "d-l32": _t("8.1.2.1.0", "split", "64x1", "20+20", "16+16"),
    "d-l1-r1": _t("8.2.2.1.1", "plain", "64x1", "1", "1"),
    "d-l24-r44": _t("8.2.3.1.2", "one", "64x1", "44", "24"),
    "d-l24-r48": _t("8.1.2.0.3", "split", "64x1", "24+24", "12+12"),
    "d-l25-r48": _t("8.1.2.1.0", "split", "64x1", "24+24", "16+9"),
    "d-l24-r49": _t("8.2.0.0.3", "split", "64x1", "28+21", "12+12"),
    "d-l25-r49": _t("8.2.0.1.0", "split", "64x1", "28+21", "16+9"),
    "d-l32-r64": _t("8.2.0.1.0", "split", "64x1", "32+32", "16+16"),
    "d-l1-r45": _t("8.1.2.0.3", "split", "64x1", "24+21", "1+none"),
    "d-l1-r64": _t("8.2.0.0.3", "split", "64x1", "32+32", "1+none"),
    "d-l25-r1": _t("8.1.2.1.0", "split", "64x1", "1+none", "16+9"),
    "d-l32-r1": _t("8.1.2.1.0", "split", "64x1", "1+none", "16+16"),
    "d-l29-r57": _t("8.2.0.1.0", "split", "64x1", "32+25", "16+13"),
    "d-l21-r45": _t("8.1.2.0.3", "split", "64x1", "24+21", "12+9"),
    "d-l17-r33": _t("8.2.2.1.1", "plain", "64x1", "33", "17"),
    "d-n32-l20-r40": _t("4.2.2.1.1", "plain", "32x1", "40", "20"),
    "d-n32-l21-r40": _t("4.2.2.2.0", "plain", "32x1", "40", "21"),
    "d-n32-l32-r39": _t("4.2.2.2.0", "plain", "32x1", "39", "32"),
    "d-n32-l20-r41": _t("4.3.0.1.1", "plain", "32x1", "41", "20"),
    "d-n32-l20-r47": _t("4.3.0.1.1", "plain", "32x1", "47", "20"),
    "d-n32-l21-r48": _t("4.3.0.2.0", "plain", "32x1", "48", "21"),
    "d-n32-l20-r49": _t("4.4.0.1.1", "plain", "32x1", "49", "20"),
    "d-n32-l32-r64": _t("4.4.0.2.0", "plain", "32x1", "64", "32"),
    "d-n32-l32-r63": _t("4.4.0.2.0", "plain", "32x1", "63", "32"),
    "d-n32-l1-r1": _t("4.2.2.1.1", "plain", "32x1", "1", "1"),
    "d-n32-l17-r33": _t("4.2.2.1.1", "plain", "32x1", "33", "17"),
    "d-n96": _t("4.2.2.1.1", "plain", "32x3", "40", "20", _NB),
    "d-n96-l21-r49": _t("4.4.0.2.0", "plain", "32x3", "49", "21", _NB),
    "d-n128": _t("8.2.2.1.1", "plain", "64x2", "40", "20", _NB),
    "d-n128-l25-r49": _t("8.2.0.1.0", "split", "64x2", "28+21", "16+9", _NB),
    "d-n128-l21-r41": _t("8.2.3.1.2", "one", "64x2", "41", "21", _NB),
    "d-n4096": _t("8.2.2.1.1", "plain", "64x64", "40", "20", _NB),
    "d-Q8": _t("8.2.2.1.1", "plain", "64x1", "40", "20"),
    "d-n32-Q8": _t("4.2.2.1.1", "plain", "32x1", "40", "20"),
    "d-Q72-T272": _t("4.2.2.1.1", "plain", "32x1", "40", "20", "nt=17 nqc=8 cap=0 wide=- lens=1+2 rot=0"),
    "d-Q192-T272": _t("4.2.2.1.1", "plain", "32x1", "40", "20", "nt=17 nqc=8 cap=0 wide=- lens=3 rot=1"),
    "d-Q512-T64": _t("4.2.2.1.1", "plain", "32x1", "40", "20", "nt=4 nqc=64 cap=0 wide=- lens=1 rot=0"),
    "d-Q192-T272-l25-r49": _t("8.2.0.1.0", "split", "64x1", "28+21", "16+9", "nt=17 nqc=8 cap=0 wide=- lens=3 rot=1"),
    "d-T48": _t("8.2.2.1.1", "plain", "64x1", "40", "20", "nt=3 nqc=8 cap=1 wide=- lens=0+1 rot=0"),
    "d-n32-T48": _t("4.2.2.1.1", "plain", "32x1", "40", "20", "nt=3 nqc=8 cap=1 wide=- lens=0+1 rot=0"),
    "d-T528": _t("4.2.2.1.1", "plain", "32x1", "40", "20", "nt=33 nqc=8 cap=0 wide=- lens=0+1 rot=0"),
    "d-n96-T48": _t("4.2.2.1.1", "plain", "32x3", "40", "20", "nt=3 nqc=8 cap=1 wide=0 lens=0+1 rot=0"),
    "d-n1376-T96": _t("4.2.2.1.1", "plain", "32x43", "40", "20", "nt=6 nqc=8 cap=0 wide=1 lens=0+1 rot=0"),
    "d-off8": _t("8.2.2.1.1", "plain", "64x1", "40", "20"),
    "d-off8-l25-r49": _t("8.2.0.1.0", "split", "64x1", "28+21", "16+9"),
    "d-n96-off8-r41": _t("4.3.0.1.1", "plain", "32x3", "41", "20", _NB),
    "e-l1": "ni3=8 ninstr=7 nct=1 map=plain strip=0",
    "e-l16": "ni3=4 ninstr=5 nct=2 map=plain strip=0",
    "e-l17": "ni3=2 ninstr=4 nct=1 map=xcd1 strip=1",
    "e-l20": "ni3=1 ninstr=3 nct=1 map=xcd2 strip=1",
    "e-n4-64-ct2": "ni3=8 ninstr=7 nct=2 map=plain strip=1",
    "e-xcd-ct2": "ni3=2 ninstr=4 nct=2 map=xcd1 strip=0",
    "e-n4-512-ct2": "ni3=1 ninstr=3 nct=2 map=xcd2 strip=1",
    "e-n1-5": "ni3=4 ninstr=5 nct=1 map=plain strip=1",
    "e-kb3": "ni3=8 ninstr=7 nct=1 map=plain strip=0",
}

# Every value the union of the tags must reach.  inst: the twelve instantiations <NBW, TP, SP, ZT, ZS>; rows: blocks of
# NB rows, one and several; cap: q chunks as the grid wants them / cut to 8 cdiv(Q / 8, 8); wide: with several blocks of rows,
# nbb nt <= 256 / beyond (q chunks fall to 8); lens: tiles per q chunk (3: three or more); rot: a chunk of three or more
# tiles walked from its first tile / from another one; pc, zr: columns of U and rows of Z per kind (`none`: kind 1 owns
# nothing, its reduce is not launched / it stores no row of Z).
BRANCHES = {
    "first": {"inst": "8.2.2.1.1 8.2.3.1.2 8.1.2.0.3 8.1.2.1.0 8.2.0.0.3 8.2.0.1.0 4.2.2.1.1 4.2.2.2.0 4.3.0.1.1 4.3.0.2.0 4.4.0.1.1 4.4.0.2.0",
              "kind": "plain one split", "rows": "32x1 32x3 64x1 64x2 64x64", "nt": "1 3 33", "cap": "0 1", "wide": "- 0 1",
              "lens": "0+1 1+2 3", "rot": "0 1", "pc": "1+none 32+32", "zr": "1+none 16+16"},
    "left": {"ni3": "1 2 4 8", "ninstr": "3 4 5 7", "nct": "1 2", "map": "plain xcd1 xcd2", "strip": "0 1"},
}


def chunks(Q, nqc):
    """(first tile, tiles, rotated start) of every q chunk: the kernel's rule, stated in dense_pass_plan.h"""
    total = Q // 8
    out = []
    for qc in range(nqc):
        beg, end = qc * total // nqc, (qc + 1) * total // nqc
        n = end - beg
        out.append((beg, n, (((qc * 2654435761) & 0xFFFFFFFF) >> 8) % n if n > 0 else 0))
    return out


def tags_of_plan(c, f):
    """the tag string of what the plan decided for case c: f maps the driver's field names to integers"""
    if c.kind == "left":
        return "ni3=%d ninstr=%d nct=%d map=%s strip=%d" % (f["ni3"], f["ninstr"], f["nct"], "xcd%d" % (c.n2 // 8) if f["xcd_map"] else "plain",
                                                          f["strip"])
    ch = chunks(c.Q, f["nqc"])
    lens = sorted({min(n, 3) for _, n, _ in ch})
    pc = "%d" % f["pcount0"] if not f["split"] else "%d+%s" % (f["pcount0"], f["pcount1"] if f["pcount1"] > 0 else "none")
    zr = "%d" % f["zcount0"] if not f["split"] else "%d+%s" % (f["zcount0"], f["zcount1"] if f["zcount1"] > 0 else "none")
    return "inst=%d.%d.%d.%d.%d kind=%s rows=%dx%d pc=%s zr=%s nt=%d nqc=%d cap=%d wide=%s lens=%s rot=%d" % (
        f["NBW"], f["TP"], f["SP"], f["ZT"], f["ZS"], "one" if f["one_kind"] else "split" if f["split"] else "plain", f["NB"], f["nbb"], pc, zr,
        f["nt"], f["nqc"], int(f["nqc"] < f["nqc_want"]), "-" if f["nbb"] == 1 else "%d" % (f["nbb"] * f["nt"] > 256), "+".join(map(str, lens)),
        int(any(n >= 3 and rot for _, n, rot in ch)))


def plan_call(c):
    """the driver's line for a case: kind, the extents, the low address bits of X | P | Z"""
    if c.kind == "left":
        return "L %d %d %d %d %d %d" % (c.n0, c.n1, c.n2, c.n3 * c.n4, c.n4, c.l)
    mis = 8 if any(c.opts.get(k) for k in ("xoff", "poff", "zoff")) else 0
    return "F %d %d %d %d %d %d" % (c.n0, c.Q, c.T, c.ll, c.r, mis)


# ------------------------------------------------------------------------------------------------ operands and truth
IN_NAMES = {"first": ("X", "C", "P"), "left": ("X", "A0", "A1t", "A2t", "A3p")}
OUT_NAMES = {"first": ("Z", "U"), "left": ("Z0", "Z1", "Z2", "E3")}


def out_shapes(c):
    if c.kind == "first":
        return {"Z": (c.ll, c.Q, c.T), "U": (c.n0, c.r, c.T)}
    C = c.n3 * c.n4
    return {"Z0": (c.l, c.n1 * c.n2 * C), "Z1": (c.l, c.n2 * C), "Z2": (c.l, C), "E3": (c.l, c.n3, c.n4)}


def products(c):
    """K of the bound: the number of products of one element of each output"""
    if c.kind == "first":
        return {"Z": c.n0, "U": c.Q}
    return {"Z0": c.n0, "Z1": c.n0 * c.n1, "Z2": c.n0 * c.n1 * c.n2, "E3": c.n0 * c.n1 * c.n2}


def offset(c, name):
    """elements between the first guard's end and the array: one for a pointer 8 bytes off"""
    return int(c.opts.get(name[0].lower() + "off", 0)) if c.kind == "first" else 0


def values(c, integer, seed, scale=1.0):
    """the numbers of one pass in their natural shapes: first pass X (n0, Q, T), C (n0, ll), P (Q, r); left pass
    X (n0, n1, n2, n3, n4) and A0 .. A3 (l, n0 .. n_mu)"""
    rng = np.random.default_rng(seed)
    draw = (lambda *s: rng.integers(-4, 5, size=s).astype(np.float64)) if integer else (lambda *s: rng.standard_normal(s))
    if c.kind == "first":
        return {"X": draw(c.n0, c.Q, c.T) * scale, "C": draw(c.n0, c.ll), "P": draw(c.Q, c.r)}
    ext = (c.n0, c.n1, c.n2, c.n3)
    v = {"X": draw(*ext, c.n4) * scale}
    for mu in range(4):
        v["A%d" % mu] = draw(c.l, *ext[:mu + 1])
    return v


def _einsums(c, v, dt):
    """every output from operands of type dt (np.int64, np.longdouble or np.float64), as matrix products"""
    if c.kind == "first":
        X = v["X"].astype(dt)
        Z = v["C"].astype(dt).T @ X.reshape(c.n0, c.Q * c.T)
        U = v["P"].astype(dt).T[None] @ X
        return {"Z": Z.reshape(c.ll, c.Q, c.T), "U": U}
    X = v["X"].astype(dt)
    out = {}
    for mu in range(3):
        A = v["A%d" % mu].astype(dt).reshape(c.l, -1)
        out["Z%d" % mu] = A @ X.reshape(A.shape[1], -1)
    A3 = v["A3"].astype(dt)
    out["E3"] = np.stack([A3[..., m].reshape(c.l, -1) @ X[:, :, :, m, :].reshape(-1, c.n4) for m in range(c.n3)], axis=1)
    return out


def truth(c, v, integer):
    """name -> (hi, lo, tol): integer pass -- the int64 result as float64 (exact), lo and tol None.  Gaussian pass -- the
    long-double result as a pair of doubles hi + lo (|got - ref| is then formed in float64 as |(got - hi) - lo|, the first
    difference exact for any got near hi) and the element-wise bound C_BOUND (K + 3) 2^-53 (|A| |B|)."""
    if integer:
        r = _einsums(c, v, np.int64)
        K = products(c)
        assert all(16 * K[n] < 2 ** 53 and int(np.abs(x).max(initial=0)) <= 16 * K[n] for n, x in r.items())
        return {n: (x.astype(np.float64), None, None) for n, x in r.items()}
    r = _einsums(c, v, LD)
    mag = _einsums(c, {k: np.abs(x) for k, x in v.items()}, np.float64)
    K = products(c)
    out = {}
    for n, x in r.items():
        hi = x.astype(np.float64)
        out[n] = (hi, (x - hi.astype(LD)).astype(np.float64), C_BOUND * (K[n] + 3) * 2.0 ** -53 * mag[n])
    return out


def _guarded(arr, off=0):
    return guarded(arr, PRE, POST, off)


def operands(c, v):
    """host images of the operand buffers, guards included, as the entry point reads them: the left pass gets A_1, A_2, A_3
    with i0 fastest -- A1t (l, n1, n0), A2t (l, n2, n1, n0), A3p (l, n2, n1, n3, n0)"""
    if c.kind == "first":
        return {n: _guarded(v[n], offset(c, n)) for n in IN_NAMES["first"]}
    return {"X": _guarded(v["X"]), "A0": _guarded(v["A0"]), "A1t": _guarded(np.ascontiguousarray(v["A1"].transpose(0, 2, 1))),
            "A2t": _guarded(np.ascontiguousarray(v["A2"].transpose(0, 3, 2, 1))),
            "A3p": _guarded(np.ascontiguousarray(v["A3"].transpose(0, 3, 2, 4, 1)))}


def sentinels(c):
    """host images of the output buffers before a call: every element the sentinel"""
    return {n: sentinel_buffer(offset(c, n) + int(np.prod(s)), PRE, POST) for n, s in out_shapes(c).items()}


def view(c, name, buf):
    s = out_shapes(c)[name]
    o = PRE + offset(c, name)
    return buf[o:o + int(np.prod(s))].reshape(s)


def float64_result(c, v):
    """what a correct kernel may return: the float64 products, in guarded buffers"""
    out = sentinels(c)
    for n, x in _einsums(c, v, np.float64).items():
        view(c, n, out[n])[...] = x
    return out


# ------------------------------------------------------------------------------------------------ the checks
def check_guards(c, out, what):
    for n, b in out.items():
        assert_guards(b, [(PRE + offset(c, n), (int(np.prod(out_shapes(c)[n])),), (1,))], "%s %s" % (what, n))


def check_untouched(out, what):
    """a refused call: nothing written at all"""
    assert_untouched(out, what)


def check_results(c, out, tr, integer, what=""):
    """the output buffers after one call (host images, guards included) against truth(): the guards first, then every
    element.  Returns the largest |err| / bound per output (0 in the integer pass, where nothing but equality passes)."""
    what = "%s %s (%s pass)" % (what, c.id, "integer" if integer else "Gaussian")
    check_guards(c, out, what)
    worst = {}
    for n in OUT_NAMES[c.kind]:
        got, (hi, lo, tol) = view(c, n, out[n]), tr[n]
        if integer:
            exact(got, hi, "%s %s" % (what, n))
            worst[n] = 0.0
        else:
            worst[n] = bounded(got, hi, lo, tol, "%s %s" % (what, n), FROB)
    return worst
