"""Reference, guarded operands and case table for the three fused chain-step kernels -- chain_step_kernel
(ttsk_chain_step), chain_wide_kernel (ttsk_chain_step_wide) and chain_sum_kernel (ttsk_chain_step_sum).  Plain module, no
GPU: tests/test_chain_edge_cover.py runs the table through the host plans and tests the checker on seeded defects,
tests/test_gpu_chain_edges.py runs every case on the device.

One step computes, per tensor b (tensor_train_drm.py:81-87),
    T_b[a, k, j] = sum_c W_b[c, a] X_b(j, k, c)            Out_b[j, a'] = sum_{a, k} T_b[a, k, j] E[a, k, a'].

A case is (entry, nb, n, K1, A, A2, J, opts); it runs in both layouts of X (right: X[j][k][c], left: X[c][k][j]) unless
opts names one, and with every way of storing T (fused / wide: none, per tensor; stacked terms: none, interleaved over the
terms, per term, per term with padded rows).

Buffers.  Every device buffer has PRE = POST = 64 guard elements around it.  Out_b, T_b and their guards start as the
sentinel -1/3 (finite, no multiple of 1/2: an unwritten element fails the integer pass, a stray store changes a guard); so
does every element of the stacked-terms T that no (b, a, k, j) addresses.  Operand elements outside their view -- the
columns A .. w_c - 1 of W, the gaps of a strided X, what lies behind the view inside x_extent, the guards -- are 1e300:
the kernels may read addressable padding against exact zeros (0 * 1e300 == 0), a read that meets a nonzero partner shows.

Options: w_pad (w_c = A + w_pad), x_gap (the slice stride and the outer stride of X grow by that many elements), x_slack
(x_extent reaches that far behind the view), x_off8 (the last tensor's X base 8 bytes off a 16-byte boundary), e_off8 (E 8
bytes off: the wide kernel only), layout, refuse (the plan must refuse the call).

Integer pass: W, X, E hold integers in [-2, 2]; every partial sum is below 4 K1 A n < 2^53, so the fp64 result is exact
in any order, slab reduce included: Out and T must EQUAL the int64 einsum (signed zeros are not told apart).
Gaussian pass: standard normal operands, truth in np.longdouble,
    |T - ref|   <= C (K1 + 2) 2^-53 (|W|^T |X|)_akj             |Out - ref| <= C (K1 + A n + 4) 2^-53 (|W|^T |X| . |E|)_jb
with C = 2 (C_BOUND, by the argument of tests/test_gpu_gemm_families.py): any order of the K1 and A n products, fused or not, cut into
chunks and reduced or not, is within that bound up to second-order terms.  (The two magnitude products are formed in
float64: they are sums of non-negative terms, right to a few 2^-53 of themselves, which moves the bound by less than
1e-13 of itself.)  Then the Frobenius ratio against 1e-12."""
from collections import namedtuple

import numpy as np

from tests.edge_kit import C_BOUND, LD, PAD, SENT, assert_guards, assert_untouched, bounded, exact, sentinel_buffer, strided  # noqa: F401

PRE = POST = 64
FROB = 1e-12
CW = (16, 24, 32, 40, 48, 56, 64)        # columns of the wide kernel's chunk structures (chain_plan.h CW_NQ, CW_SQ); the cover test compares
KINDS = {"fused": "ttsk_chain_step", "wide": "ttsk_chain_step_wide", "sum": "ttsk_chain_step_sum"}

Case = namedtuple("Case", "id kind nb n K1 A A2 J opts")


def case(id, kind, nb, n, K1, A, A2, J, **opts):
    return Case(id, kind, nb, n, K1, A, A2, J, opts)


# ------------------------------------------------------------------------------------------------ the table
def fused_cases():
    F = lambda id, nb=2, n=5, K1=8, A=16, A2=None, J=20, **o: case("f-" + id, "fused", nb, n, K1, A, A if A2 is None else A2, J, **o)
    c = [F("J%d" % J, J=J) for J in (1, 16, 17, 64, 65, 112)]
    c += [F("K%d" % K1, K1=K1) for K1 in (1, 3, 4, 5, 20, 21, 96, 100, 101, 128)]
    c += [F("A%d" % A, A=A, pack=1) for A in (16, 20, 24, 26, 32, 48, 52, 54, 56, 58, 64, 68, 80, 96, 100, 104, 112)]
    c += [F("A%d-%d" % aa, A=aa[0], A2=aa[1]) for aa in ((52, 50), (100, 98), (53, 54), (57, 58))]
    c += [F("lds", A=112, K1=60, J=112)]
    # the levelled 12-wave deal: two slices per workgroup, J > 64
    L = lambda id, **o: F("lv-" + id, **dict(dict(nb=32, n=16), **o))
    c += [L("A%d-J%d" % (A, J), A=A, J=J, pack=1) for A in (26, 48, 56, 64, 96, 100) for J in (65, 68, 69)]
    c += [L("n%d" % n, n=n, A=48, J=65) for n in (15, 17)]
    c += [L("A104-J%d" % J, A=104, J=J) for J in (65, 68, 69)] + [L("A24", A=24, J=65)]
    c += [L("K100", K1=100, J=112, A=100, pack=1)]
    # geometry
    c += [F("g1-n%d" % n, nb=1, n=n, J=65) for n in (1, 255, 256, 257, 512)]
    c += [F("g16-n%d" % n, nb=16, n=n) for n in (1, 2, 31, 32, 33)]
    c += [F("g32-n%d" % n, nb=32, n=n) for n in (8, 17)] + [F("g3-n171", nb=3, n=171)]
    for name, o in OPTIONS[:4]:
        c += [F(name, **o), L(name, A=48, J=65, **o)]
    return c


def wide_cases():
    Wd = lambda id, nb=1, n=4, K1=8, A=16, A2=16, J=20, **o: case("w-" + id, "wide", nb, n, K1, A, A2, J, **o)
    c = [Wd("A2-%d" % A2, A2=A2) for A2 in (1, 3, 4, 5, 8, 9, 16, 95, 144, 148, 152, 153, 160)]
    c += [Wd("J%d" % J, J=J) for J in (1, 16, 17, 48, 49, 112, 113, 176)]
    c += [Wd("J%d-A2-128" % J, J=J, A2=128) for J in (1, 48, 112)]
    c += [Wd("K%d" % K1, K1=K1, layout="left") for K1 in (129, 150, 200, 256)]
    c += [Wd("A%d" % A, K1=20, A2=110, A=A) for A in (1, 5, 20, 30, 45, 56, 57, 65, 112, 113, 168, 169, 225, 257)]
    c += [Wd("lds-A2-%d" % A2, A=64, K1=150, J=100, A2=A2) for A2 in (80, 82)]
    c += [Wd("nb%d-J%d" % (nb, J), nb=nb, n=6, K1=20, A=100, A2=100, J=J) for nb in (1, 2, 7, 8) for J in (16, 32, 33, 48, 49)]
    for name, o in OPTIONS:
        c += [Wd(name, **o), Wd("c2-" + name, K1=20, A2=110, A=65, **o)]
    return c


def sum_cases():
    S = lambda id, nb=8, n=6, K1=20, A=32, A2=32, J=20, **o: case("s-" + id, "sum", nb, n, K1, A, A2, J, **o)
    c = [S("J%d-K%d" % jk, J=jk[0], K1=jk[1]) for jk in ((1, 1), (4, 4), (5, 5), (16, 16), (17, 17), (20, 20), (19, 17))]
    c += [S("A%d" % A, A=A) for A in (4, 16, 17, 32, 33, 64, 65, 100, 128)]
    c += [S("A2-%d" % A2, A2=A2) for A2 in (4, 8, 10, 16, 20, 24, 26, 48, 52, 54, 58, 80, 100, 104, 112, 120, 128)]
    c += [S("nb%d" % nb, nb=nb, A=100, A2=100) for nb in (1, 2, 3, 4, 5, 9, 32)]
    c += [S("n%d" % n, n=n, A=100, A2=100) for n in (1, 2, 7, 9, 64, 128)]
    c += [S("tpw2", nb=12, A=112, A2=112), S("tpw1", A=128, A2=104)]
    c += [S(name, **o) for name, o in OPTIONS[:4]]
    return c


def refusals():
    """the far side of each cover limit: the plan must refuse, nothing may be written"""
    R = lambda id, kind, nb=2, n=5, K1=8, A=16, A2=16, J=20, **o: case("x-" + id, kind, nb, n, K1, A, A2, J, refuse=1, **o)
    return [R("f-J113", "fused", J=113), R("f-K129", "fused", K1=129), R("f-A2odd", "fused", A=18, A2=17),
            R("f-A52-48", "fused", A=52, A2=48), R("f-lds", "fused", A=112, A2=112, K1=61, J=112), R("f-eoff8", "fused", e_off8=1),
            R("f-nb33", "fused", nb=33, n=2), R("f-wc", "fused", w_pad=-1),
            R("w-A2-161", "wide", nb=1, A2=161), R("w-J177", "wide", nb=1, J=177), R("w-J113-A2-128", "wide", nb=1, J=113, A2=128),
            R("s-J21", "sum", nb=8, K1=20, J=21, A=32, A2=32), R("s-K21", "sum", nb=8, K1=21, J=20, A=32, A2=32),
            R("s-A129", "sum", nb=8, K1=20, J=20, A=129, A2=32), R("s-A2odd", "sum", nb=8, K1=20, J=20, A=32, A2=31),
            R("s-eoff8", "sum", nb=8, K1=20, J=20, A=32, A2=32, e_off8=1)]


OPTIONS = (("wpad", dict(w_pad=3)), ("xgap", dict(x_gap=3)), ("xslack", dict(x_slack=1000)), ("xoff8", dict(x_off8=1)),
           ("eoff8", dict(e_off8=1)))


def all_cases():
    return fused_cases() + wide_cases() + sum_cases()


# What each accepted case is meant to reach: the plan's fields at 256 compute units (tests/test_chain_edge_cover.py
# asserts every one of them against chain_fused_plan / chain_wide_plan / chain_sum_plan).  fused: `piece` counts the
# waves of a levelled workgroup by kind (W whole row tile, F / R first and rest of a cut one, 4 four rows, L loader).
TAGS = {
    "f-J1": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-J16": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-J17": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-J64": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-J65": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-J112": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-K1": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-K3": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-K4": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-K5": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-K20": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-K21": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-K96": "nf=1 str=0 ebuf=2 unr=25 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-K100": "nf=1 str=0 ebuf=2 unr=25 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-K101": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-K128": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A16": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A20": "nf=1 str=1 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A24": "nf=1 str=2 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A26": "nf=2 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A32": "nf=2 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A48": "nf=3 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A52": "nf=3 str=1 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A54": "nf=3 str=2 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A56": "nf=3 str=2 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A58": "nf=4 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A64": "nf=4 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A68": "nf=4 str=1 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A80": "nf=5 str=0 ebuf=1 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A96": "nf=6 str=0 ebuf=1 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A100": "nf=6 str=1 ebuf=1 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A104": "nf=6 str=2 ebuf=1 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A112": "nf=7 str=0 ebuf=1 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A52-50": "nf=3 str=1 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A100-98": "nf=6 str=1 ebuf=1 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A53-54": "nf=3 str=2 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-A57-58": "nf=4 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-lds": "nf=7 str=0 ebuf=1 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-lv-A26-J65": "nf=2 str=0 ebuf=2 unr=5 waves=12 wpp=8 xcd_map=1 piece=W4,41,L7",
    "f-lv-A26-J68": "nf=2 str=0 ebuf=2 unr=5 waves=12 wpp=8 xcd_map=1 piece=W4,41,L7",
    "f-lv-A26-J69": "nf=2 str=0 ebuf=2 unr=5 waves=12 wpp=8 xcd_map=1 piece=W4,F1,R1,L6",
    "f-lv-A48-J65": "nf=3 str=0 ebuf=2 unr=5 waves=12 wpp=8 xcd_map=1 piece=W4,41,L7",
    "f-lv-A48-J68": "nf=3 str=0 ebuf=2 unr=5 waves=12 wpp=8 xcd_map=1 piece=W4,41,L7",
    "f-lv-A48-J69": "nf=3 str=0 ebuf=2 unr=5 waves=12 wpp=8 xcd_map=1 piece=W3,F2,R2,L5",
    "f-lv-A56-J65": "nf=3 str=2 ebuf=2 unr=5 waves=12 wpp=8 xcd_map=1 piece=W4,41,L7",
    "f-lv-A56-J68": "nf=3 str=2 ebuf=2 unr=5 waves=12 wpp=8 xcd_map=1 piece=W4,41,L7",
    "f-lv-A56-J69": "nf=3 str=2 ebuf=2 unr=5 waves=12 wpp=8 xcd_map=1 piece=W3,F2,R2,L5",
    "f-lv-A64-J65": "nf=4 str=0 ebuf=2 unr=5 waves=12 wpp=8 xcd_map=1 piece=W4,41,L7",
    "f-lv-A64-J68": "nf=4 str=0 ebuf=2 unr=5 waves=12 wpp=8 xcd_map=1 piece=W4,41,L7",
    "f-lv-A64-J69": "nf=4 str=0 ebuf=2 unr=5 waves=12 wpp=8 xcd_map=1 piece=W3,F2,R2,L5",
    "f-lv-A96-J65": "nf=6 str=0 ebuf=1 unr=5 waves=12 wpp=8 xcd_map=1 piece=W4,41,L7",
    "f-lv-A96-J68": "nf=6 str=0 ebuf=1 unr=5 waves=12 wpp=8 xcd_map=1 piece=W4,41,L7",
    "f-lv-A96-J69": "nf=6 str=0 ebuf=1 unr=5 waves=12 wpp=8 xcd_map=1 piece=W3,F2,R2,L5",
    "f-lv-A100-J65": "nf=6 str=1 ebuf=1 unr=5 waves=12 wpp=8 xcd_map=1 piece=W4,41,L7",
    "f-lv-A100-J68": "nf=6 str=1 ebuf=1 unr=5 waves=12 wpp=8 xcd_map=1 piece=W4,41,L7",
    "f-lv-A100-J69": "nf=6 str=1 ebuf=1 unr=5 waves=12 wpp=8 xcd_map=1 piece=W3,F2,R2,L5",
    "f-lv-n15": "nf=3 str=0 ebuf=2 unr=5 waves=8 wpp=8 xcd_map=1 piece=-",
    "f-lv-n17": "nf=3 str=0 ebuf=2 unr=5 waves=12 wpp=8 xcd_map=1 piece=W4,41,L7",
    "f-lv-A104-J65": "nf=6 str=2 ebuf=1 unr=5 waves=8 wpp=8 xcd_map=1 piece=-",
    "f-lv-A104-J68": "nf=6 str=2 ebuf=1 unr=5 waves=8 wpp=8 xcd_map=1 piece=-",
    "f-lv-A104-J69": "nf=6 str=2 ebuf=1 unr=5 waves=8 wpp=8 xcd_map=1 piece=-",
    "f-lv-A24": "nf=1 str=2 ebuf=2 unr=5 waves=8 wpp=8 xcd_map=1 piece=-",
    "f-lv-K100": "nf=6 str=1 ebuf=1 unr=25 waves=8 wpp=8 xcd_map=1 piece=-",
    "f-g1-n1": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=1 xcd_map=0 piece=-",
    "f-g1-n255": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=255 xcd_map=0 piece=-",
    "f-g1-n256": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=256 xcd_map=1 piece=-",
    "f-g1-n257": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=256 xcd_map=1 piece=-",
    "f-g1-n512": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=256 xcd_map=1 piece=-",
    "f-g16-n1": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=1 xcd_map=0 piece=-",
    "f-g16-n2": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=2 xcd_map=0 piece=-",
    "f-g16-n31": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=16 xcd_map=1 piece=-",
    "f-g16-n32": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=16 xcd_map=1 piece=-",
    "f-g16-n33": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=16 xcd_map=1 piece=-",
    "f-g32-n8": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=8 xcd_map=1 piece=-",
    "f-g32-n17": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=8 xcd_map=1 piece=-",
    "f-g3-n171": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=85 xcd_map=0 piece=-",
    "f-wpad": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-lv-wpad": "nf=3 str=0 ebuf=2 unr=5 waves=12 wpp=8 xcd_map=1 piece=W4,41,L7",
    "f-xgap": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-lv-xgap": "nf=3 str=0 ebuf=2 unr=5 waves=12 wpp=8 xcd_map=1 piece=W4,41,L7",
    "f-xslack": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-lv-xslack": "nf=3 str=0 ebuf=2 unr=5 waves=12 wpp=8 xcd_map=1 piece=W4,41,L7",
    "f-xoff8": "nf=1 str=0 ebuf=2 unr=5 waves=8 wpp=5 xcd_map=0 piece=-",
    "f-lv-xoff8": "nf=3 str=0 ebuf=2 unr=5 waves=12 wpp=8 xcd_map=1 piece=W4,41,L7",
    "w-A2-1": "ci=0 nn=0 sn=1 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A2-3": "ci=0 nn=0 sn=1 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A2-4": "ci=0 nn=0 sn=1 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A2-5": "ci=0 nn=0 sn=2 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A2-8": "ci=0 nn=0 sn=2 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A2-9": "ci=0 nn=1 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A2-16": "ci=0 nn=1 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A2-95": "ci=0 nn=6 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A2-144": "ci=0 nn=9 sn=0 unr=5 mt2=0 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A2-148": "ci=0 nn=9 sn=1 unr=5 mt2=0 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A2-152": "ci=0 nn=9 sn=2 unr=5 mt2=0 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A2-153": "ci=0 nn=10 sn=0 unr=5 mt2=0 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A2-160": "ci=0 nn=10 sn=0 unr=5 mt2=0 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-J1": "ci=0 nn=1 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-J16": "ci=0 nn=1 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-J17": "ci=0 nn=1 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-J48": "ci=0 nn=1 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-J49": "ci=0 nn=1 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-J112": "ci=0 nn=1 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-J113": "ci=0 nn=1 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-J176": "ci=0 nn=1 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-J1-A2-128": "ci=0 nn=8 sn=0 unr=5 mt2=0 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-J48-A2-128": "ci=0 nn=8 sn=0 unr=5 mt2=0 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-J112-A2-128": "ci=0 nn=8 sn=0 unr=5 mt2=0 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-K129": "ci=0 nn=1 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-K150": "ci=0 nn=1 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-K200": "ci=0 nn=1 sn=0 unr=25 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-K256": "ci=0 nn=1 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A1": "ci=0 nn=7 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A5": "ci=0 nn=7 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A20": "ci=1 nn=7 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A30": "ci=2 nn=7 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A45": "ci=4 nn=7 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A56": "ci=5 nn=7 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A57": "ci=6 nn=7 sn=0 unr=5 mt2=0 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-A65": "ci=3 nn=7 sn=0 unr=5 mt2=1 nac=2 tpw=1 ebuf2=1 xcd_map=1",
    "w-A112": "ci=5 nn=7 sn=0 unr=5 mt2=1 nac=2 tpw=1 ebuf2=1 xcd_map=1",
    "w-A113": "ci=6 nn=7 sn=0 unr=5 mt2=0 nac=2 tpw=1 ebuf2=1 xcd_map=1",
    "w-A168": "ci=5 nn=7 sn=0 unr=5 mt2=1 nac=3 tpw=1 ebuf2=1 xcd_map=0",
    "w-A169": "ci=6 nn=7 sn=0 unr=5 mt2=0 nac=3 tpw=1 ebuf2=1 xcd_map=0",
    "w-A225": "ci=6 nn=7 sn=0 unr=5 mt2=0 nac=4 tpw=1 ebuf2=1 xcd_map=1",
    "w-A257": "ci=5 nn=7 sn=0 unr=5 mt2=1 nac=5 tpw=1 ebuf2=1 xcd_map=0",
    "w-lds-A2-80": "ci=6 nn=5 sn=0 unr=5 mt2=0 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-lds-A2-82": "ci=6 nn=5 sn=1 unr=5 mt2=0 nac=1 tpw=1 ebuf2=0 xcd_map=0",
    "w-nb1-J16": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=1 ebuf2=1 xcd_map=0",
    "w-nb1-J32": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=1 ebuf2=1 xcd_map=0",
    "w-nb1-J33": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=1 ebuf2=1 xcd_map=0",
    "w-nb1-J48": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=1 ebuf2=1 xcd_map=0",
    "w-nb1-J49": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=1 ebuf2=1 xcd_map=0",
    "w-nb2-J16": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=2 ebuf2=1 xcd_map=0",
    "w-nb2-J32": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=2 ebuf2=1 xcd_map=0",
    "w-nb2-J33": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=2 ebuf2=1 xcd_map=0",
    "w-nb2-J48": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=2 ebuf2=1 xcd_map=0",
    "w-nb2-J49": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=1 ebuf2=1 xcd_map=0",
    "w-nb7-J16": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=7 ebuf2=1 xcd_map=0",
    "w-nb7-J32": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=7 ebuf2=1 xcd_map=0",
    "w-nb7-J33": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=3 ebuf2=1 xcd_map=0",
    "w-nb7-J48": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=3 ebuf2=1 xcd_map=0",
    "w-nb7-J49": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=1 ebuf2=1 xcd_map=0",
    "w-nb8-J16": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=7 ebuf2=1 xcd_map=0",
    "w-nb8-J32": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=7 ebuf2=1 xcd_map=0",
    "w-nb8-J33": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=3 ebuf2=1 xcd_map=0",
    "w-nb8-J48": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=3 ebuf2=1 xcd_map=0",
    "w-nb8-J49": "ci=5 nn=6 sn=1 unr=5 mt2=1 nac=2 tpw=1 ebuf2=1 xcd_map=0",
    "w-wpad": "ci=0 nn=1 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-c2-wpad": "ci=3 nn=7 sn=0 unr=5 mt2=1 nac=2 tpw=1 ebuf2=1 xcd_map=1",
    "w-xgap": "ci=0 nn=1 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-c2-xgap": "ci=3 nn=7 sn=0 unr=5 mt2=1 nac=2 tpw=1 ebuf2=1 xcd_map=1",
    "w-xslack": "ci=0 nn=1 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-c2-xslack": "ci=3 nn=7 sn=0 unr=5 mt2=1 nac=2 tpw=1 ebuf2=1 xcd_map=1",
    "w-xoff8": "ci=0 nn=1 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-c2-xoff8": "ci=3 nn=7 sn=0 unr=5 mt2=1 nac=2 tpw=1 ebuf2=1 xcd_map=1",
    "w-eoff8": "ci=0 nn=1 sn=0 unr=5 mt2=1 nac=1 tpw=1 ebuf2=1 xcd_map=0",
    "w-c2-eoff8": "ci=3 nn=7 sn=0 unr=5 mt2=1 nac=2 tpw=1 ebuf2=1 xcd_map=1",
    "s-J1-K1": "na_run=1 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-J4-K4": "na_run=1 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-J5-K5": "na_run=1 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-J16-K16": "na_run=1 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-J17-K17": "na_run=1 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-J20-K20": "na_run=1 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-J19-K17": "na_run=1 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-A4": "na_run=1 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-A16": "na_run=1 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-A17": "na_run=1 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-A32": "na_run=1 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-A33": "na_run=2 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-A64": "na_run=2 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-A65": "na_run=3 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-A100": "na_run=4 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-A128": "na_run=4 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-A2-4": "na_run=1 tpw=4 NNF=0 NS=1 nranges=1 xcd_map=0",
    "s-A2-8": "na_run=1 tpw=4 NNF=0 NS=2 nranges=1 xcd_map=0",
    "s-A2-10": "na_run=1 tpw=4 NNF=1 NS=0 nranges=1 xcd_map=0",
    "s-A2-16": "na_run=1 tpw=4 NNF=1 NS=0 nranges=1 xcd_map=0",
    "s-A2-20": "na_run=1 tpw=4 NNF=1 NS=1 nranges=1 xcd_map=0",
    "s-A2-24": "na_run=1 tpw=4 NNF=1 NS=2 nranges=1 xcd_map=0",
    "s-A2-26": "na_run=1 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-A2-48": "na_run=1 tpw=4 NNF=3 NS=0 nranges=1 xcd_map=0",
    "s-A2-52": "na_run=1 tpw=4 NNF=3 NS=1 nranges=1 xcd_map=0",
    "s-A2-54": "na_run=1 tpw=4 NNF=3 NS=2 nranges=1 xcd_map=0",
    "s-A2-58": "na_run=1 tpw=4 NNF=4 NS=0 nranges=1 xcd_map=0",
    "s-A2-80": "na_run=1 tpw=4 NNF=5 NS=0 nranges=1 xcd_map=0",
    "s-A2-100": "na_run=1 tpw=4 NNF=6 NS=1 nranges=1 xcd_map=0",
    "s-A2-104": "na_run=1 tpw=4 NNF=6 NS=2 nranges=1 xcd_map=0",
    "s-A2-112": "na_run=1 tpw=4 NNF=7 NS=0 nranges=1 xcd_map=0",
    "s-A2-120": "na_run=1 tpw=4 NNF=7 NS=2 nranges=1 xcd_map=0",
    "s-A2-128": "na_run=1 tpw=4 NNF=8 NS=0 nranges=1 xcd_map=0",
    "s-nb1": "na_run=4 tpw=4 NNF=6 NS=1 nranges=2 xcd_map=0",
    "s-nb2": "na_run=4 tpw=4 NNF=6 NS=1 nranges=2 xcd_map=0",
    "s-nb3": "na_run=4 tpw=4 NNF=6 NS=1 nranges=2 xcd_map=0",
    "s-nb4": "na_run=4 tpw=4 NNF=6 NS=1 nranges=2 xcd_map=0",
    "s-nb5": "na_run=4 tpw=4 NNF=6 NS=1 nranges=2 xcd_map=0",
    "s-nb9": "na_run=4 tpw=4 NNF=6 NS=1 nranges=2 xcd_map=0",
    "s-nb32": "na_run=4 tpw=4 NNF=6 NS=1 nranges=2 xcd_map=0",
    "s-n1": "na_run=4 tpw=4 NNF=6 NS=1 nranges=1 xcd_map=0",
    "s-n2": "na_run=4 tpw=4 NNF=6 NS=1 nranges=1 xcd_map=0",
    "s-n7": "na_run=4 tpw=4 NNF=6 NS=1 nranges=2 xcd_map=0",
    "s-n9": "na_run=4 tpw=4 NNF=6 NS=1 nranges=3 xcd_map=0",
    "s-n64": "na_run=4 tpw=4 NNF=6 NS=1 nranges=16 xcd_map=1",
    "s-n128": "na_run=4 tpw=4 NNF=6 NS=1 nranges=40 xcd_map=1",
    "s-tpw2": "na_run=2 tpw=2 NNF=7 NS=0 nranges=2 xcd_map=0",
    "s-tpw1": "na_run=1 tpw=1 NNF=6 NS=2 nranges=1 xcd_map=0",
    "s-wpad": "na_run=1 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-xgap": "na_run=1 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-xslack": "na_run=1 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
    "s-xoff8": "na_run=1 tpw=4 NNF=2 NS=0 nranges=1 xcd_map=0",
}

# every branch of the three plans some case must reach (test_table_covers_every_branch)
BRANCHES = {
    "fused": {"nf": "1 2 3 4 5 6 7", "str": "0 1 2", "ebuf": "1 2", "unr": "5 25", "waves": "8 12", "wpp": "1 2 5 8 16 85 255 256", "xcd_map": "0 1",
              "piece": "- W4,41,L7 W4,F1,R1,L6 W3,F2,R2,L5"},
    "wide": {"ci": "0 1 2 3 4 5 6", "nn": "0 1 5 6 7 8 9 10", "sn": "0 1 2", "unr": "5 25", "mt2": "0 1", "nac": "1 2 3 4 5", "tpw": "1 2 3 7",
             "ebuf2": "0 1", "xcd_map": "0 1"},
    "sum": {"na_run": "1 2 3 4", "tpw": "1 2 4", "NNF": "0 1 2 3 4 5 6 7 8", "NS": "0 1 2", "nranges": "1 2 3 16 40", "xcd_map": "0 1"},
}
TAG_KEYS = {k: tuple(v) for k, v in BRANCHES.items()}


def tags_of_plan(kind, f):
    """the tagged fields of one accepted plan (a record of test_chain_plan.parse) as the string TAGS holds"""
    g = {}
    for k in TAG_KEYS[kind]:
        if k == "piece":
            p = [int(x) >> 16 for x in f["a.piece"].split(",")]
            g[k] = "-" if int(f["waves"]) == 8 else ",".join("%s%d" % (s, p.count(i)) for i, s in ((1, "W"), (2, "F"), (3, "R"), (4, "4"), (0, "L")) if p.count(i))
        else:
            g[k] = f[k] if k in f else f["a." + k]
    return " ".join("%s=%s" % kv for kv in g.items())


# ------------------------------------------------------------------------------------------------ calls
T_MODES = {"fused": (0, 1), "wide": (0, 1), "sum": (0, 1, 2, 3)}     # sum: 1 interleaved, 2 per term, 3 per term, rows of J + 2


def layouts(c):
    return (c.opts["layout"],) if "layout" in c.opts else ("right", "left")


def geometry(c, layout, wt=0):
    """strides, extents and offsets (elements) of one call"""
    o = c.opts
    gap = o.get("x_gap", 0)
    if layout == "right":
        x_c, x_k = 1, c.K1 + gap
        x_j = c.n * x_k + gap
    else:
        x_j, x_k = 1, c.J + gap
        x_c = c.n * x_k + gap
    span = (c.J - 1) * x_j + (c.n - 1) * x_k + (c.K1 - 1) * x_c + 1
    g = dict(w_c=c.A + o.get("w_pad", 0), x_j=x_j, x_k=x_k, x_c=x_c, x_span=span, x_extent=span + o.get("x_slack", 0),
             x_off=1 if o.get("x_off8") else 0, e_off=1 if o.get("e_off8") else 0, t_b=0, t_ld=0, t_extent=0)
    if c.kind == "sum" and wt:
        ld = {1: c.nb * c.J, 2: c.J, 3: c.J + 2}[wt]
        g.update(t_ld=ld, t_b=c.J if wt == 1 else c.A * c.n * ld, t_extent=c.A * c.n * ld * (1 if wt == 1 else c.nb))
    return g


def plan_call(c, layout, wt=2):
    """the call in the terms of test_chain_plan.CALL_KEYS (byte offsets of E and of the last X)"""
    g = geometry(c, layout, wt)
    return [c.nb, c.n, c.K1, c.A, c.A2, c.J, g["w_c"], g["x_j"], g["x_k"], g["x_c"], g["x_extent"], 8 * g["e_off"], 8 * g["x_off"],
            g["t_b"], g["t_ld"], g["t_extent"]]


def macs(c):
    return c.nb * c.n * c.J * (c.K1 * c.A + c.A * c.A2)


# ------------------------------------------------------------------------------------------------ operands and truth
def values(c, integer, seed):
    """W_b (K1, A), X_b as (J, n, K1), E (A, n, A2): the numbers of one pass, whatever the layout"""
    rng = np.random.default_rng(seed)
    draw = (lambda *s: rng.integers(-2, 3, size=s).astype(np.float64)) if integer else (lambda *s: rng.standard_normal(s))
    return [draw(c.K1, c.A) for _ in range(c.nb)], [draw(c.J, c.n, c.K1) for _ in range(c.nb)], draw(c.A, c.n, c.A2)


def _one_truth(c, w, x, E, integer):
    dt = np.int64 if integer else LD
    xt = x.transpose(2, 1, 0).reshape(c.K1, c.n * c.J)                  # [c][(k, j)]
    t = w.astype(dt).T @ xt.astype(dt)                                   # [a][(k, j)]
    o = t.reshape(c.A * c.n, c.J).T @ E.astype(dt).reshape(c.A * c.n, c.A2)
    t = t.reshape(c.A, c.n, c.J)
    if integer:
        return t.astype(np.float64), None, None, o.astype(np.float64), None, None, int(np.abs(o).max(initial=0))
    eps = 2.0 ** -53
    m = np.abs(w).T @ np.abs(xt)
    mo = m.reshape(c.A * c.n, c.J).T @ np.abs(E).reshape(c.A * c.n, c.A2)
    split = lambda r: (r.astype(np.float64), (r - r.astype(np.float64).astype(LD)).astype(np.float64))
    return split(t) + (C_BOUND * (c.K1 + 2) * eps * m.reshape(c.A, c.n, c.J),) + split(o) + (C_BOUND * (c.K1 + c.A * c.n + 4) * eps * mo,)


def truth(c, vals, integer):
    """Per tensor (T, Out): integer pass -- the int64 einsum as float64 (exact: below 2^50).  Gaussian pass -- the long-double
    result as a pair of doubles hi + lo (hi the nearest double, lo the rest: |got - ref| is then formed in float64 as
    |(got - hi) - lo|, the first difference exact for any got near hi) and the element-wise bound.  The tensors are
    independent: a few threads share them (long-double products run outside the interpreter lock)."""
    from concurrent.futures import ThreadPoolExecutor
    W, X, E = vals
    with ThreadPoolExecutor(max_workers=min(8, c.nb)) as ex:
        r = list(ex.map(lambda wx: _one_truth(c, wx[0], wx[1], E, integer), zip(W, X)))
    if integer:
        assert max(x[6] for x in r) < 2 ** 50 and 4 * c.K1 * c.A * c.n < 2 ** 53
    return dict(T=[x[0] for x in r], T_lo=[x[1] for x in r], T_tol=[x[2] for x in r], Out=[x[3] for x in r], Out_lo=[x[4] for x in r],
                Out_tol=[x[5] for x in r])


def operands(c, layout, vals):
    """host images of the device buffers, guards included: ([W_b], [X_b], E) and the element offset of every base"""
    g = geometry(c, layout)
    W, X, E = vals
    hW, hX, offX = [], [], []
    for b in range(c.nb):
        w = np.full(PRE + c.K1 * g["w_c"] + POST, PAD)
        strided(w, PRE, (c.K1, c.A), (g["w_c"], 1))[...] = W[b]
        hW.append(w)
        off = PRE + (g["x_off"] if b == c.nb - 1 else 0)
        x = np.full(off + g["x_extent"] + POST, PAD)
        strided(x, off, (c.J, c.n, c.K1), (g["x_j"], g["x_k"], g["x_c"]))[...] = X[b]
        hX.append(x)
        offX.append(off)
    e = np.full(PRE + g["e_off"] + E.size + POST, PAD)
    e[PRE + g["e_off"]:PRE + g["e_off"] + E.size] = E.reshape(-1)
    return hW, hX, e, dict(W=[PRE] * c.nb, X=offX, E=PRE + g["e_off"])


def sentinels(c, layout, wt):
    """host images of Out_b and T: every element the sentinel.  T: None, nb buffers (fused, wide) or one (stacked terms)"""
    g = geometry(c, layout, wt)
    new = lambda m: sentinel_buffer(m, PRE, POST)
    out = [new(c.J * c.A2) for _ in range(c.nb)]
    if not wt:
        return out, None
    return out, [new(g["t_extent"])] if c.kind == "sum" else [new(c.A * c.n * c.J) for _ in range(c.nb)]


def t_views(c, layout, wt, bufs):
    """T_b (A, n, J) of every tensor as a view of the buffers"""
    if c.kind != "sum":
        return [strided(t, PRE, (c.A, c.n, c.J), (c.n * c.J, c.J, 1)) for t in bufs]
    g = geometry(c, layout, wt)
    return [strided(bufs[0], PRE + b * g["t_b"], (c.A, c.n, c.J), (c.n * g["t_ld"], g["t_ld"], 1)) for b in range(c.nb)]


# ------------------------------------------------------------------------------------------------ the checks
def check_guards(c, layout, wt, out, tb, what):
    """every element of the Out and T buffers outside the results still holds the sentinel"""
    g = geometry(c, layout, wt)
    for b, o in enumerate(out):
        assert_guards(o, [(PRE, (c.J * c.A2,), (1,))], "%s Out[%d]" % (what, b))
    if tb is None:
        return
    if c.kind == "sum":
        views = [[(PRE + b * g["t_b"], (c.A, c.n, c.J), (c.n * g["t_ld"], g["t_ld"], 1)) for b in range(c.nb)]]
    else:
        views = [[(PRE, (c.A * c.n * c.J,), (1,))] for _ in tb]
    for b, (t, v) in enumerate(zip(tb, views)):
        assert_guards(t, v, "%s T[%d]" % (what, b))


def check_untouched(c, out, tb, what):
    """a refused call: nothing written at all"""
    assert_untouched(out, what + " Out")
    assert_untouched(tb or [], what + " T")


def check_results(c, layout, wt, out, tb, tr, integer, what=""):
    """Out and T of one call (host images of the buffers after it) against the truth `tr` of truth(); guards included.
    Returns the largest |err| / bound of Out and of T (Gaussian pass; 0 in the integer pass, where nothing but equality passes)."""
    worst = {"Out": 0.0, "T": 0.0}
    what = "%s %s %s T%d (%s pass)" % (what, c.id, layout, wt, "integer" if integer else "Gaussian")
    check_guards(c, layout, wt, out, tb, what)
    tv = t_views(c, layout, wt, tb) if tb is not None else None
    for b in range(c.nb):
        for name, got in (("Out", out[b][PRE:PRE + c.J * c.A2].reshape(c.J, c.A2)), ("T", None if tv is None else tv[b])):
            if got is None:
                continue
            if integer:
                exact(got, tr[name][b], "%s %s[%d]" % (what, name, b))
            else:
                worst[name] = max(worst[name], bounded(got, tr[name][b], tr[name + "_lo"][b], tr[name + "_tol"][b], "%s %s[%d]" % (what, name, b), FROB))
    return worst


def float64_result(c, layout, wt, vals):
    """what a correct kernel may return: the two float64 einsums of the existing chain tests, in guarded buffers"""
    W, X, E = vals
    out, tb = sentinels(c, layout, wt)
    tv = t_views(c, layout, wt, tb) if tb is not None else None
    for b in range(c.nb):
        t = np.einsum("ca,jkc->akj", W[b], X[b])
        out[b][PRE:PRE + c.J * c.A2] = np.einsum("akj,akb->jb", t, E).reshape(-1)
        if tv is not None:
            tv[b][...] = t
    return out, tb
