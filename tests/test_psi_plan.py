"""The host-side plans of the two Psi product kernels (csrc/psi_plan.h, plain C++): a short driver compiled with the host
compiler prints every non-pointer field of what psi_stream_plan / psi_stream_sum_plan decide and what stream_small_chunks
returns, and that is checked here -- before any kernel reads it.

(a) tests/golden/psi_plan_cases.json holds, for a list of calls, what the launchers of the commit before psi_plan.h decided
    (recorded from that commit's own stream_small.hip, compiled for the host and linked against stubs that print what they
    are handed -- the method tests/test_chain_plan.py describes): the verdict, and for an accepted call the kernel-argument
    struct, the instantiation, LDS, grid, the profiling bracket's name and work.  The plans must give the same, field by
    field -- but for the empty column chunks of the sum kernel, which the plan drops (without_empty_chunks), and a guard on the
    32-bit byte offsets of W that stream_small_kernel's launcher lacked (test_the_w_guard_is_the_plans_own).
(b) On every accepted plan of the edge list below -- the smallest shapes on either side of each branch, the three 32-bit
    guards included, which no GPU test can reach without buffers of gigabytes -- the invariants the kernels rely on.
(c) Every case of tests/psi_stream_ref.py (what tests/test_gpu_psi_edges.py runs on the device) reaches the plan branch it
    is tagged with, the refusals are refused, and the tags cover both launch tables completely."""
import json
import os

import numpy as np
import pytest

from tests import psi_stream_ref as ref
from tests.host_driver import ROOT, compile_driver, run_driver

FIXTURE = os.path.join(ROOT, "tests", "golden", "psi_plan_cases.json")

LIM32 = (1 << 32) - 64
LDS_MAX = 160 * 1024
N_CU = (256, 20)        # 20: fewer compute units than problems of a launch -- the wpp clamp, the chunk growth of the sum kernel
CALL_KEYS = ("nb", "J", "K1", "A", "s_j", "w_c", "c_j", "s_b", "w_b", "acc", "off")

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "psi_plan.h"
using namespace ttsk;

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    const int n_cu = atoi(argv[1]);
    FILE *f = fopen(argv[2], "r");
    if (!f) return 2;
    printf("const PSI_LDS_MAX=%zu PSI_SUM_IMAGE_MAX=%d PSI_LIM32=%lld SK_MAXB=%d ERR_HIP=%d\n", PSI_LDS_MAX, PSI_SUM_IMAGE_MAX, (long long)PSI_LIM32,
           SK_MAXB, (int)TTSK_ERR_HIP);
#define ST(NF, STR) printf(" %d,%d", NF, STR);
    printf("ss_table"); PSI_STREAM_STRUCTURES(ST)
    printf("\nsss_table"); PSI_STREAM_SUM_STRUCTURES(ST)
    printf("\n");
    char id[128], kind[16];
    long long v[11];
    while (fscanf(f, "%127s %15s", id, kind) == 2) {
        for (int i = 0; i < 11; ++i)
            if (fscanf(f, "%lld", &v[i]) != 1) return 3;
        if (!strcmp(kind, "ch")) { printf("%s ncu=%d ch rc=%d\n", id, n_cu, stream_small_chunks(v[0], v[1], (int)v[2])); continue; }
        const int nb = (int)v[0], ntab = nb < 1 ? 1 : (nb > SK_MAXB ? SK_MAXB + 1 : nb);
        const double *S[SK_MAXB + 1], *W[SK_MAXB + 1];
        double *C[SK_MAXB + 1];
        for (int b = 0; b < ntab; ++b) {           // never dereferenced: integers cast to pointers
            S[b] = (const double *)(0x20000000ull + 0x100000ull * b + (b == ntab - 1 ? v[10] : 0));
            W[b] = (const double *)(0x30000000ull + 0x100000ull * b);
            C[b] = (double *)(0x50000000ull + 0x100000ull * b);
        }
        if (!strcmp(kind, "ss")) {
            StreamSmallArgs c{nb, (int)v[1], (int)v[2], (int)v[3], S, v[4], W, v[5], C, v[6], (int)v[9]};
            PsiStreamPlan p;
            const int rc = psi_stream_plan(c, n_cu, p);
            printf("%s ncu=%d ss rc=%d", id, n_cu, rc);
            if (rc == 1) {
                const StreamSmall &a = p.a;
                int ok = 1;
                for (int b = 0; b < SK_MAXB; ++b) {
                    const bool in = b < nb;
                    ok &= a.S[b] == (in ? S[b] : nullptr) && a.W[b] == (in ? W[b] : nullptr) && a.C[b] == (in ? C[b] : nullptr);
                }
                printf(" nf=%d str=%d unr=%d lds=%zu grid=%d flops=%.17g a.nb=%d a.wpp=%d a.nac=%d a.ac=%d a.J=%d a.K1=%d a.A=%d a.s_j=%lld a.w_c=%lld"
                       " a.c_j=%lld a.s_extent=%lld a.c_extent=%lld a.AP=%d a.accumulate=%d tables=%d KB1=%d name=%s", p.nf, p.str, p.unr, p.l.lds,
                       p.l.grid, p.l.flops, a.nb, a.wpp, a.nac, a.ac, a.J, a.K1, a.A, (long long)a.s_j, (long long)a.w_c, (long long)a.c_j,
                       (long long)a.s_extent, (long long)a.c_extent, a.AP, a.accumulate, ok, p.KB1, p.l.name);
            }
            printf("\n");
        } else {
            StreamSmallSumArgs c{nb, (int)v[1], (int)v[2], (int)v[3], S[ntab - 1], v[4], v[7], W[0], v[5], v[8], C[0], v[6], (int)v[9]};
            PsiStreamSumPlan p;
            const int rc = psi_stream_sum_plan(c, n_cu, p);
            printf("%s ncu=%d sss rc=%d", id, n_cu, rc);
            if (rc == 1) {
                const StreamSmallSum &a = p.a;
                printf(" nf=%d str=%d unr=%d lds=%zu grid=%d flops=%.17g a.nb=%d a.groups=%d a.nac=%d a.ac=%d a.J=%d a.K1=%d a.A=%d a.s_j=%lld"
                       " a.w_c=%lld a.c_j=%lld a.s_b=%lld a.w_b=%lld a.s_extent=%lld a.w_extent=%lld a.c_extent=%lld a.AP=%d a.xcd_map=%d"
                       " a.accumulate=%d tables=%d KB1=%d name=%s", p.nf, p.str, p.unr, p.l.lds, p.l.grid, p.l.flops, a.nb, a.groups, a.nac, a.ac,
                       a.J, a.K1, a.A, (long long)a.s_j, (long long)a.w_c, (long long)a.c_j, (long long)a.s_b, (long long)a.w_b,
                       (long long)a.s_extent, (long long)a.w_extent, (long long)a.c_extent, a.AP, a.xcd_map, a.accumulate,
                       (int)(a.S == c.S && a.W == c.W && a.C == c.C), p.KB1, p.l.name);
            }
            printf("\n");
        }
    }
    fclose(f);
    return 0;
}
"""


def call(kind, nb=None, J=1024, K1=8, A=32, **over):
    """A call as the GPU test makes it: tight rows, the terms of a sum behind one another; `over` replaces single numbers."""
    c = dict(nb=(1 if kind == "ss" else 2) if nb is None else nb, J=J, K1=K1, A=A, s_j=K1, w_c=A, c_j=A, s_b=J * K1, w_b=K1 * A, acc=0, off=0)
    if kind == "ss":
        c.update(s_b=0, w_b=0)
    c.update(over)
    return [kind] + [c[k] for k in CALL_KEYS]


def chunks(K, A, mx):
    return ["ch", K, A, mx] + [0] * 8


def edge_list():
    """(id, call): the smallest shapes on either side of each branch of the two plans and of stream_small_chunks"""
    e = []
    P = lambda id, **o: ("ep-" + id, call("ss", **o))
    S = lambda id, **o: ("es-" + id, call("sss", **o))
    # ---- stream_small_kernel
    e += [P("nb%d" % nb, nb=nb) for nb in (0, 1, 2, 20, 21, 32, 33)]
    e += [P("J%d" % J, J=J) for J in (1023, 1024, 1025, 1039, 1041, 2048, 1 << 20)]
    e += [P("K%d" % K1, K1=K1) for K1 in (0, 1, 3, 4, 5, 20, 21, 80, 81, 100, 101, 180, 181, 600)]
    e += [P("A%d" % A, A=A) for A in (3, 4, 8, 9, 12, 16, 17, 20, 21, 24, 25, 32, 104, 105, 112, 113, 130, 224, 225, 1792, 1793)]
    e += [P("K%d-A%d" % (K1, A), K1=K1, A=A) for K1, A in ((600, 32), (600, 33), (600, 64), (600, 512), (600, 513), (160, 112), (161, 112), (1260, 16), (1261, 16))]
    e += [P("sj-1", s_j=7), P("wc-1", w_c=31), P("cj-1", c_j=31), P("pads", s_j=11, w_c=37, c_j=39), P("acc", acc=1), P("off4", off=4), P("off8", off=8)]
    e += [P("nb32-J%d" % J, nb=32, J=J) for J in (1024, 1107, 1152)] + [P("nb%d-A130" % nb, nb=nb, A=130) for nb in (5, 8, 16)]
    # the 32-bit guards: S with the look-ahead of wpp * 8 tiles, C
    J = 1 << 20
    nt, wpp = J // 16, 256
    sj = (LIM32 // 8 - 256 - 1) // ((nt + wpp * 8 + 2) * 16)
    e += [P("sj-under", J=J, s_j=sj), P("sj-over", J=J, s_j=sj + 1)]
    cj = (LIM32 // 8 - 256 - 1) // ((nt + 1) * 16)
    e += [P("cj-under", J=J, c_j=cj), P("cj-over", J=J, c_j=cj + 1)]
    wc = (LIM32 // 8 - 256 - 1) // 8
    e += [P("wc-under", w_c=wc), P("wc-over", w_c=wc + 1)]
    # ---- stream_small_sum_kernel
    e += [S("nb%d" % nb, nb=nb) for nb in (1, 2, 3, 8, 33, 100)]
    e += [S("J%d" % J, J=J) for J in (1023, 1024, 1025, 1039, 1041, 2048, 2049, 2176, 2177, 4096, 12288, 12289)]
    e += [S("K%d" % K1, K1=K1) for K1 in (0, 1, 3, 4, 5, 20, 21, 80, 81, 100, 101, 380, 381)]
    e += [S("A%d" % A, A=A) for A in (7, 8, 16, 17, 32, 33, 40, 45, 47, 48, 64, 112, 113, 128, 896, 897)]
    e += [S("J2049-A%d" % A, J=2049, A=A) for A in (256, 257, 320, 384, 512, 576, 640, 768, 832, 896, 897)]
    e += [S("J1025-A%d" % A, J=1025, A=A) for A in (32, 128)]
    e += [S("sj-1", s_j=7), S("wc-1", w_c=31), S("cj-1", c_j=31), S("sb-1", s_b=-1), S("wb-1", w_b=-1), S("sb0", s_b=0, w_b=0),
          S("pads", s_j=11, w_c=37, c_j=39, s_b=1024 * 11 + 5, w_b=8 * 37 + 3), S("acc", acc=1), S("off4", off=4)]
    sb = (LIM32 // 8 - 256 - 4 * 5 - 65 * 16 * 8 - 1) // 2
    e += [S("sb-under", s_b=sb), S("sb-over", s_b=sb + 1)]
    wb = (LIM32 // 8 - 256 - 8 * 32 - 1) // 2
    e += [S("wb-under", w_b=wb), S("wb-over", w_b=wb + 1)]
    e += [S("cj-under", J=J, c_j=cj), S("cj-over", J=J, c_j=cj + 1)]
    # ---- stream_small_chunks: K % t, (K / t) % 4, the LDS image of a chunk
    e += [("ec-%d-%d-%d" % kam, chunks(*kam)) for kam in ((640, 100, 32), (640, 100, 3), (640, 100, 4), (168, 100, 32), (172, 100, 32), (168, 101, 32),
                                                       (168, 104, 32), (168, 105, 32), (642, 20, 32), (644, 20, 32), (6, 20, 32), (8, 20, 32),
                                                       (6400, 100, 32), (6400, 100, 64), (3200, 100, 32), (0, 100, 32), (640, 100, 0))]
    return e


def parse(text):
    """driver / recorder output -> {(id, ncu, kind): fields}, header lines apart"""
    out, head = {}, {}
    for line in text.splitlines():
        line, _, name = line.partition(" name=")
        w = line.split()
        if w[0] in ("const", "ss_table", "sss_table"):
            head[w[0]] = w[1:]
            continue
        f = dict(x.split("=", 1) for x in w[3:])
        if name:
            f["name"] = name
        out[(w[0], int(w[1][4:]), w[2])] = f
    return out, head


def run_plans(tmp_path_factory, cases, n_cus):
    """cases {id: call} through the plans at each compute-unit count"""
    exe = compile_driver(tmp_path_factory, "psi_plan", DRIVER)
    txt = exe.parent / "cases.txt"
    txt.write_text("".join("%s %s\n" % (k, " ".join(str(x) for x in v)) for k, v in cases.items()))
    res, head = {}, None
    for n_cu in n_cus:
        r, head = parse(run_driver(exe, [n_cu, txt]))
        res.update(r)
    return res, head


@pytest.fixture(scope="module")
def fixture_file():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def plans(tmp_path_factory, fixture_file):
    """every case of the fixture, of the edge list and of the GPU test's table through the plans"""
    todo = {c[0]: c[1] for c in fixture_file["cases"]}
    for name, c in edge_list() + ref.plan_calls():
        assert todo.setdefault(name, c) == c, name
    res, head = run_plans(tmp_path_factory, todo, N_CU + (0,))
    return res, head, todo


def test_the_w_guard_is_the_plans_own(plans, fixture_file):
    """psi_stream_plan refuses a W whose byte offsets pass 32 bits; the launcher it replaces accepted the call (its kernel would
    have read wrapped offsets).  The fixture records the old verdict; this is the one case where the plan's differs."""
    res, _, _ = plans
    rec = {c[0]: c[2] for c in fixture_file["cases"]}
    assert rec["ep-wc-over"][0][0] == 1 and int(res[("ep-wc-over", 256, "ss")]["rc"]) == 0
    assert rec["ep-wc-under"][0][0] == 1 and int(res[("ep-wc-under", 256, "ss")]["rc"]) == 1


W_GUARD_ONLY = ("ep-wc-over",)


def without_empty_chunks(kind, want):
    """The one decision psi_stream_sum_plan takes differently from the launcher it replaces: column chunks that begin behind
    A (the old launcher grew the chunk count past ceil(A / ac); those workgroups stored nothing) are not launched.  The
    recorded plan with them dropped: nac, the grid and the XCD map that follows from it; every other field as recorded."""
    if kind != "sss":
        return want
    A, ac, nac, groups = (int(want[k]) for k in ("a.A", "a.ac", "a.nac", "a.groups"))
    keep = -(-A // ac)
    assert 2 <= keep <= nac
    if keep < nac:
        want = dict(want, **{"a.nac": str(keep), "grid": str(groups * keep), "a.xcd_map": str(1 if groups * keep % 8 == 0 else 0)})
    return want


def test_plans_equal_the_launchers_they_replace(plans, fixture_file):
    """A case of the fixture: [id, call, records]; records: per compute-unit count the verdict and, of an accepted call,
    the values of fixture["fields"][kind] in that order (KB1 is the plan's own: the old launchers left it to the kernel)."""
    res, _, _ = plans
    assert fixture_file["n_cu"] == list(N_CU) + [0] and len(fixture_file["cases"]) >= 150
    checked = 0
    for name, call_, records in fixture_file["cases"]:
        kind = call_[0]
        if name in W_GUARD_ONLY:                      # test_the_w_guard_is_the_plans_own
            continue
        for n_cu, rec in zip(fixture_file["n_cu"], records):
            got = dict(res[(name, n_cu, kind)])
            assert int(got.pop("rc")) == rec[0], (name, n_cu)
            if rec[0] != 1 or kind == "ch":           # stream_small_chunks: its verdict is all it returns
                assert got == {}, (name, n_cu)
                continue
            got.pop("KB1")
            want = without_empty_chunks(kind, dict(zip(fixture_file["fields"][kind], rec[1:])))
            assert set(got) == set(want), (name, n_cu, set(got) ^ set(want))
            for k in want:
                assert got[k] == want[k], (name, n_cu, k, got[k], want[k])
            checked += 1
    print("accepted plans compared field by field:", checked)
    assert checked >= 200


def test_fixture_holds_the_edge_list_and_the_gpu_cases(fixture_file):
    have = {c[0]: c[1] for c in fixture_file["cases"]}
    for name, c in edge_list() + ref.plan_calls():
        assert have.get(name) == c, name


def structure(need):
    """full 16-wide tiles, 4-wide strips of a chunk of `need` columns (a remainder of 9..15 is a zero-padded full tile)"""
    nf, rem = divmod(need, 16)
    return (nf, 0) if rem == 0 else (nf, 1) if rem <= 4 else (nf, 2) if rem <= 8 else (nf + 1, 0)


def runs(K1):
    kb = (K1 + 3) // 4
    pad25, pad5 = (kb + 24) // 25 * 25, (kb + 4) // 5 * 5
    return (25, pad25) if pad25 <= pad5 + 1 else (5, pad5)


def check_common(f, c, kind, head):
    nf, st, unr, kb1, ap, nac, ac = (int(f[k]) for k in ("nf", "str", "unr", "KB1", "a.AP", "a.nac", "a.ac"))
    assert (unr, kb1) == runs(c["K1"]) and kb1 % unr == 0 and 4 * kb1 >= c["K1"]
    assert "%d,%d" % (nf, st) in head[kind + "_table"], "no instantiation"
    assert f["name"] == "stream_small%s_kernel<%d, %d, 5, %d>" % ("_sum" if kind == "sss" else "", nf, st, unr)
    assert int(f["lds"]) <= LDS_MAX
    assert ap == 16 * nf + 4 * st >= min(ac, c["A"]) and (nac - 1) * ac < c["A"] <= nac * ac
    assert nac == 1 or ((nf, st) == structure(ac) and ac % 4 == 0)
    for k in ("nb", "J", "K1", "A", "s_j", "w_c", "c_j"):
        assert int(f["a." + k]) == c[k], k
    assert int(f["a.accumulate"]) == c["acc"] and int(f["tables"]) == 1
    assert float(f["flops"]) == 2.0 * c["nb"] * c["J"] * c["K1"] * c["A"]
    assert int(f["a.c_extent"]) == (c["J"] - 1) * c["c_j"] + c["A"]
    return nf, st, unr, kb1, ap, nac, ac


def check_ss(f, c, n_cu, head):
    nf, st, unr, kb1, ap, nac, ac = check_common(f, c, "ss", head)
    assert c["off"] % 8 == 0 and 1 <= c["nb"] <= 32 and c["J"] >= 1024 and nac <= 16
    assert int(f["lds"]) == 4 * (kb1 + 1) * ap * 8
    # the fewest chunks: one fewer has no instantiation or no room
    if nac > 1:
        need = (-(-c["A"] // (nac - 1)) + 3) // 4 * 4
        n2, s2 = structure(need)
        assert n2 + (1 if s2 else 0) > 7 or 4 * (kb1 + 1) * (16 * n2 + 4 * s2) * 8 > LDS_MAX
    ntiles, wpp = (c["J"] + 15) // 16, int(f["a.wpp"])
    assert wpp == max(1, min(n_cu // (c["nb"] * nac), (ntiles + 7) // 8)) and int(f["grid"]) == c["nb"] * wpp * nac
    assert int(f["a.s_extent"]) == (c["J"] - 1) * c["s_j"] + c["K1"]
    # every byte offset the kernel forms: S of the farthest look-ahead (the tile one visit behind a wave's last, its ring of
    # 4 KB1 columns), C of the last row of the last tile -- rows beyond J are formed and masked
    tstep = wpp * 8
    last_visit = ntiles - 1 + tstep
    assert ((last_visit * 16 + 15) * c["s_j"] + 4 * kb1 + 3) * 8 < LIM32
    assert ((ntiles * 16 - 1) * c["c_j"] + c["A"]) * 8 < LIM32
    assert ((c["K1"] - 1) * c["w_c"] + c["A"]) * 8 < LIM32


def check_sss(f, c, n_cu, head):
    nf, st, unr, kb1, ap, nac, ac = check_common(f, c, "sss", head)
    assert c["off"] % 8 == 0 and c["nb"] >= 2 and c["J"] >= 1024 and nac >= 2
    img = 4 * (kb1 + 1) * ap
    assert img <= int(dict(x.split("=") for x in head["const"])["PSI_SUM_IMAGE_MAX"]) == 512 * 12 and int(f["lds"]) == 2 * img * 8
    ntiles = (c["J"] + 15) // 16
    groups = (ntiles + 7) // 8
    assert int(f["a.groups"]) == groups and int(f["grid"]) == groups * nac and int(f["a.xcd_map"]) == (1 if groups * nac % 8 == 0 else 0)
    # chunks grow while they fill the chip in one round and keep a full tile of columns
    assert nac == 2 or nac <= 16 or (groups * nac <= n_cu + n_cu // 8 and -(-c["A"] // nac) >= 16)
    assert int(f["a.s_b"]) == c["s_b"] and int(f["a.w_b"]) == c["w_b"]
    assert int(f["a.s_extent"]) == (c["nb"] - 1) * c["s_b"] + (c["J"] - 1) * c["s_j"] + c["K1"]
    assert int(f["a.w_extent"]) == (c["nb"] - 1) * c["w_b"] + (c["K1"] - 1) * c["w_c"] + c["A"]
    # byte offsets: S of the prefetch into the term behind the last one, W of the last term, C of the last tile
    assert (c["nb"] * c["s_b"] + (ntiles * 16 - 1) * c["s_j"] + 4 * kb1 + 3) * 8 < LIM32
    assert ((c["nb"] - 1) * c["w_b"] + (c["K1"] - 1) * c["w_c"] + c["A"]) * 8 < LIM32
    assert ((ntiles * 16 - 1) * c["c_j"] + c["A"]) * 8 < LIM32


def test_invariants_at_the_dispatch_edges(plans):
    res, head, todo = plans
    accepted = {"ss": 0, "sss": 0}
    assert len(head["ss_table"]) == 19 and len(head["sss_table"]) == 9
    for name, c in edge_list() + ref.plan_calls():
        kind, c = c[0], dict(zip(CALL_KEYS, c[1:]))
        if kind == "ch":
            continue
        for n_cu in N_CU:
            f = dict(res[(name, n_cu, kind)])
            if int(f.pop("rc")) == 1:
                try:
                    (check_ss if kind == "ss" else check_sss)(f, c, n_cu, head)
                except AssertionError as e:
                    raise AssertionError((name, n_cu, f)) from e
                accepted[kind] += 1
        # no compute units: never a plan -- an error where the shape is covered (the guards behind that test may still refuse)
        err = int(dict(x.split("=") for x in head["const"])["ERR_HIP"])
        assert int(res[(name, 0, kind)]["rc"]) in ((err,) if int(res[(name, 256, kind)]["rc"]) == 1 else (err, 0)), name
    print("accepted plans of the edge list and the GPU table:", accepted)
    assert min(accepted.values()) >= 100


def test_the_edges_fall_on_the_sides_they_are_named_for(plans):
    res, _, _ = plans
    v = lambda name, kind="ss", n_cu=256: int(res[(name, n_cu, kind)]["rc"])
    g = lambda name, key, kind="ss", n_cu=256: int(res[(name, n_cu, kind)][key])
    assert [v("ep-nb%d" % nb) for nb in (0, 1, 2, 20, 21, 32, 33)] == [0, 1, 1, 1, 1, 1, 0]
    assert [g("ep-nb%d" % nb, "a.wpp", n_cu=20) for nb in (20, 21)] == [1, 1] and [g("ep-nb%d" % nb, "a.wpp") for nb in (1, 32)] == [8, 8]
    assert [v("ep-J%d" % J) for J in (1023, 1024)] == [0, 1] and [g("ep-J%d" % J, "a.wpp") for J in (1024, 1025, 2048)] == [8, 9, 16]
    assert [v("ep-K%d" % K) for K in (0, 1)] == [0, 1]
    assert [g("ep-K%d" % K, "unr") for K in (1, 20, 21, 80, 81, 100, 101, 180, 181)] == [5, 5, 5, 5, 25, 25, 5, 5, 25]
    assert [v("ep-A%d" % A) for A in (3, 4, 8, 9, 1792, 1793)] == [0, 0, 0, 1, 1, 0]
    assert [(g("ep-A%d" % A, "nf"), g("ep-A%d" % A, "str")) for A in (16, 17, 20, 21, 24, 25)] == [(1, 0), (1, 1), (1, 1), (1, 2), (1, 2), (2, 0)]
    assert [g("ep-A%d" % A, "a.nac") for A in (112, 113, 224, 225)] == [1, 2, 2, 3] and g("ep-A130", "a.ac") == 68
    assert [g("ep-K600-A%d" % A, "a.nac") for A in (32, 33, 64, 512)] == [1, 2, 2, 16] and v("ep-K600-A513") == 0
    assert [g("ep-K%d-A112" % K, "a.nac") for K in (160, 161)] == [1, 2] and [v("ep-K%d-A16" % K) for K in (1260, 1261)] == [1, 0]
    assert [v("ep-" + n) for n in ("sj-1", "wc-1", "cj-1", "pads", "acc", "off4", "off8")] == [0, 0, 0, 1, 1, 0, 1]
    assert [v("ep-" + n) for n in ("sj-under", "sj-over", "cj-under", "cj-over", "wc-under", "wc-over")] == [1, 0, 1, 0, 1, 0]
    s = lambda name: v(name, "sss")
    assert [s("es-nb%d" % nb) for nb in (1, 2, 3, 8, 33, 100)] == [0, 1, 1, 1, 1, 1]
    assert [s("es-J%d" % J) for J in (1023, 1024)] == [0, 1]
    assert [g("es-J%d" % J, "a.xcd_map", "sss") for J in (1024, 1025)] == [1, 0] and g("es-J1025-A128", "a.xcd_map", "sss") == 1
    assert [g("es-J1025-A%d" % A, "grid", "sss") for A in (32, 128)] == [18, 72]
    assert [s("es-K%d" % K) for K in (0, 1, 380, 381)] == [0, 1, 1, 0]
    assert [g("es-K%d" % K, "unr", "sss") for K in (1, 20, 21, 80, 81, 100, 101)] == [5, 5, 5, 5, 25, 25, 5]
    assert [s("es-A%d" % A) for A in (7, 8, 16, 17, 896, 897)] == [0, 0, 0, 1, 1, 0]
    assert [g("es-A%d" % A, "a.nac", "sss") for A in (45, 47, 48, 64)] == [2, 3, 3, 4]
    assert [g("es-A%d" % A, "a.nac", "sss", 20) for A in (48, 64, 896)] == [2, 2, 16]
    assert [g("es-J%d" % J, "a.nac", "sss") for J in (2048, 2049)] == [2, 2]
    assert [g("es-J2049-A%d" % A, "a.nac", "sss") for A in (256, 896)] == [16, 16] and s("es-J2049-A897") == 0
    assert [(g("es-J2049-A%d" % A, "nf", "sss"), g("es-J2049-A%d" % A, "str", "sss")) for A in (256, 257, 896)] == [(1, 0), (1, 1), (3, 2)]
    assert [s("es-" + n) for n in ("sj-1", "wc-1", "cj-1", "sb-1", "wb-1", "sb0", "pads", "acc", "off4")] == [0, 0, 0, 0, 0, 1, 1, 1, 0]
    assert [s("es-" + n) for n in ("sb-under", "sb-over", "wb-under", "wb-over", "cj-under", "cj-over")] == [1, 0, 1, 0, 1, 0]
    c = lambda *kam: int(res[("ec-%d-%d-%d" % kam, 256, "ch")]["rc"])
    assert [c(640, 100, 32), c(640, 100, 3), c(640, 100, 4)] == [4, 0, 4]
    assert [c(168, 100, 32), c(172, 100, 32), c(168, 101, 32), c(168, 104, 32), c(168, 105, 32)] == [1, 0, 2, 2, 2]
    assert [c(642, 20, 32), c(644, 20, 32), c(6, 20, 32), c(8, 20, 32)] == [0, 1, 0, 1]
    assert [c(6400, 100, 32), c(6400, 100, 64), c(3200, 100, 32), c(0, 100, 32), c(640, 100, 0)] == [0, 0, 20, 1, 0]


# ------------------------------------------------------------------------------------- (c) the table of the GPU test
def test_tags_equal_the_plans(plans):
    res, head, _ = plans
    n = 0
    for c in ref.all_cases():
        f = dict(res[(c.id, 256, c.kind)])
        assert int(f.pop("rc")) == 1, c.id
        assert ref.tags_of_plan(c.kind, f) == ref.TAGS[c.id], (c.id, ref.tags_of_plan(c.kind, f))
        assert f["name"] == ref.expected_name(c), c.id
        n += 1
    print("plans compared with their tags:", n)


def test_table_covers_both_launch_tables_and_every_branch(plans):
    _, head, _ = plans
    cases = ref.all_cases()
    ids = [c.id for c in cases + ref.refusals()]
    assert len(set(ids)) == len(ids) and set(ref.TAGS) == {c.id for c in cases}
    tag = lambda c: dict(kv.split("=") for kv in ref.TAGS[c.id].split())
    for kind in ("ss", "sss"):
        mine = [c for c in cases if c.kind == kind]
        want = {(x, unr) for x in head[kind + "_table"] for unr in ("5", "25")}
        seen = {("%s,%s" % (t["nf"], t["str"]), t["unr"]) for t in map(tag, mine)}
        assert seen == want, "instantiations no case reaches: %s" % sorted(want - seen)
        seen = {k: {tag(c)[k] for c in mine} for k in ref.BRANCHES[kind]}
        missing = {k: sorted(set(w.split()) - seen[k]) for k, w in ref.BRANCHES[kind].items() if set(w.split()) - seen[k]}
        assert not missing, "plan branches no case reaches: %s" % missing
        for opt in ref.OPTIONS[kind]:
            assert any(c.opts.get(opt) for c in mine), (kind, opt)
        assert {c.opts.get("acc", 0) for c in mine} == {0, 1}
    assert {c.nb for c in cases if c.kind == "ss"} >= {1, 2, 32} and {c.nb for c in cases if c.kind == "sss"} >= {2, 3, 8}
    assert {c.J for c in cases if c.kind == "ss"} >= {1024, 1025, 1039, 1041} and {c.J for c in cases if c.kind == "sss"} >= {1024, 1025, 1039, 1041}
    assert {c.K1 for c in cases if c.kind == "ss"} >= {1, 3, 4, 5, 20, 21, 80, 81, 100, 101, 600}
    assert {c.K1 for c in cases if c.kind == "sss"} >= {1, 3, 4, 5, 20, 21, 80, 81, 100, 101}
    over = {c.id for c in cases if ref.macs(c) > ref.BUDGET}
    assert not over, over
    # a wave of the nb = 32 case visits a second tile, another does not
    c = next(c for c in cases if c.id == "p-nb32-wrap")
    ntiles, tstep = (c.J + 15) // 16, int(tag(c)["wpp"]) * 8
    assert tstep < ntiles < 2 * tstep and int(tag(c)["wpp"]) == 8


def test_cases_beyond_the_cover_are_refused_by_the_plan(plans):
    res, _, _ = plans
    for c in ref.refusals():
        assert c.opts.get("refuse") and int(res[(c.id, 256, c.kind)]["rc"]) == 0, c.id


# ---------------------------------------------------------------------------------------------------- the checker
SMALL = ("p-A17", "p-pads-acc", "s-nb3", "s-pads-acc")


def _case(id):
    return next(c for c in ref.all_cases() if c.id == id)


def defects(c, vals):
    """(name, C buffers): the float64 result with one defect each"""
    S, W, prior = vals
    b = c.nb - 1
    ob = b if c.kind == "ss" else 0

    def fresh():
        out = ref.float64_result(c, vals)
        return out, ref.c_views(c, out)

    out, V = fresh()
    j, a = c.J - 1, c.A - 1
    terms = S[b][j, :] * W[b][:, a]
    k = int(np.argmax(np.abs(terms)))
    assert terms[k] != 0
    V[ob][j, a] -= terms[k]
    yield "one k term dropped from one element", out
    out, V = fresh()
    V[ob][c.J - 1, c.A - 1] = np.uint64(ref.SENT).view(np.float64)
    yield "one element left at the sentinel", out
    out, V = fresh()
    V[ob][15, :] = V[ob][14, :]
    yield "a row tile's last row taken from the row above", out
    out, V = fresh()
    k = int(np.argmax(np.abs(W[b][:, c.A - 1])))
    assert W[b][k, c.A - 1] != 0 and S[b][:, k].any()
    V[ob][:, c.A - 1] += S[b][:, k] * W[b][k, c.A - 1]
    yield "one k counted twice in the last column", out
    out, V = fresh()
    out[ob][ref.PRE - 1] = 0.0
    yield "a store in front of C", out
    out, V = fresh()
    out[ob][-ref.POST] = V[ob][0, 0]
    yield "a store behind C", out
    if c.opts.get("c_pad"):
        out, V = fresh()
        out[ob][ref.PRE + c.A] = 1.0
        yield "a store into the row padding of C", out
    if c.opts.get("acc"):
        out, V = fresh()
        V[ob][3, 1] -= prior[ob][3, 1]
        yield "one element stored, not accumulated", out


@pytest.mark.parametrize("id", SMALL)
@pytest.mark.parametrize("integer", (True, False), ids=("integer", "gaussian"))
def test_checker_rejects_one_wrong_piece_and_accepts_float64(id, integer):
    c = _case(id)
    vals = ref.values(c, integer, 7)
    tr = ref.truth(c, vals, integer)
    ref.check_results(c, ref.float64_result(c, vals), tr, integer)
    rejected = 0
    for name, out in defects(c, vals):
        with pytest.raises(AssertionError):
            ref.check_results(c, out, tr, integer, what=name)
        rejected += 1
    assert rejected >= 6


def test_checker_sees_a_name_that_is_off_and_a_written_refused_call():
    c = _case("p-A17")
    assert ref.expected_name(c) == "stream_small_kernel<1, 1, 5, 5>" != ref.expected_name(_case("p-A21"))
    assert ref.expected_name(_case("s-nb3")).startswith("stream_small_sum_kernel<")
    r = ref.refusals()[0]
    out = ref.sentinels(r)
    ref.check_untouched(r, out, r.id)
    out[0][ref.PRE + 3] = 0.0
    with pytest.raises(AssertionError):
        ref.check_untouched(r, out, r.id)


def test_the_nan_gap_cases_pin_the_documented_contract():
    """csrc/stream_small.h: a non-finite element of S behind a row, inside the descriptor, makes that row NaN and no other.
    The expectation of the direct cases is formed here from a float64 result, so that the GPU test asserts it as it stands."""
    for c in ref.all_cases():
        if not c.opts.get("nan_gap"):
            continue
        assert c.kind == "sss" and c.K1 % 2 == 1 and c.opts.get("s_gap", 0) >= 1 and c.nb >= 3
        g = ref.geometry(c)
        hS = ref.operands(c, ref.values(c, False, 3))[0]
        nan_at = np.flatnonzero(np.isnan(hS[0]))
        assert nan_at.tolist() == [ref.PRE + b * g["s_b"] + c.J * g["s_j"] for b in range(c.nb - 1)]      # the gap doubles, and only they
        vals = ref.values(c, False, 3)
        tr = ref.truth(c, vals, False)
        out = ref.float64_result(c, vals)
        with pytest.raises(AssertionError):
            ref.check_results(c, out, tr, False)             # a finite last row is NOT what the contract says
        ref.c_views(c, out)[0][c.J - 1, :] = np.nan
        ref.check_results(c, out, tr, False)
        ref.c_views(c, out)[0][c.J - 2, 0] = np.nan
        with pytest.raises(AssertionError):
            ref.check_results(c, out, tr, False)
