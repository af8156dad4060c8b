"""What tests/test_gpu_dense_pass_edges.py runs on the device, checked on the host first (no GPU).

(a) Its case tables (tests/dense_pass_ref.py) go through dense_first_plan / dense_left_plan (csrc/dense_pass_plan.h, plain
    C++): a short driver compiled with the host compiler prints every field of what they decide.  Every accepted case
    carries tags, the plan fields it is meant to reach; each must equal what the plan decides, and the plan must hold the
    invariants the kernels rely on.  The union of the tags must cover the branch lists; every case meant to be refused
    must be refused with its message; no case asks for more scratch than its poison shape.
(b) The checker itself: from the truth of three small cases, "kernel results" with one defect each.  The integer and the
    Gaussian check must reject every one and accept the float64 result."""

import numpy as np
import pytest

from tests import dense_pass_ref as ref
from tests.host_driver import compile_driver, run_driver

TTSK_ERR_UNSUPPORTED = -3
LDS_MAX = 160 * 1024

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "dense_pass_plan.h"
using namespace ttsk;

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char id[128], kind[8];
    long long v[6];
    while (fscanf(f, "%127s %7s", id, kind) == 2) {
        for (int i = 0; i < 6; ++i)
            if (fscanf(f, "%lld", &v[i]) != 1) return 3;
        if (kind[0] == 'F') {
            DenseFirstPlan p;
            const int rc = dense_first_plan(v[0], v[1], v[2], v[3], v[4], (unsigned)v[5], &p);
            printf("%s rc=%d", id, rc);
            if (!rc)
                printf(" one_kind=%d split=%d p_half=%d z_half=%d NBW=%d TP=%d SP=%d ZT=%d ZS=%d NB=%d nbb=%d nt=%d nqc=%d nqc_want=%d kinds=%d"
                       " grid1=%lld grid=%lld sl64=%lld pr=%lld lds=%zu slab_bytes=%zu pad_bytes=%zu zblock=%lld zpart_bytes=%zu elems=%lld"
                       " p_off0=%d p_off1=%d pcount0=%d pcount1=%d z_off0=%d z_off1=%d zcount0=%d zcount1=%d prow=%d",
                       (int)p.one_kind, (int)p.split, p.p_half, p.z_half, p.NBW, p.TP, p.SP, p.ZT, p.ZS, p.NB, p.nbb, p.nt, p.nqc, p.nqc_want, p.kinds,
                       (long long)p.grid1, (long long)p.grid, (long long)p.sl64, (long long)p.pr, p.lds, p.slab_bytes, p.pad_bytes, (long long)p.zblock,
                       p.zpart_bytes, (long long)p.elems, p.p_off[0], p.p_off[1], p.pcount[0], p.pcount[1], p.z_off[0], p.z_off[1], p.zcount[0], p.zcount[1],
                       dp_prow(p.TP, p.SP));
            printf(" | %s\n", p.msg);
        } else {
            DenseLeftPlan p;
            const int rc = dense_left_plan(v[0], v[1], v[2], v[3], v[4], (int)v[5], &p);
            printf("%s rc=%d", id, rc);
            if (!rc)
                printf(" ni3=%d nct=%d xcd_map=%d strip=%d nsets=%d ninstr=%d grid=%lld lds=%zu slab=%lld scratch_bytes=%zu flops=%.17g LP_CT=%d LP_XP=%d",
                       p.ni3, p.nct, p.xcd_map, p.strip, p.nsets, p.ninstr, (long long)p.grid, p.lds, (long long)p.slab, p.scratch_bytes, p.flops, LP_CT,
                       LP_XP);
            printf(" | %s\n", p.msg);
        }
    }
    return 0;
}
"""


def parse(text):
    res = {}
    for line in text.splitlines():
        head, msg = line.split(" | ", 1) if " | " in line else (line.rstrip(" |"), "")
        w = head.split()
        res[w[0]] = (dict((k, float(x) if k == "flops" else int(x)) for k, x in (kv.split("=") for kv in w[1:])), msg)
    return res


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "dense_pass_plan", DRIVER)
    cases = exe.parent / "cases.txt"
    todo = ref.all_cases() + ref.refusals() + [ref.POISON_FIRST, ref.POISON_LEFT]
    cases.write_text("".join("%s %s\n" % (c.id, ref.plan_call(c)) for c in todo))
    return parse(run_driver(exe, [cases]))


def check_first(c, f):
    """what dense_pass_kernel, dense_pass_reduce and dense_pass_zsum rely on"""
    assert (f["NB"], f["nt"], f["pr"]) == (8 * f["NBW"], c.T // 16, c.r + c.r % 2) and c.n0 == f["nbb"] * f["NB"]
    assert f["kinds"] == (2 if f["split"] else 1) and not (f["split"] and f["one_kind"])
    assert f["grid1"] == f["nbb"] * f["nt"] * f["nqc"] and f["grid"] == f["grid1"] * f["kinds"] and f["grid"] < 2 ** 31
    # every kind's accumulators hold the columns of U and the rows of Z it owns; the kinds' ranges partition r and ll
    cols, rows, ucap, zcap = [], [], 16 * f["TP"] + 4 * f["SP"], 16 * f["ZT"] + 4 * f["ZS"]
    for k in range(f["kinds"]):
        p_off, z_off = f["p_off%d" % k], f["z_off%d" % k]
        assert (p_off, z_off) == (k * f["p_half"], k * f["z_half"])          # what the kernel adds to its column and row indices
        cols += list(range(p_off, p_off + max(f["pcount%d" % k], 0)))
        rows += list(range(z_off, z_off + max(f["zcount%d" % k], 0)))
        assert f["pcount%d" % k] <= ucap and f["zcount%d" % k] <= zcap, (k, f)
    assert cols == list(range(c.r)) and rows == list(range(c.ll)), (cols, rows)
    if f["kinds"] == 1:
        assert f["pcount1"] == 0 and f["zcount1"] == 0
    # the P image: every 16-byte unit a tile or strip reads lies inside a row of the image, the rows are brought by whole waves
    assert f["prow"] >= ucap and (8 * f["prow"] // 2) % 64 == 0 and 8 * f["prow"] // 2 <= 512
    assert f["lds"] == 8 * (2 * f["NB"] * 128 + 16 * f["prow"] + f["NB"] * zcap) <= LDS_MAX
    # the q chunks partition the tiles; nqc is a multiple of 8 (the block-id decode) and at most the capped wish
    ch = ref.chunks(c.Q, f["nqc"])
    assert f["nqc"] % 8 == 0 and 8 <= f["nqc"] <= f["nqc_want"]
    assert [t for beg, n, _ in ch for t in range(beg, beg + n)] == list(range(c.Q // 8))
    assert all(0 <= rot < max(n, 1) for _, n, rot in ch)
    # the block-id decode reaches every (t range, q chunk) of a block of rows once
    seen = {((idl >> 3) % f["nt"], (idl & 7) + 8 * (idl // (8 * f["nt"]))) for idl in range(f["nt"] * f["nqc"])}
    assert seen == {(tr, qc) for tr in range(f["nt"]) for qc in range(f["nqc"])}
    # scratch and the launches behind the pass
    assert f["sl64"] == 64 * (4 * f["TP"] + f["SP"]) and f["slab_bytes"] == 8 * f["grid"] * f["NB"] * f["sl64"] <= 4 << 30
    assert f["pad_bytes"] == (8 * c.Q * f["pr"] + 64 if c.r % 2 else 0)
    assert f["zblock"] == c.ll * c.Q * c.T and f["zblock"] % 2 == 0 and 3 * c.Q * c.T * 8 < 2 ** 32
    assert f["zpart_bytes"] == (8 * f["nbb"] * f["zblock"] if f["nbb"] > 1 else 0) <= 4 << 30
    assert f["elems"] == f["NB"] * f["sl64"] * f["nt"] * f["nbb"]


def check_left(c, f):
    C = c.n3 * c.n4
    assert f["LP_CT"] == 512 and f["ni3"] * c.n4 == 512 and f["nct"] * 512 == C and f["nsets"] == 3 + f["ni3"]
    assert f["ninstr"] == -(-40 * f["nsets"] // 64) and 1 <= f["ninstr"] <= 7          # wave m issues instruction m: fewer than the 8 waves
    assert f["grid"] == c.n2 * f["nct"] and f["xcd_map"] == int(c.n2 % 8 == 0) and f["strip"] == int(c.l > 16)
    aimg = (f["nsets"] * 80 + 127) // 128 * 128 + 128
    assert 128 * f["ninstr"] <= aimg and f["lds"] == 8 * (16 * f["LP_XP"] + 4 * aimg) <= LDS_MAX
    assert f["slab"] == c.n2 * c.l * C and f["scratch_bytes"] == 16 * f["slab"] + 64
    assert f["flops"] == 8.0 * c.l * c.n0 * c.n1 * c.n2 * C


def test_tags_equal_the_plans(plans):
    n = 0
    seen = {}
    for c in ref.all_cases():
        f, msg = plans[c.id]
        assert f.pop("rc") == 0 and msg == "", (c.id, msg)
        tags = ref.tags_of_plan(c, f)
        assert tags == ref.TAGS[c.id], (c.id, tags)
        try:
            (check_first if c.kind == "first" else check_left)(c, f)
        except AssertionError as e:
            raise AssertionError((c.id, f)) from e
        for kv in tags.split():
            k, v = kv.split("=")
            seen.setdefault((c.kind, k), set()).add(v)
        n += 1
    print("plans compared with their tags:", n)
    for (kind, k), v in sorted(seen.items()):
        print("  %s %s: %s" % (kind, k, " ".join(sorted(v))))


def test_tables_cover_every_branch():
    cases = ref.all_cases()
    ids = [c.id for c in cases + ref.refusals()]
    assert len(set(ids)) == len(ids) and set(ref.TAGS) == {c.id for c in cases}
    tag = lambda c: dict(kv.split("=") for kv in ref.TAGS[c.id].split())
    seen = {kind: {k: set() for k in b} for kind, b in ref.BRANCHES.items()}
    for c in cases:
        for k, v in tag(c).items():
            if k in seen[c.kind]:
                seen[c.kind][k].add(v)
            if k == "lens" and "3" in v.split("+"):
                seen[c.kind][k].add("3")
    missing = {(kind, k): sorted(set(want.split()) - seen[kind][k]) for kind, b in ref.BRANCHES.items() for k, want in b.items()}
    missing = {k: v for k, v in missing.items() if v}
    assert not missing, "plan branches no case reaches: %s" % missing
    first = [c for c in cases if c.kind == "first"]
    left = [c for c in cases if c.kind == "left"]
    # both sides of every rank edge, with whole blocks of 64 rows (the one-kind and the split forms) and with blocks of 32
    whole, half = [c for c in first if c.n0 % 64 == 0], [c for c in first if c.n0 % 64]
    assert {c.r for c in whole} >= {1, 33, 40, 41, 44, 45, 48, 49, 64} and {c.ll for c in whole} >= {1, 17, 20, 21, 24, 25, 32}
    assert {c.r for c in half} >= {1, 33, 40, 41, 48, 49, 64} and {c.ll for c in half} >= {1, 17, 20, 21, 32}
    # an odd r (the padded copy of P) in every shape of the U accumulators
    ushape = lambda c: tag(c)["inst"].split(".")[1:3]
    assert {tuple(ushape(c)) for c in first if c.r % 2} == {tuple(ushape(c)) for c in first} and len({tuple(ushape(c)) for c in first}) == 6
    # a split over several blocks of rows; a rotated chunk under a split; the limit of the first mode
    assert any(tag(c)["kind"] == "split" and c.n0 > 64 for c in first) and any(tag(c)["kind"] == "split" and tag(c)["rot"] == "1" for c in first)
    assert any(tag(c)["kind"] == "one" and c.n0 > 64 for c in first)
    assert any(c.n0 == 4096 for c in first)
    # U and C 8 bytes off, in the plain form, under a split and with blocks of 32
    off = [c for c in first if c.opts.get("uoff") and c.opts.get("coff")]
    assert {tag(c)["kind"] for c in off} >= {"plain", "split"} and {c.n0 % 64 for c in off} == {0, 32}
    # the left pass: the rank edges, Z_0 flushed once and several times, one and several k-blocks per i1, one to four k-blocks
    assert {c.l for c in left} >= {1, 16, 17, 20} and {c.n1 for c in left} >= {1, 2} and {c.n0 for c in left} >= {4, 12}
    assert {c.n2 for c in left} >= {1, 3, 8, 16} and {c.n4 for c in left} == {64, 128, 256, 512}
    assert {min(c.n1 * c.n0 // 4, 4) for c in left} == {1, 2, 3, 4}
    # sizes: no X beyond 2^22 doubles, most below 2^18
    size = lambda c: c.n0 * c.Q * c.T if c.kind == "first" else c.n0 * c.n1 * c.n2 * c.n3 * c.n4
    assert all(size(c) <= 2 ** 22 for c in cases) and 2 * sum(size(c) < 2 ** 18 for c in cases) > len(cases)


def test_cases_beyond_the_cover_are_refused_with_their_message(plans):
    assert {c.id[2:] for c in ref.first_refusals()} >= {"n48", "n4128", "T24", "Q10", "l33", "r65", "QT27", "partials", "xoff8", "poff8", "zoff8"}
    assert {c.id[2:] for c in ref.left_refusals()} >= {"n6", "C500", "n4-32", "n4-48", "l21", "n2-big"}
    for c in ref.refusals():
        f, msg = plans[c.id]
        assert f == {"rc": TTSK_ERR_UNSUPPORTED}, (c.id, f)
        if c.kind == "left":
            want = "ttsk_dense_left_pass: shape (%d, %d, %d, C = %d, n4 = %d), l = %d is outside the kernel's cover" % (
                c.n0, c.n1, c.n2, c.n3 * c.n4, c.n4, c.l)
        elif c.opts.get("msg") == "partial":
            want = "ttsk_dense_first_pass: 40 blocks of rows would need more than 4 GB of partial results"
        else:
            want = ("ttsk_dense_first_pass: shape outside the kernel's cover (first mode a multiple of 32, last mode a multiple of 16, "
                    "middle extent a multiple of 8, left rank <= 32, right rank <= 64)")
        assert msg == want, (c.id, msg)


def test_no_case_needs_more_scratch_than_its_poison_shape(plans):
    pf, pl = plans[ref.POISON_FIRST.id][0], plans[ref.POISON_LEFT.id][0]
    assert pf["rc"] == 0 and pl["rc"] == 0 and pf["nbb"] > 1
    # the poison call leaves no zero behind: a workgroup stores its accumulators whether or not its q chunk had a tile, so
    # every chunk must own one; every slot of the slab must be a column of U in use, every row of the partial Z a row in use
    p = ref.POISON_FIRST
    assert min(n for _, n, _ in ref.chunks(p.Q, pf["nqc"])) >= 1
    assert pf["kinds"] == 1 and pf["pcount0"] == p.r == 16 * pf["TP"] and pf["SP"] == 0 and pf["sl64"] == 64 * 4 * pf["TP"]
    assert pf["zcount0"] == p.ll and pf["zpart_bytes"] == 8 * pf["nbb"] * p.ll * p.Q * p.T
    # left pass: the kernel stores rows a < l of both slabs for every i2 and column; the slabs are [i2][l][C]
    assert pl["slab"] == ref.POISON_LEFT.n2 * ref.POISON_LEFT.l * ref.POISON_LEFT.n3 * ref.POISON_LEFT.n4
    for c in ref.all_cases():
        f = plans[c.id][0]
        if c.kind == "first":
            assert f["slab_bytes"] <= pf["slab_bytes"] and f["slab_bytes"] + f["pad_bytes"] <= pf["slab_bytes"] + pf["pad_bytes"], c.id
            assert f["zpart_bytes"] <= pf["zpart_bytes"], c.id
        else:
            assert f["scratch_bytes"] <= pl["scratch_bytes"], c.id


# ---------------------------------------------------------------------------------------------------- the checker
SMALL = ("d-r40", "d-n128", "e-n4-64-ct2")


def _case(id):
    return next(c for c in ref.all_cases() if c.id == id)


def defects(c, v):
    """(name, output buffers): the float64 result with one defect each"""
    sent = np.uint64(ref.SENT).view(np.float64)
    names = ref.OUT_NAMES[c.kind]

    def fresh():
        out = ref.float64_result(c, v)
        return out, {n: ref.view(c, n, out[n]) for n in names}

    for n in names:
        out, V = fresh()
        i = tuple(s - 1 for s in V[n].shape)
        V[n][i] += max(abs(V[n][i]), 1.0) * 2.0 ** -30
        yield "one wrong element of %s" % n, out
        out, V = fresh()
        V[n][tuple(s // 2 for s in V[n].shape)] = sent
        yield "one element of %s left at the sentinel" % n, out
        out, V = fresh()
        out[n][ref.PRE - 1] = 0.0
        yield "a store in front of %s" % n, out
        out, V = fresh()
        out[n][-ref.POST] = V[n].reshape(-1)[0]
        yield "a store behind %s" % n, out
    if c.kind == "first":
        X, C, P = v["X"], v["C"], v["P"]
        out, V = fresh()
        V["U"][c.n0 - 1, :16, :16] = V["U"][c.n0 - 1, :16, :16].T.copy()
        yield "p and t transposed within a tile of U", out
        out, V = fresh()
        V["U"][...] -= np.einsum("qp,bqt->bpt", P[8:16], X[:, 8:16, :])
        yield "one q chunk missing from U", out
        out, V = fresh()
        V["Z"][...] -= np.einsum("bp,bqt->pqt", C[:32], X[:32])
        yield "one block of rows missing from Z", out
    else:
        out, V = fresh()
        V["E3"][:, [0, 1], :] = V["E3"][:, [1, 0], :]
        assert out["E3"].size and np.allclose(V["E3"].sum(axis=1), ref.float64_result(c, v)["E3"][ref.PRE:-ref.POST].reshape(V["E3"].shape).sum(axis=1))
        yield "two i3 of E3 swapped (the sum over i3 is the same)", out


@pytest.mark.parametrize("id", SMALL)
@pytest.mark.parametrize("integer", (True, False), ids=("integer", "gaussian"))
def test_checker_rejects_one_wrong_piece_and_accepts_float64(id, integer):
    c = _case(id)
    v = ref.values(c, integer, 7)
    tr = ref.truth(c, v, integer)
    ref.check_results(c, ref.float64_result(c, v), tr, integer)
    rejected = 0
    for name, out in defects(c, v):
        with pytest.raises(AssertionError):
            ref.check_results(c, out, tr, integer, what=name)
        rejected += 1
    assert rejected == (4 * 2 + 3 if c.kind == "first" else 4 * 4 + 1)


def test_checker_sees_a_write_by_a_refused_call():
    c = ref.first_refusals()[0]
    out = ref.sentinels(c)
    ref.check_untouched(out, c.id)
    out["U"][3] = 0.0
    with pytest.raises(AssertionError):
        ref.check_untouched(out, c.id)
