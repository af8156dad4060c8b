"""The host plans of the three vector entry points (csrc/vector_plan.h, plain C++): a short driver compiled with the host
compiler reads case lines and prints every field of what copy_strided_plan / sum_slices_plan / axpby_plan decide; each
field is recomputed here, independently -- before any kernel reads it, and before tests/test_gpu_vector_ops.py hands the
library a NULL pointer or an oversize extent.

(a) every refusal of tests/vector_ops_ref.py, with its status and a fragment of its message; the calls with nothing to do;
(b) the copy's padding of ndim < 5 and its grid on either side of the cap; the route of the slice sum with each of its four
    conditions broken alone and its grid at both caps; the axpby grid; sizes no device could hold (the overflow refusals,
    a size_t near its end);
(c) every case the GPU module runs goes through the plan: it is accepted, takes the route its name says, and the cap cases
    make the trips of the grid-stride loop they are there for.
The driver is built once more with AddressSanitizer and UBSan as a stand-alone program and must print the same."""
import pytest

from tests import vector_ops_ref as ref
from tests.host_driver import compile_driver, run_driver

DRIVER = r"""
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "vector_plan.h"
using namespace ttsk;

static void list(const char *name, const int64_t *v)
{
    printf(" %s=", name);
    for (int i = 0; i < 5; ++i) printf("%s%lld", i ? "," : "", (long long)v[i]);
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    printf("const T=%d DIMS=%d COPY=%lld AXPBY=%lld SUM=%lld OK=%d ARG=%d UNSUPPORTED=%d\n", VEC_THREADS, COPY_MAX_DIMS, (long long)COPY_BLOCKS_MAX,
           (long long)AXPBY_BLOCKS_MAX, (long long)SUM_SLICES_BLOCKS_MAX, (int)TTSK_OK, (int)TTSK_ERR_ARG, (int)TTSK_ERR_UNSUPPORTED);
    char id[128], kind[16];
    while (fscanf(f, "%127s %15s", id, kind) == 2) {
        if (!strcmp(kind, "copy")) {
            // dst src ndim has_shape has_ds has_ss, then 8 extents, 8 dst strides, 8 src strides (the first ndim are meant)
            unsigned long long dst, src;
            int ndim, has[3];
            int64_t v[3][8];
            if (fscanf(f, "%llx %llx %d %d %d %d", &dst, &src, &ndim, &has[0], &has[1], &has[2]) != 6) return 3;
            for (int k = 0; k < 3; ++k)
                for (int i = 0; i < 8; ++i)
                    if (fscanf(f, "%" SCNd64, &v[k][i]) != 1) return 3;
            CopyPlan p;
            memset(&p, 0x5a, sizeof(p));
            const int rc = copy_strided_plan((const double *)(uintptr_t)dst, (const double *)(uintptr_t)src, ndim, has[0] ? v[0] : nullptr,
                                             has[1] ? v[1] : nullptr, has[2] ? v[2] : nullptr, &p);
            printf("%s rc=%d blocks=%lld total=%lld", id, rc, (long long)p.blocks, (long long)p.c.total);
            if (rc == TTSK_OK) { list("shape", p.c.shape); list("ds", p.c.ds); list("ss", p.c.ss); }
            printf(" msg=%s\n", p.msg);
        } else if (!strcmp(kind, "sum")) {
            unsigned long long dst, src, stride, n;
            int nb, acc;
            if (fscanf(f, "%llx %llx %d %llu %llu %d", &dst, &src, &nb, &stride, &n, &acc) != 6) return 3;
            SumSlicesPlan p;
            memset(&p, 0x5a, sizeof(p));
            const int rc = sum_slices_plan((const double *)(uintptr_t)dst, (const double *)(uintptr_t)src, nb, (size_t)stride, (size_t)n, acc, &p);
            printf("%s rc=%d blocks=%lld vector=%d stride=%zu n=%zu msg=%s\n", id, rc, (long long)p.blocks, p.vector, p.stride, p.n, p.msg);
        } else if (!strcmp(kind, "axpby")) {
            unsigned long long y, x, n;
            if (fscanf(f, "%llx %llx %llu", &y, &x, &n) != 3) return 3;
            AxpbyPlan p;
            memset(&p, 0x5a, sizeof(p));
            const int rc = axpby_plan((const double *)(uintptr_t)y, (const double *)(uintptr_t)x, 1.5, 0.0, (size_t)n, &p);
            printf("%s rc=%d blocks=%lld msg=%s\n", id, rc, (long long)p.blocks, p.msg);
        } else {
            return 4;
        }
    }
    fclose(f);
    return 0;
}
"""

T, CB, AB, SB = ref.T, ref.K["COPY_BLOCKS_MAX"], ref.K["AXPBY_BLOCKS_MAX"], ref.K["SUM_SLICES_BLOCKS_MAX"]
DST, SRC = ref.FAKE_BASE, ref.FAKE_BASE + (1 << 32)               # never dereferenced
STATUS = {"ok": "OK", "arg": "ARG", "unsupported": "UNSUPPORTED"}


def pad8(v, fill=1):
    v = [int(x) for x in v]
    return v + [fill] * (8 - len(v))


def copy_line(ndim, shape, ds=None, ss=None, dst=DST, src=SRC, null=()):
    ds = ref.c_strides([max(n, 1) for n in shape]) if ds is None else ds
    ss = ds if ss is None else ss
    has = [int(k not in null) for k in ("shape", "ds", "ss")]
    nums = [ndim] + has + pad8(shape, 99) + pad8(ds, 77) + pad8(ss, 55)             # the slots behind ndim hold values a plan that read them would show
    return "copy %x %x %s" % (0 if "dst" in null else dst, 0 if "src" in null else src, " ".join(map(str, nums)))


def sum_line(nb, stride, n, acc, dst=DST, src=SRC, null=()):
    return "sum %x %x %d %d %d %d" % (0 if "dst" in null else dst, 0 if "src" in null else src, nb, stride, n, acc)


def axpby_line(n, y=DST, x=SRC, null=()):
    return "axpby %x %x %d" % (0 if "y" in null else y, 0 if "x" in null else x, n)


def case_addr(base, off):
    return base + 8 * (ref.GUARD + off)


# ---- (b) the edges that are the plans' own
COPY_TOTALS = (1, T, T + 1, T * CB, T * CB + 1)
SUM_ROUTES = {                          # name -> (n, stride, dst offset in bytes, src offset in bytes, vector route?)
    "all-hold": (512, 518, 0, 0, 1),
    "odd-n": (511, 518, 0, 0, 0),
    "odd-stride": (512, 519, 0, 0, 0),
    "dst-off8": (512, 518, 8, 0, 0),
    "src-off8": (512, 518, 0, 8, 0),
    "both-off8": (512, 518, 8, 8, 0),
    "dst-off16": (512, 518, 16, 0, 1),
    "n2": (2, 2, 0, 0, 1),
    "n1": (1, 2, 0, 0, 0),
    "stride0": (512, 0, 0, 0, 1),
}
SUM_BLOCKS = {                          # n -> (vector route?, workgroups) on either side of both caps
    2 * T * (SB - 1): (1, SB - 1), 2 * T * (SB - 1) + 2: (1, SB), 2 * T * SB - 2: (1, SB), 2 * T * SB: (1, SB), 2 * T * SB + 2: (1, SB), 8 * T * SB: (1, SB),
    T * SB - 1: (0, SB), T * (SB - 1) + 1: (0, SB), T * (SB - 1) - 1: (0, SB - 1), T * SB + 1: (0, SB), 8 * T * SB + 1: (0, SB),
    2: (1, 1), 2 * T: (1, 1), 2 * T + 2: (1, 2), 1: (0, 1), T - 1: (0, 1), T + 1: (0, 2),
}
AXPBY_BLOCKS = {1: 1, T - 1: 1, T: 1, T + 1: 2, T * (AB - 1) + 1: AB, T * AB: AB, T * AB + 1: AB, 2 * T * AB + 3: AB, (1 << 64) - 1: AB, (1 << 64) - 255: AB}


def all_lines():
    """{id: case line}"""
    L = {}
    for r in ref.copy_refusals():
        ndim, shape = r.args
        L["copy-refusal-" + r.id] = copy_line(ndim, shape, null=r.null)
    for r in ref.sum_refusals():
        nb, acc, n = r.args
        L["sum-refusal-" + r.id] = sum_line(nb, n, n, acc, null=r.null)
    for r in ref.axpby_refusals():
        L["axpby-refusal-" + r.id] = axpby_line(r.args[0], null=r.null)
    for nd in range(6):
        L["copy-pad-%d" % nd] = copy_line(nd, (3, 4, 5, 6, 7)[:nd], ds=(11, 12, 13, 14, 15)[:nd], ss=(21, 22, 23, 24, 25)[:nd])
    for t in COPY_TOTALS:
        L["copy-total-%d" % t] = copy_line(1, (t,))
        L["copy-total2-%d" % t] = copy_line(3, (1, t, 1))
    L["copy-largest"] = copy_line(1, ((1 << 63) - 1 - T * CB,))             # the largest total with a grid stride to spare
    L["copy-largest+"] = copy_line(2, ((1 << 62) - T * CB // 2, 2))
    for name, (n, stride, doff, soff, _) in SUM_ROUTES.items():
        for acc in (0, 1):
            L["sum-route-%s-%d" % (name, acc)] = sum_line(9, stride, n, acc, DST + doff, SRC + soff)
    for n in SUM_BLOCKS:
        L["sum-blocks-%d" % n] = sum_line(1, n, n, 0)
    for n in AXPBY_BLOCKS:
        L["axpby-blocks-%d" % n] = axpby_line(n)
    for c in ref.copy_cases():
        L["copy-case-" + c.id] = copy_line(len(c.shape), c.shape, c.ds, c.ss, case_addr(DST, c.doff), case_addr(SRC, c.soff))
    for c in ref.sum_cases() + ref.sum_cap_cases():
        L["sum-case-" + c.id] = sum_line(c.nb, c.stride, c.n, c.acc, case_addr(DST, c.doff), case_addr(SRC, c.soff))
    for c in ref.axpby_cases():
        L["axpby-case-" + c.id] = axpby_line(c.n, case_addr(DST, c.yoff), case_addr(DST if c.alias else SRC, c.xoff))
    return L


def parse(text):
    out, head = {}, None
    for line in text.splitlines():
        line, _, msg = line.partition(" msg=")
        w = line.split()
        f = dict(x.split("=", 1) for x in w[1:])
        if w[0] == "const":
            head = {k: int(v) for k, v in f.items()}
            continue
        f["msg"] = msg
        out[w[0]] = f
    return out, head


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    lines = all_lines()
    text = "".join("%s %s\n" % kv for kv in lines.items())
    exe = compile_driver(tmp_path_factory, "vector_plan", DRIVER)
    txt = exe.parent / "cases.txt"
    txt.write_text(text)
    stdout = run_driver(exe, [txt])
    res, head = parse(stdout)
    assert set(res) == set(lines)
    return res, head, stdout, txt


def ints(s):
    return [int(x) for x in s.split(",")]


def check_ok(f, head):
    assert int(f["rc"]) == head["OK"] and f["msg"] == "", f


def test_constants_are_the_ones_the_cases_are_built_from(plans):
    _, head, _, _ = plans
    assert (head["T"], head["DIMS"], head["COPY"], head["AXPBY"], head["SUM"]) == (T, ref.K["COPY_MAX_DIMS"], CB, AB, SB)
    assert head["DIMS"] == 5 and head["OK"] == 0 and head["ARG"] == -2 and head["UNSUPPORTED"] == -3


def test_every_refusal_has_its_status_and_message(plans):
    res, head, _, _ = plans
    n = 0
    for kind, table in (("copy", ref.copy_refusals()), ("sum", ref.sum_refusals()), ("axpby", ref.axpby_refusals())):
        for r in table:
            f = res["%s-refusal-%s" % (kind, r.id)]
            assert int(f["rc"]) == head[STATUS[r.status]], (kind, r.id, f)
            assert int(f["blocks"]) == 0, (kind, r.id, "a refused or empty call must not launch")
            if r.status == "ok":
                assert f["msg"] == "", (kind, r.id)
            else:
                assert r.fragment and r.fragment in f["msg"] and f["msg"].startswith("ttsk_"), (kind, r.id, f["msg"])
            n += 1
    statuses = {(k, r.status) for k, t in (("copy", ref.copy_refusals()), ("sum", ref.sum_refusals()), ("axpby", ref.axpby_refusals())) for r in t}
    assert statuses >= {("copy", "arg"), ("copy", "unsupported"), ("copy", "ok"), ("sum", "arg"), ("sum", "ok"), ("axpby", "arg"), ("axpby", "ok")}
    assert n >= 25


def test_copy_pads_ndim_below_five_in_front(plans):
    res, head, _, _ = plans
    for nd in range(6):
        f = res["copy-pad-%d" % nd]
        check_ok(f, head)
        shape, ds, ss = (3, 4, 5, 6, 7)[:nd], (11, 12, 13, 14, 15)[:nd], (21, 22, 23, 24, 25)[:nd]
        assert ints(f["shape"]) == [1] * (5 - nd) + list(shape)
        assert ints(f["ds"]) == [0] * (5 - nd) + list(ds) and ints(f["ss"]) == [0] * (5 - nd) + list(ss)
        assert int(f["total"]) == ref.prod(shape) and int(f["blocks"]) == min(-(-ref.prod(shape) // T), CB)


def test_copy_grid_on_either_side_of_the_cap(plans):
    res, head, _, _ = plans
    want = dict(zip(COPY_TOTALS, (1, 1, 2, CB, CB)))
    for t in COPY_TOTALS:
        for name in ("copy-total-%d", "copy-total2-%d"):
            f = res[name % t]
            check_ok(f, head)
            assert (int(f["total"]), int(f["blocks"])) == (t, want[t]), (t, f)
    f = res["copy-largest"]
    check_ok(f, head)
    assert int(f["total"]) == (1 << 63) - 1 - T * CB and int(f["blocks"]) == CB
    assert int(f["total"]) - 1 + CB * T < 1 << 63                   # the largest index the loop's last test forms
    f = res["copy-largest+"]
    assert int(f["rc"]) == head["UNSUPPORTED"] and int(f["blocks"]) == 0


def test_sum_slices_route_with_each_condition_broken_alone(plans):
    res, head, _, _ = plans
    for name, (n, stride, doff, soff, vector) in SUM_ROUTES.items():
        for acc in (0, 1):
            f = res["sum-route-%s-%d" % (name, acc)]
            check_ok(f, head)
            assert int(f["vector"]) == vector, (name, f)
            unit = 2 if vector else 1
            assert (int(f["n"]), int(f["stride"])) == (n // unit, stride // unit), (name, f)
            assert int(f["blocks"]) == min(-(-(n // unit) // T), SB)
    assert sum(v[4] for v in SUM_ROUTES.values()) >= 3 and sum(1 - v[4] for v in SUM_ROUTES.values()) >= 5


def test_sum_slices_grid_at_both_caps(plans):
    res, head, _, _ = plans
    for n, (vector, blocks) in SUM_BLOCKS.items():
        f = res["sum-blocks-%d" % n]
        check_ok(f, head)
        assert (int(f["vector"]), int(f["blocks"])) == (vector, blocks), (n, f)
        assert int(f["n"]) == (n // 2 if vector else n)


def test_axpby_grid(plans):
    res, head, _, _ = plans
    for n, blocks in AXPBY_BLOCKS.items():
        f = res["axpby-blocks-%d" % n]
        check_ok(f, head)
        assert int(f["blocks"]) == blocks, (n, f)


# ------------------------------------------------------------------------------------- (c) the tables of the GPU module
def test_gpu_copy_cases_are_accepted_and_cover_what_they_name(plans):
    res, head, _, _ = plans
    cases = ref.copy_cases()
    assert len({c.id for c in cases}) == len(cases)
    for c in cases:
        f = res["copy-case-" + c.id]
        check_ok(f, head)
        nd = len(c.shape)
        assert ints(f["shape"]) == [1] * (5 - nd) + list(c.shape) and int(f["total"]) == ref.prod(c.shape)
        # the destination addresses each element once (unit extents apart, whose strides count for nothing)
        idx = ref.strided(ref.np.arange(ref.extent(c.shape, c.ds) + 1), 0, c.shape, c.ds).reshape(-1)
        assert ref.np.unique(idx).size == idx.size == ref.prod(c.shape), c.id
    perms = [c for c in cases if c.id.startswith("perm-")]
    assert len(perms) == 120 and len({c.ss for c in perms}) == 120 and all(ref.prod(c.shape) == 2310 for c in perms)
    assert {len(c.shape) for c in cases} == set(range(6))
    by = {c.id: c for c in cases}
    assert [ref.copy_trips(by[k]) for k in ("cap", "cap+", "cap-third-trip")] == [1, 2, 3]
    assert ref.prod(by["cap"].shape) == T * CB and T * CB < ref.prod(by["cap+"].shape) < 2 * T * CB
    assert 2 * T * CB + T - 1 < ref.prod(by["cap-third-trip"].shape) < 3 * T * CB
    for k in ("dst-gaps", "dst-gaps-perm"):                       # a gap behind every run: each stride passes the extent of what lies inside it
        c = by[k]
        assert all(c.ds[i] > ref.extent(c.shape[i + 1:], c.ds[i + 1:]) for i in range(5)), k
    assert by["dst-gaps"].ds[-1] == 2 and 0 in by["broadcast"].ss and by["odd-offsets"].soff % 2 == 1 and by["odd-offsets"].doff % 2 == 1
    assert {ref.prod(by[k].shape) for k in by if k.startswith("total")} == {T - 1, T, T + 1}
    assert max(8 * (ref.extent(c.shape, c.ss) + ref.extent(c.shape, c.ds)) for c in cases) < 40 << 20


def test_gpu_sum_cases_take_the_route_they_name(plans):
    res, head, _, _ = plans
    cases = ref.sum_cases() + ref.sum_cap_cases()
    assert len({c.id for c in cases}) == len(cases)
    for c in cases:
        f = res["sum-case-" + c.id]
        check_ok(f, head)
        holds = ref.sum_vector_route(c)
        assert int(f["vector"]) == int(all(holds)) == int(c.id.startswith("v-")), (c.id, holds, f)
        assert c.stride >= c.n or c.n == 1
    broken = {k: ref.sum_vector_route(next(c for c in cases if c.id == k)) for k in ("s-odd-n", "s-odd-stride", "s-dst-off8", "s-src-off8")}
    assert [v.index(False) for v in broken.values()] == [0, 1, 2, 3] and all(sum(v) == 3 for v in broken.values())
    for route in "vs":
        small = [c for c in ref.sum_cases() if c.id.startswith(route + "-nb")]
        assert {(c.nb, c.acc) for c in small} == {(nb, acc) for nb in ref.NBS for acc in (0, 1)}
        caps = [c for c in ref.sum_cap_cases() if c.id.startswith(route)]
        assert sorted(ref.sum_trips(c) for c in caps) == [1, 1, 2, 2] and {c.nb for c in caps} == {1, 9} and {c.acc for c in caps} == {0, 1}
        assert all(int(res["sum-case-" + c.id]["blocks"]) == SB for c in caps)
    assert {c.n for c in cases if c.id.startswith("v-n")} == {2, 2 * T - 2, 2 * T, 2 * T + 2}
    assert max(8 * ((c.nb - 1) * c.stride + 2 * c.n) for c in cases) < 340 << 20


def test_gpu_sum_cases_tell_ascending_from_descending():
    """every small case with nb >= 3: the reference itself asserts that the descending sum has other bits (the cap cases do
    the same when the GPU module builds their reference)"""
    n = 0
    for c in ref.sum_cases():
        _, _, slices, prior = ref.sum_operands(c, ref.sum_seed(c))
        want = ref.sum_reference(c, slices, prior)
        if c.n >= 4:                        # the column of -0.0: +0.0 from a fresh accumulator, -0.0 kept on a -0.0
            assert ref.np.signbit(want[-1]) == bool(c.acc) and want[-1] == 0
        n += c.nb >= 3
    assert n >= 40


def test_gpu_axpby_cases(plans):
    res, head, _, _ = plans
    cases = ref.axpby_cases()
    for c in cases:
        f = res["axpby-case-" + c.id]
        check_ok(f, head)
        assert c.exact or c.n <= 4096
    assert {(c.a, c.b) for c in cases} >= {(1.0, 1.0), (1.0, -1.0), (1.75, -0.5), (ref.PI, ref.E), (0.0, 1.0)}
    assert [ref.axpby_trips(c) for c in cases if c.exact] == [1, 2, 3]
    zero_b = [c for c in cases if c.b == 0 and c.yfill is not None]
    assert {(str(c.b), str(c.yfill)) for c in zero_b} == {(b, y) for b in ("0.0", "-0.0") for y in ("nan", "inf", "-inf")}
    # the three candidates differ on the general coefficients: a test that accepted only one of them would be a guess
    c = next(c for c in cases if c.id == "ab-3")
    x, y = ref.axpby_operands(c, 1)
    cand = ref.axpby_candidates(c.a, c.b, x, y)
    assert (cand[0] != cand[1]).any() and (cand[0] != cand[2]).any() and (cand[1] != cand[2]).any()
    ref.axpby_check(c, cand[1], x, y)
    wrong = cand[0].copy()
    wrong[17] = ref.np.nextafter(cand.max(axis=0)[17], ref.np.inf)
    with pytest.raises(AssertionError):
        ref.axpby_check(c, wrong, x, y)


def test_driver_under_sanitizers_prints_the_same(plans, tmp_path_factory):
    """the same driver as a stand-alone program with AddressSanitizer and UBSan: no report, the same output"""
    _, _, stdout, txt = plans
    exe = compile_driver(tmp_path_factory, "vector_plan_san", DRIVER,
                         extra=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"))
    out, err = run_driver(exe, [txt], with_stderr=True)
    assert out == stdout and "runtime error" not in err and "Sanitizer" not in err, err[-2000:]
