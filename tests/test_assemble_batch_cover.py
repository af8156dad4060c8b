"""What tests/test_gpu_assemble_batch_edges.py runs on the device, checked on the host first (no GPU).

(a) Its case table (tests/assemble_batch_ref.py) goes through csrc/assemble_batch_plan.h (plain C++): a short driver
    compiled with the host compiler prints, for every case and every Omega shape of it, the cover verdict, the staging
    layout, the groups and every launch of the Gram and the apply stage.  Each case's tags must equal what the plan
    decides, the tags must cover the branch list, the plan must hold the invariants the kernels rely on, the poison shape
    must dominate every case, and the two refusal messages are as the driver states them.
(b) The checker itself: from the truth of three small cases, "kernel results" with one seeded defect each.  The integer
    and the Gaussian check must reject every one and accept the float64 restatement of the kernel."""

import numpy as np
import pytest

from tests import assemble_batch_ref as ref
from tests.host_driver import compile_driver, run_driver

LDS_MAX = 160 * 1024

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "assemble_batch_plan.h"
using namespace ttsk;

static void launch_line(const char *stage, const AbLaunchPlan &t)
{
    printf("%s g0=%d ng=%d base=%d wgs=%d first=", stage, t.g0, t.ng, t.base, t.wgs);
    for (int i = 0; i < t.ng; ++i) printf("%s%d", i ? "," : "", t.first[i]);
    printf(" chunks=");
    for (int i = 0; i < t.ng; ++i) printf("%s%d", i ? "," : "", t.chunks[i]);
    printf("\n");
}

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    char msg[200], word[32], id[128];
    printf("const AB_TM=%d AB_THREADS=%d AB_MAXG=%d AB_TILES_PER_WG=%d AB_COVER_MIN=%d AB_COVER_MAX=%d AB_LDS_MAX=%zu\n", AB_TM, AB_THREADS, AB_MAXG,
           AB_TILES_PER_WG, AB_COVER_MIN, AB_COVER_MAX, AB_LDS_MAX);
    ab_msg_jacobi(msg, sizeof(msg), 57, 112);
    printf("msg jacobi %s\n", msg);
    ab_msg_lds(msg, sizeof(msg));
    printf("msg lds %s\n", msg);
    // the whole cover, both directions: the largest LDS of the fused apply, and how many shapes it refuses
    size_t worst = 0;
    int refused = 0, off = 0;
    for (int l = 1; l <= 130; ++l)
        for (int r = 1; r <= 130; ++r)
            for (int dir = 0; dir < 2; ++dir) {
                AbShapePlan p;
                ab_shape_plan(l, r, dir, 1, true, &p);
                if (!p.covered) continue;
                worst = p.apply_lds > worst ? p.apply_lds : worst;
                refused += !p.apply_lds_ok;
                ab_shape_plan(l, r, dir, 1, false, &p);
                off += p.covered;
            }
    printf("sweep worst_apply_lds=%zu refused=%d covered_without_fast_pinv=%d\n", worst, refused, off);
    int direction, nshapes;
    while (fscanf(f, "%31s %127s %d %d", word, id, &direction, &nshapes) == 4) {
        printf("case %s\n", id);
        for (int s = 0; s < nshapes; ++s) {
            long long l, r;
            int T;
            if (fscanf(f, "%31s %lld %lld %d", word, &l, &r, &T) != 4) return 3;
            std::vector<AbPairOff> pairs(T);
            for (int i = 0; i < T; ++i) {
                long long k, m, a, b, c, d;
                if (fscanf(f, "%lld %lld %lld %lld %lld %lld", &k, &m, &a, &b, &c, &d) != 6) return 3;
                pairs[i] = AbPairOff{a, b, c, d, m, (int)k};
            }
            AbShapePlan p;
            ab_shape_plan(l, r, direction, T, true, &p);
            printf("shape l=%lld r=%lld covered=%d T=%d n=%d K=%d lr=%zu nn=%zu szO=%zu szG=%zu off_Os=%zu off_Ps=%zu off_Gm=%zu off_Rinv=%zu off_Ginv=%zu"
                   " off_status=%zu bytes=%zu gram_lds=%zu solve_lds=%zu a=%d b=%d apply_lds=%zu apply_lds_ok=%d\n",
                   l, r, (int)p.covered, p.T, p.n, p.K, p.lr, p.nn, p.szO, p.szG, p.off_Os, p.off_Ps, p.off_Gm, p.off_Rinv, p.off_Ginv, p.off_status,
                   p.bytes, p.gram_lds, p.solve_lds, p.a, p.b, p.apply_lds, (int)p.apply_lds_ok);
            if (!p.covered) continue;
            const std::vector<AbGroupPlan> groups = ab_make_groups(pairs);
            for (const AbGroupPlan &g : groups)
                printf("group first=%d count=%d s_psi=%lld s_om=%lld s_c=%lld s_work=%lld m=%lld\n", g.first, g.count, (long long)g.s_psi,
                       (long long)g.s_om, (long long)g.s_c, (long long)g.s_work, (long long)g.m);
            printf("launches n=%d\n", ab_launches(groups.size()));
            AbLaunchPlan t;
            for (size_t g0 = 0; g0 < groups.size(); g0 += AB_MAXG) { ab_gram_launch(groups, g0, &t); launch_line("gram", t); }
            for (size_t g0 = 0; g0 < groups.size(); g0 += AB_MAXG) { ab_apply_launch(groups, g0, &t); launch_line("apply", t); }
        }
    }
    return 0;
}
"""


def _kv(words, lists=()):
    out = {}
    for w in words:
        k, v = w.split("=")
        out[k] = [int(x) for x in v.split(",")] if k in lists else int(v)
    return out


def parse(text):
    """-> (header: {const, msg jacobi, msg lds, sweep}, {case id: [shape dict with groups / gram / apply lists]})"""
    head, res, cur = {}, {}, None
    for line in text.splitlines():
        w = line.split()
        if w[0] == "const" or w[0] == "sweep":
            head[w[0]] = _kv(w[1:])
        elif w[0] == "msg":
            head["msg " + w[1]] = line.split(" ", 2)[2]
        elif w[0] == "case":
            cur = res.setdefault(w[1], [])
        elif w[0] == "shape":
            cur.append(dict(_kv(w[1:]), groups=[], gram=[], apply=[]))
        elif w[0] == "group":
            cur[-1]["groups"].append(_kv(w[1:]))
        elif w[0] == "launches":
            cur[-1]["launches"] = _kv(w[1:])["n"]
        else:
            cur[-1][w[0]].append(_kv(w[1:], lists=("first", "chunks")))
    return head, res


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "assemble_batch_plan", DRIVER)
    cases = exe.parent / "cases.txt"
    cases.write_text("".join(ref.plan_input(c) for c in ref.cases() + [ref.POISON]))
    return parse(run_driver(exe, [cases]))


def check_shape(c, s):
    """what assemble_gram_kernel, the Cholesky / solve / Jacobi stages and assemble_apply_kernel rely on"""
    l, r, T = s["l"], s["r"], s["T"]
    assert s["covered"] == int(ref.covered(l, r))
    if not s["covered"]:
        return
    blk = lambda v: (v + 31) // 32 * 32
    assert (s["n"], s["K"], s["lr"], s["nn"]) == (min(l, r), max(l, r), l * r, min(l, r) ** 2)
    assert (s["a"], s["b"]) == ((r, l) if c.direction == 0 else (l, r))
    # staging: the regions hold what the stages write and follow one another without overlap
    assert s["szO"] == blk(T * l * r) and s["szG"] == blk(T * s["nn"])
    regions = [("Os", s["szO"], T * l * r), ("Ps", s["szO"], T * l * r), ("Gm", s["szG"], T * s["nn"]), ("Rinv", s["szG"], T * s["nn"]),
               ("Ginv", s["szG"], T * s["nn"]), ("status", blk(T), (T + 1) // 2)]
    end = 0
    for name, size, used in regions:
        assert s["off_" + name] == end and used <= size, (name, s)
        end += size
    assert s["bytes"] == 8 * end
    # LDS of the three kernels
    u4, u16 = lambda x: (x + 3) // 4 * 4, lambda x: (x + 15) // 16 * 16
    a, b = s["a"], s["b"]
    assert s["gram_lds"] == 8 * s["K"] * s["n"] <= LDS_MAX and s["solve_lds"] == 8 * (s["K"] * s["n"] + s["nn"]) <= LDS_MAX
    assert s["apply_lds"] == 8 * (u4(a) * u16(b) + u4(b) * u16(a) + ref.TM * (u16(a) + 2) + ref.TM * (u16(b) + 2)) <= LDS_MAX
    assert s["apply_lds_ok"] == 1
    # the prefetch registers hold a whole tile: 14 slots of 256 threads
    assert ref.TM * u16(a) <= 14 * 256
    # groups: a partition of the pairs in order, each inside one mode with one m
    G = s["groups"]
    assert G[0]["first"] == 0 and all(G[i + 1]["first"] == G[i]["first"] + G[i]["count"] for i in range(len(G) - 1))
    assert G[-1]["first"] + G[-1]["count"] == T and all(g["count"] >= 1 for g in G)
    assert s["launches"] == -(-len(G) // ref.MAXG) == len(s["gram"]) == len(s["apply"])
    for i, (lg, la) in enumerate(zip(s["gram"], s["apply"])):
        mine = G[i * ref.MAXG:(i + 1) * ref.MAXG]
        assert lg["g0"] == la["g0"] == i * ref.MAXG and lg["ng"] == la["ng"] == len(mine) <= ref.MAXG
        # Gram: workgroup = pair, rebased to the launch's first pair; find_group needs `first` increasing from 0
        assert lg["base"] == mine[0]["first"] and lg["first"] == [g["first"] - lg["base"] for g in mine]
        assert lg["wgs"] == sum(g["count"] for g in mine) and lg["chunks"] == [1] * len(mine)
        assert lg["first"][0] == 0 and all(x < y for x, y in zip(lg["first"], lg["first"][1:]))
        # apply: `chunks` workgroups per tensor, no chunk without a tile
        at = 0
        for g, first, ch in zip(mine, la["first"], la["chunks"]):
            ntiles = -(-g["m"] // ref.TM)
            assert ch == max(1, -(-ntiles // ref.TILES_PER_WG)) <= ntiles and first == at
            at += g["count"] * ch
        assert la["wgs"] == at and all(x < y for x, y in zip(la["first"], la["first"][1:]))


def expected_groups(c, l, r):
    """the groups the layout is built to give: runs of tensors with equal slot steps in every kind, per mode of this shape"""
    out = []
    for k in range(c.d - 1):
        if (c.lr[k], c.rr[k]) != (l, r):
            continue
        step = lambda b: tuple(ref.slots_of(c, kind)[b] - ref.slots_of(c, kind)[b - 1] for kind in ref.KINDS)
        b = 0
        while b < c.count:
            e = b + 1
            if e < c.count:
                st = step(e)
                while e < c.count and step(e) == st:
                    e += 1
            out.append(e - b)
            b = e
    return out


def test_tags_equal_the_plan(plans):
    head, res = plans
    assert head["const"] == dict(AB_TM=ref.TM, AB_THREADS=256, AB_MAXG=ref.MAXG, AB_TILES_PER_WG=ref.TILES_PER_WG, AB_COVER_MIN=ref.COVER_MIN,
                                 AB_COVER_MAX=ref.COVER_MAX, AB_LDS_MAX=LDS_MAX)
    seen = {}
    for c in ref.cases():
        shapes = res[c.id]
        assert [(s["l"], s["r"]) for s in shapes] == sorted({(c.lr[k], c.rr[k]) for k in range(c.d - 1)})
        tags = ref.tags_of_plan(c, shapes)
        assert tags == ref.TAGS[c.id], (c.id, tags)
        for s in shapes:
            try:
                check_shape(c, s)
            except AssertionError as e:
                raise AssertionError((c.id, s)) from e
            if s["covered"]:
                assert [g["count"] for g in s["groups"]] == expected_groups(c, s["l"], s["r"]), c.id
        for part in tags.split(" | "):
            for kv in part.split():
                k, v = kv.split("=")
                seen.setdefault(k, set()).add(v)
    print("plans compared with their tags:", len(ref.cases()))
    for k, v in sorted(seen.items()):
        print("  %s: %s" % (k, " ".join(sorted(v))))


def test_table_covers_every_branch_and_every_case_of_the_issue():
    cs = ref.cases()
    ids = [c.id for c in cs]
    assert len(set(ids)) == len(ids) and set(ref.TAGS) == set(ids)
    seen = {k: set() for k in ref.BRANCHES}
    for c in cs:
        for part in ref.TAGS[c.id].split(" | "):
            for k, v in (kv.split("=") for kv in part.split()):
                if k in seen:
                    seen[k] |= set(v.replace("0+", "0 +").replace("+", " ").split()) if k in ("chunks", "last") else (
                        set(v) if k == "strides" else {v})
    missing = {k: sorted(set(want.split()) - seen[k]) for k, want in ref.BRANCHES.items()}
    missing = {k: v for k, v in missing.items() if v}
    assert not missing, "plan branches no case reaches: %s" % missing
    tag = lambda c: dict(kv.split("=") for kv in ref.TAGS[c.id].split(" | ")[-1].split())
    for direction in (0, 1):
        mine = [c for c in cs if c.direction == direction]
        d2 = [c for c in mine if c.d == 2]
        assert {(c.lr[0], c.rr[0]) for c in d2} >= set(ref.PAD_SHAPES) | set(ref.OUTSIDE)
        assert {int(tag(c)[k]) for c in mine if "nbc" in tag(c) for k in ("nbc", "nba")} >= {1, 2, 7}
        rows = {(c.n[direction], c.lr[0], c.rr[0]) for c in d2}
        assert {m for m, _, _ in rows} >= {1, 31, 32, 33, 511, 512, 513, 1025}
        for m in (513, 1025):                                    # the chunked sizes, narrow and wide
            assert {(l, r) for mm, l, r in rows if mm == m} >= {(3, 5), (56, 112)}
        assert any(c.d == 18 and c.count == 2 and len(set(c.lr + c.rr)) == 1 for c in mine)
        assert any(c.d == 4 and len({m for _, _, _, m in ref.pair_list(c)}) == 3 for c in mine)
        assert any(c.count == 33 for c in mine) and any(c.count == 1 for c in mine)
        assert any(c.opts.get("robust") and c.count == 4 for c in mine)
        assert sum(1 for c in mine if c.opts.get("refine") and c.count == 3) == 2
        assert any(len({(c.lr[k], c.rr[k]) for k in range(c.d - 1)}) == 2 and "fallback" in ref.TAGS[c.id] and "covered" in ref.TAGS[c.id] for c in mine)
    # sizes: nothing beyond 1100 rows or d = 18
    assert all(c.d <= 18 and max(m for _, _, _, m in ref.pair_list(c)) <= 1100 for c in cs)


def test_a_later_shape_needs_more_staging(plans):
    for D in "RL":
        first, second = plans[1]["s-two-covered-" + D]
        assert first["covered"] and second["covered"] and second["bytes"] > first["bytes"]


def test_poison_dominates_every_case_and_writes_every_region_in_full(plans):
    (p,) = plans[1][ref.POISON.id]
    assert p["covered"] and p["szO"] == p["T"] * p["lr"] and p["szG"] == p["T"] * p["nn"]       # no padding: no word left unwritten
    for c in ref.cases():
        for s in plans[1][c.id]:
            if s["covered"]:
                assert s["T"] <= p["T"] and s["szO"] <= p["szO"] and s["szG"] <= p["szG"] and s["bytes"] <= p["bytes"], c.id


def test_refusal_messages_and_the_cover_rule(plans):
    head = plans[0]
    assert head["msg jacobi"] == "ttsk_tt_assemble_batch: Jacobi kernel outside its LDS cover (57 x 112)"
    assert head["msg lds"] == "ttsk_tt_assemble_batch: LDS of the fused apply"
    # inside the cover the fused apply always fits its LDS (the widest shape takes 153600 bytes); without the fast
    # pseudo-inverse nothing is covered
    assert head["sweep"] == dict(worst_apply_lds=153600, refused=0, covered_without_fast_pinv=0)


# ---------------------------------------------------------------------------------------------------- the checker
SMALL = ("pad-3x5-R", "g-three-m-L", "refine-13x29-R")


def defects(c, v, mode):
    """(name, output arenas): the float64 restatement with one defect each"""
    fresh = lambda: ref.float64_result(c, v, mode)
    k, b, j, m = ref.pair_list(c)[-1]
    cn, wn = ref.pair_arenas(c, k, j)[2:]
    o, sz = ref.place(c, cn, b)
    shape = ref.out_core_shape(c, j)
    out = fresh()
    Cm = out[cn][o:o + sz].reshape((m, -1) if c.direction == 0 else (-1, m))
    i = (m - 1, Cm.shape[1] - 1) if c.direction == 0 else (Cm.shape[0] - 1, m - 1)       # last row, last column of the normalised C
    Cm[i] += max(abs(Cm[i]), 1.0) * 2.0 ** -30
    yield "a wrong element in a padded column", out
    # the last full tile (or all rows of a short matrix) shifted by one row
    kk, bb, jj, mm = max(ref.pair_list(c), key=lambda p: p[3])
    cn2 = ref.pair_arenas(c, kk, jj)[2]
    o2, sz2 = ref.place(c, cn2, bb)
    out = fresh()
    Cm = out[cn2][o2:o2 + sz2].reshape((mm, -1) if c.direction == 0 else (-1, mm))
    lo = max(0, (mm // 32 - 1) * 32)
    hi = min(mm, lo + 32)
    if c.direction == 0:
        Cm[lo:hi] = np.roll(Cm[lo:hi], 1, axis=0)
    else:
        Cm[:, lo:hi] = np.roll(Cm[:, lo:hi], 1, axis=1)
    yield "a tile's rows shifted", out
    for name in (cn, wn):
        out = fresh()
        (o0, s0), (o1, _) = ref.place(c, name, 0), ref.place(c, name, 1)
        t = out[name][o0:o0 + s0].copy()
        out[name][o0:o0 + s0] = out[name][o1:o1 + s0]
        out[name][o1:o1 + s0] = t
        yield "two tensors of a group swapped in %s" % name, out
    out = fresh()
    ow, sw = ref.place(c, wn, b)
    out[wn][ow:ow + sw] = ref.SENT_F
    yield "P not copied to work", out
    out = fresh()
    out[cn][o - 1] = 0.0
    yield "one guard word in front of C overwritten", out
    out = fresh()
    out[wn][ow + sw] = out[wn][ow]
    yield "one guard word behind work overwritten", out


@pytest.mark.parametrize("id", SMALL)
@pytest.mark.parametrize("integer", (True, False), ids=("integer", "gaussian"))
def test_checker_rejects_one_seeded_defect_and_accepts_float64(id, integer):
    c = ref.by_id(id)
    mode = "integer" if integer else ref.gaussian_mode(c)
    v = ref.values(c, mode, 7)
    worst = ref.check_results(c, v, ref.float64_result(c, v, mode), mode)
    print(id, mode, worst)
    rejected = 0
    for name, out in defects(c, v, mode):
        with pytest.raises(AssertionError):
            ref.check_results(c, v, out, mode, what=name)
        rejected += 1
    assert rejected == 7


@pytest.mark.parametrize("id", [c.id for c in ref.cases() if c.opts.get("refine")])
@pytest.mark.parametrize("seed", (1, 2, 3))
def test_refinement_bar_separates_the_refined_from_the_first_product(id, seed):
    """the bar of the refine cases is a condition on the host: the float64 restatement passes with margin, the same
    without the residual step fails with margin, and the Cholesky gate accepts every Omega of the case"""
    c = ref.by_id(id)
    v = ref.values(c, "refine", seed)
    for name in v:
        if name.startswith("om"):
            assert all(ref.chol_spread(M) > 3 * ref.CHOL_GATE for M in v[name].values())
    worst = ref.check_results(c, v, ref.float64_result(c, v, "refine"), "refine")
    assert worst["refine"] <= ref.REFINE_MARGIN / 4, worst
    bare = ref.float64_result(c, v, "refine", refine=False)
    ratios = [err / e for err, e in (ref.refine_err(Xn, On, Cn) for _, _, Xn, On, _, Cn in ref.pairs_of(c, ref.arenas_in(c, v), bare))]
    assert max(ratios) >= 2 * ref.REFINE_MARGIN, ratios          # the case is its group of 3: one pair beyond the bar rejects it
    with pytest.raises(AssertionError):
        ref.check_results(c, v, bare, "refine")
    print(id, seed, worst)


def test_robust_omegas_are_rejected_by_the_gate_and_their_neighbours_accepted():
    for c in (c for c in ref.cases() if c.opts.get("robust")):
        v = ref.values(c, "robust", 0)
        spread = [ref.chol_spread(v["om0"][s]) for s in range(4)]
        assert spread[1] < ref.CHOL_GATE / 10 and spread[2] < ref.CHOL_GATE / 10 and min(spread[0], spread[3]) > 3 * ref.CHOL_GATE, spread
        ref.check_results(c, v, ref.float64_result(c, v, "robust"), "robust")


def test_checker_sees_a_write_by_a_refused_call():
    c = ref.by_id("pad-3x5-R")
    out = ref.arenas_out(c)
    ref.check_untouched(out, c.id)
    out["work0"][3] = 0.0
    with pytest.raises(AssertionError):
        ref.check_untouched(out, c.id)
