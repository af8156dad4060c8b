"""What tests/test_gpu_chain_edges.py runs on the device, checked on the host first (no GPU).

(a) Its case table (tests/chain_step_ref.py) goes through chain_fused_plan / chain_wide_plan / chain_sum_plan at 256
    compute units -- the driver, `call` conventions and parser of tests/test_chain_plan.py, unchanged.  Every accepted
    case carries tags, the plan fields it is meant to reach; each must equal what the plan decides, in both layouts, with
    and without T, and the plan must hold the invariants test_chain_plan.py states.  The union of the tags must cover the
    branch list; every case meant to be refused must be refused with force = 1.
(b) The checker itself: from the truth of three small cases, "kernel results" with one defect each.  The integer and the
    Gaussian check must reject every one and accept the float64 einsum result."""
import numpy as np
import pytest

from tests import chain_step_ref as ref
from tests.host_driver import compile_driver, run_driver
from tests.test_chain_plan import CALL_KEYS, DRIVER, check_fused, check_sum, check_wide, parse

N_CU = 256
BUDGET = 5e8                       # multiply-adds of the two products of a case: about 3 s of long-double arithmetic on one core
# the one levelled candidate at TT rank 100 with seven row tiles: a levelled deal needs nb n >= 512 slices on 256 compute
# units, so no smaller shape asks the plan this question; its tensors are spread over threads like every case's
OVER_BUDGET = {"f-lv-K100"}


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "chain_edges", DRIVER)
    cases = exe.parent / "cases.txt"
    lines = []
    for c in ref.all_cases() + ref.refusals():
        for layout in ref.layouts(c):
            for wt in ref.T_MODES[c.kind][1:]:
                lines.append("%s|%s|%d %s\n" % (c.id, layout, wt, " ".join(str(x) for x in ref.plan_call(c, layout, wt))))
    cases.write_text("".join(lines))
    return parse(run_driver(exe, [N_CU, cases]))


def records(res, c):
    """(layout, wt, T, plan record with force = 1) of every way the GPU test calls the case"""
    for layout in ref.layouts(c):
        for wt in ref.T_MODES[c.kind][1:]:
            for T in (0, 1):
                yield layout, wt, T, dict(res[("%s|%s|%d" % (c.id, layout, wt), N_CU, T, 1, c.kind)])


def test_tags_equal_the_plans(plans):
    res, head = plans
    assert tuple(int(x) for x in head["cw"]) == ref.CW
    check = {"fused": check_fused, "wide": check_wide, "sum": check_sum}
    n = 0
    for c in ref.all_cases():
        for layout, wt, T, f in records(res, c):
            where = (c.id, layout, wt, T)
            assert int(f.pop("rc")) == 1, where
            assert ref.tags_of_plan(c.kind, f) == ref.TAGS[c.id], (where, ref.tags_of_plan(c.kind, f))
            assert int(f["wt"]) == T, where
            try:
                check[c.kind](f, dict(zip(CALL_KEYS, ref.plan_call(c, layout, wt))), T, N_CU, head)
            except AssertionError as e:
                raise AssertionError((where, f)) from e
            n += 1
    print("plans compared with their tags:", n)


def test_table_covers_every_branch():
    cases = ref.all_cases()
    ids = [c.id for c in cases + ref.refusals()]
    assert len(set(ids)) == len(ids) and set(ref.TAGS) == {c.id for c in cases}
    seen = {kind: {k: set() for k in ref.BRANCHES[kind]} for kind in ref.BRANCHES}
    for c in cases:
        for kv in ref.TAGS[c.id].split():
            k, v = kv.split("=")
            seen[c.kind][k].add(v)
    missing = {(kind, k): sorted(set(want.split()) - seen[kind][k]) for kind, b in ref.BRANCHES.items() for k, want in b.items()}
    missing = {k: v for k, v in missing.items() if v}
    assert not missing, "plan branches no case reaches: %s" % missing
    # both layouts, every option, the packed core on every tile structure of the fused kernel and on every levelled deal
    for kind in ref.BRANCHES:
        mine = [c for c in cases if c.kind == kind]
        assert any("layout" not in c.opts for c in mine)
        for name, o in ref.OPTIONS[:5 if kind == "wide" else 4]:
            assert any(all(c.opts.get(k) == v for k, v in o.items()) for c in mine), (kind, name)
    tag = lambda c: dict(kv.split("=") for kv in ref.TAGS[c.id].split())
    packed = [tag(c) for c in cases if c.opts.get("pack")]
    fused = [tag(c) for c in cases if c.kind == "fused"]
    assert {(t["nf"], t["str"]) for t in packed} == {(t["nf"], t["str"]) for t in fused}
    assert {t["piece"] for t in packed} >= {t["piece"] for t in fused}
    over = {c.id for c in cases if ref.macs(c) > BUDGET}
    assert over == OVER_BUDGET, over


def test_cases_beyond_the_cover_are_refused_by_the_plan(plans):
    res, _ = plans
    for c in ref.refusals():
        assert c.opts.get("refuse")
        for layout, wt, T, f in records(res, c):
            assert int(f["rc"]) == 0, (c.id, layout, wt, T)


# ---------------------------------------------------------------------------------------------------- the checker
SMALL = ("f-J17", "w-c2-xgap", "s-J19-K17")


def _case(id):
    return next(c for c in ref.all_cases() if c.id == id)


def _views(c, layout, wt, out, tb):
    O = [o[ref.PRE:ref.PRE + c.J * c.A2].reshape(c.J, c.A2) for o in out]
    return O, ref.t_views(c, layout, wt, tb)


def defects(c, layout, wt, vals):
    """(name, Out buffers, T buffers): the float64 result with one defect each"""
    W, X, E = vals
    b = c.nb - 1
    t64 = np.einsum("ca,jkc->akj", W[b], X[b])

    def fresh():
        out, tb = ref.float64_result(c, layout, wt, vals)
        return out, tb, _views(c, layout, wt, out, tb)

    out, tb, (O, T) = fresh()
    a, k, j = c.A - 1, c.n - 1, c.J - 1
    cc = int(np.argmax(np.abs(W[b][:, a] * X[b][j, k, :])))
    assert W[b][cc, a] * X[b][j, k, cc] != 0
    T[b][a, k, j] -= W[b][cc, a] * X[b][j, k, cc]
    yield "one c term dropped from one element of T", out, tb

    out, tb, (O, T) = fresh()
    j, col = c.J - 1, c.A2 - 1
    terms = t64[:, :, j] * E[:, :, col]
    a, k = np.unravel_index(int(np.argmax(np.abs(terms))), terms.shape)
    assert terms[a, k] != 0
    O[b][j, col] -= terms[a, k]
    yield "one (a, k) term dropped from one element of Out", out, tb

    out, tb, (O, T) = fresh()
    O[b][c.J - 1, c.A2 - 1] = np.uint64(ref.SENT).view(np.float64)
    yield "one element of Out left at the sentinel", out, tb

    out, tb, (O, T) = fresh()
    O[b][15, :] = O[b][14, :]
    yield "a row tile's last row taken from the row above", out, tb

    out, tb, (O, T) = fresh()
    out[b][ref.PRE - 1] = 0.0
    yield "a store in front of Out", out, tb
    out, tb, (O, T) = fresh()
    tb[-1][-ref.POST] = O[b][0, 0]
    yield "a store behind T", out, tb
    if c.kind == "sum" and wt == 3:
        out, tb, (O, T) = fresh()
        tb[0][ref.PRE + c.J] = 1.0
        yield "a store into the row padding of T", out, tb

    out, tb, (O, T) = fresh()
    for bb in range(c.nb):
        O[bb][...] += np.einsum("aj,ab->jb", np.einsum("ca,jc->aj", W[bb], X[bb][:, c.n - 1, :]), E[:, c.n - 1, :])
    yield "the last slice counted twice", out, tb


@pytest.mark.parametrize("id", SMALL)
@pytest.mark.parametrize("integer", (True, False), ids=("integer", "gaussian"))
def test_checker_rejects_one_wrong_piece_and_accepts_float64(id, integer):
    c = _case(id)
    assert c.J >= 16
    vals = ref.values(c, integer, 7)
    tr = ref.truth(c, vals, integer)
    rejected = 0
    for layout in ref.layouts(c):
        for wt in ref.T_MODES[c.kind]:
            out, tb = ref.float64_result(c, layout, wt, vals)
            ref.check_results(c, layout, wt, out, tb, tr, integer)
            if not wt:
                continue
            for name, out, tb in defects(c, layout, wt, vals):
                with pytest.raises(AssertionError):
                    ref.check_results(c, layout, wt, out, tb, tr, integer, what=name)
                rejected += 1
    assert rejected >= 7 * len(ref.layouts(c))


def test_checker_sees_an_unwritten_refused_call():
    c = ref.refusals()[0]
    out, tb = ref.sentinels(c, "right", 1)
    ref.check_untouched(c, out, tb, c.id)
    tb[0][3] = 0.0
    with pytest.raises(AssertionError):
        ref.check_untouched(c, out, tb, c.id)
