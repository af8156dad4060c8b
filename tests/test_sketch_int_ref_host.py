"""tests/sketch_int_ref.py on the host: every Case is built, so that its two assertions run without a GPU -- every entry of an
integer sketch, times the number of tensors, stays below 2^53, and the int64 einsums equal the oracle's sketch -- and the policy
of csrc/sketch_split.h, compiled into a small driver, splits the one shape that is there for it ("b8").

policy_budgets(n_cu, case, tmp_path_factory) is what the GPU tests ask for the budgets the driver of tt_fused.hip takes for a pipelined call of
`case` on two streams whose interior chain steps are all on chain_step_kernel."""
import pytest

from tests.host_driver import compile_driver, run_driver
from tests.sketch_int_ref import SHAPES, Case

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "sketch_split.h"
using namespace ttsk;

// argv: n_cu nb s l r d n_0 .. n_{d-1}: the policy for a pipelined call on two streams, fused family
int main(int argc, char **argv)
{
    if (argc < 7) return 2;
    const int n_cu = atoi(argv[1]), nb = atoi(argv[2]), s = atoi(argv[3]), l = atoi(argv[4]), r = atoi(argv[5]), d = atoi(argv[6]);
    if (d < 2 || argc != 7 + d) return 2;
    std::vector<int64_t> n(d), ss(d + 1, s), lt(d, l), rt(d, r);
    for (int mu = 0; mu < d; ++mu) n[mu] = atoi(argv[7 + mu]);
    ss[0] = ss[d] = 1; lt[0] = 1; rt[0] = 1;
    const SketchSplit sp = sketch_split_policy(SketchSplitIn{n_cu, nb, d, n.data(), ss.data(), lt.data(), rt.data(), true, true, SKETCH_FUSED});
    printf("%d %d %d\n", sp.right, sp.left, sp.psi);
    return 0;
}
"""

_exe = []


def policy_budgets(n_cu, case, tmp_path_factory):
    """-> (right, left, psi): sketch_split_policy for `case` (a Case) on n_cu compute units, pipelined, two streams, fused family.
    tmp_path_factory: pytest's fixture (the driver is compiled on first use, once per process)"""
    if not _exe:
        _exe.append(compile_driver(tmp_path_factory, "sketch_policy", DRIVER))
    out = run_driver(_exe[0], [n_cu, case.nb, case.s, case.l, case.r, len(case.shape), *case.shape])
    right, left, psi = (int(x) for x in out.split())
    return right, left, psi


@pytest.fixture(scope="module")
def cases():
    return {name: Case(name) for name in sorted(SHAPES)}          # the bound and the oracle equality are asserted in there


def test_every_case_builds_with_both_kinds_of_cores(cases):
    for name, case in cases.items():
        shape, s, l, r, nb = SHAPES[name]
        d = len(shape)
        for kind in ("int", "gauss"):
            ld, rd, tts, want, want_sum = case.data[kind]
            assert len(tts) == len(want) == nb and len(want_sum) == 2 * d - 1, (name, kind)
            assert [c.shape for c in tts[0]] == [(1 if mu == 0 else s, shape[mu], 1 if mu == d - 1 else s) for mu in range(d)], (name, kind)
            assert want[0][d].shape == (l, r) and want[0][1].shape == (l, shape[1], r), (name, kind)


@pytest.mark.parametrize("n_cu", [256, 304])
def test_the_policy_splits_b8(tmp_path_factory, cases, n_cu):
    case = cases["b8"]
    right, left, psi = policy_budgets(n_cu, case, tmp_path_factory)
    print("b8 on %d CUs: right %d, left %d, psi %d" % (n_cu, right, left, psi))
    assert (right, left, psi) != (0, 0, 0)
    # whole workgroups per tensor for each chain, the two chains side by side, one of the n = 4 workgroups of a tensor left free
    assert right > 0 and left > 0 and right % case.nb == 0 and left % case.nb == 0 and right + left <= n_cu
    assert right // case.nb + left // case.nb == min(n_cu // case.nb, min(case.shape[1:-1])) - 1


def test_the_policy_leaves_the_small_batches_whole(tmp_path_factory, cases):
    for name in ("a3", "a5", "b2"):
        assert policy_budgets(256, cases[name], tmp_path_factory) == (0, 0, 0), name
