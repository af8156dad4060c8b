"""The one-call TT sketches (ttsk_tt_sketch_batch, ttsk_tt_sketch_sum) under CU budgets (ttsk_tt_sketch_split,
csrc/sketch_split.h): a budget changes the grid of the chain steps and of the Psi products -- how many slices a workgroup
walks, how many slab partials are summed -- and must change nothing else.

Shapes: the smallest that reach the levelled 12-wave deal (two slices or more per workgroup) and both tile structures:
(a) TT rank 68, l = 36, r = 68 on n = (6, 5, 7, 6) with 3 and 5 tensors, (b) the headline structure -- TT rank 100, l = 50,
r = 100 -- at n = 4 with 2 and 8 tensors (tests/sketch_int_ref.py).  Splits: the policy, full width, nearly everything to the
right chain, nearly everything to the left chain and Psi, and halves.

Cores of small integers: every partial sum of every product is an integer below 2^53 (the largest entry, an Omega_0 of
shape (b), is below 2^42), so fp64 is exact whatever the order and the grid: every Psi and Omega must EQUAL the int64
einsum, under every split.  Gaussian cores: the oracle's general_sketch to the tolerance of tests/test_gpu_parity.py for
the one-call path (1e-12 in the Frobenius norm), and a second run of the same split gives the same bits."""
import pytest

from tests.edge_kit import exact, nat, num_cu, same_bits, tsa  # noqa: F401
from tests.golden_io import rel
from tests.sketch_int_ref import SHAPES, Case, gpu_step, split_of

pytestmark = pytest.mark.gpu

TOL = 1e-12                 # tests/test_gpu_parity.py: test_batched_one_call_path, test_sketch_of_a_sum_in_one_call
SPLITS = ("auto", "full", "right", "left", "halves")

_cases = {}


@pytest.fixture(scope="module")
def cases():
    def get(name):
        if name not in _cases:
            _cases[name] = Case(name)
        return _cases[name]
    yield get
    _cases.clear()


def sketches(nat, case, kind, split, what):
    """-> (the nb sketches of the batch call, the sketch of the sum call), each a list of host arrays Psi + Omega"""
    from tt_sketch_amd.device import DevArray
    plan, X, _ = case.on_device(kind)
    nb, stride = case.nb, plan.size + 5
    out, out_sum = DevArray.zeros((nb * stride,)), DevArray.zeros((plan.size,))
    nat.call("ttsk_tt_sketch_split", *split)
    try:
        with gpu_step(nat, what + " batch"):
            plan.run_batch(X, nb, out, stride)
        with gpu_step(nat, what + " sum"):
            plan.run_sum(X, nb, out_sum)
    finally:
        nat.call("ttsk_tt_sketch_split", -1, -1, -1)
    per = []
    for b in range(nb):
        Psi, Om = plan.views(out[b * stride:b * stride + plan.size])
        per.append([a.get() for a in Psi + Om])
    Psi, Om = plan.views(out_sum)
    return per, [a.get() for a in Psi + Om]


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_integer_cores_equal_the_int64_einsum_under_every_split(tsa, nat, num_cu, cases, shape, split):  # noqa: F811
    case = cases(shape)
    what = "%s %s" % (shape, split)
    per, total = sketches(nat, case, "int", split_of(split, num_cu, case.nb), what)
    _, _, _, want, want_sum = case.data["int"]
    for b, (got, w) in enumerate(zip(per, want)):
        for i, (a, c) in enumerate(zip(got, w)):
            exact(a, c, "%s tensor %d piece %d" % (what, b, i))
    for i, (a, c) in enumerate(zip(total, want_sum)):
        exact(a, c, "%s sum piece %d" % (what, i))


@pytest.mark.parametrize("split", SPLITS)
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_gaussian_cores_match_the_oracle_and_repeat_their_bits(tsa, nat, num_cu, cases, shape, split):  # noqa: F811
    case = cases(shape)
    what = "%s %s" % (shape, split)
    cfg = split_of(split, num_cu, case.nb)
    per, total = sketches(nat, case, "gauss", cfg, what)
    _, _, _, want, want_sum = case.data["gauss"]
    for b, (got, w) in enumerate(zip(per, want)):
        for i, (a, c) in enumerate(zip(got, w)):
            r = rel(a, c)
            print("%s tensor %d piece %d: rel %.3e" % (what, b, i, r))
            assert a.shape == c.shape and r < TOL, (what, b, i, r)
    for i, (a, c) in enumerate(zip(total, want_sum)):
        r = rel(a, c)
        print("%s sum piece %d: rel %.3e" % (what, i, r))
        assert a.shape == c.shape and r < TOL, (what, "sum", i, r)
    per2, total2 = sketches(nat, case, "gauss", cfg, what + " (second run)")
    same_bits(per, per2, what + ": the batch's sketches of two runs")
    same_bits(total, total2, what + ": the sum's sketch of two runs")


def test_the_setting_is_checked_and_restored(nat):  # noqa: F811
    with pytest.raises(ValueError):
        nat.call("ttsk_tt_sketch_split", -2, 0, 0)
    nat.call("ttsk_tt_sketch_split", -1, -1, -1)
