"""Many pairs of operator-times-train products closed in one launch, without a GPU: the host-side plan of
``ttsk_op_close_batch`` (csrc/op_close_batch_plan.h, plain C++) compiled with the host compiler -- every pair planned as the
single call plans it, the table that maps a workgroup to its pair, the slab, every refusal -- and ``operator_gram.op_gram``
on host factors against dense NumPy with the device, ``to_tt`` and the operators' ``__call__`` forbidden."""
import itertools

import numpy as np
import pytest

from tests import hadamard_ref
from tests import op_close_ref as ref
from tests.host_driver import compile_driver, run_driver

ERR_ARG, UNSUPPORTED = -2, -3
ARRAYS = ("Wl", "N", "Y", "dims", "strides", "ldw", "out", "work")      # the bits of `null`
ELEMENTS = ("Wl", "N", "Y", "out")                                     # the arrays of pointers

# ---- 1. the plan
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "op_close_batch_plan.h"
using namespace ttsk;
static long long next() { long long v = 0; if (scanf("%lld", &v) != 1) exit(3); return v; }
int main()
{
    static double cell;
    const int records = (int)next(), npairs = (int)next(), accumulate = (int)next();
    const long long work_doubles = next();
    const int null = (int)next(), null_pair = (int)next(), null_which = (int)next(), enumerate = (int)next();
    std::vector<int64_t> dims(7 * records), strides(7 * records), ldw(records), offsets(records + 1, -1);
    std::vector<const double *> Wl(records, &cell), N(records, &cell), Y(records, &cell);
    std::vector<double *> out(records, &cell);
    for (int t = 0; t < records; ++t) {
        for (int i = 0; i < 7; ++i) dims[7 * t + i] = next();
        for (int i = 0; i < 7; ++i) strides[7 * t + i] = next();
        ldw[t] = next();
    }
    if (null_which == 0) Wl[null_pair] = nullptr;
    if (null_which == 1) N[null_pair] = nullptr;
    if (null_which == 2) Y[null_pair] = nullptr;
    if (null_which == 3) out[null_pair] = nullptr;
    static OpCloseBatchPlan p, q;
    const int rc = op_close_batch_plan(npairs, null & 1 ? nullptr : Wl.data(), null & 2 ? nullptr : N.data(), null & 4 ? nullptr : Y.data(),
                                       null & 8 ? nullptr : dims.data(), null & 16 ? nullptr : strides.data(), null & 32 ? nullptr : ldw.data(),
                                       null & 64 ? nullptr : out.data(), accumulate, null & 128 ? nullptr : &cell, work_doubles, &p);
    printf("rc %d\nmsg %s\n", rc, p.msg);
    printf("const %d %zu %zu\n", OP_CLOSE_MAX_PAIRS, sizeof(OpCloseBatchArgs), sizeof(OpClosePair));
    const int lrc = op_close_batch_layout(npairs, null & 8 ? nullptr : dims.data(), offsets.data(), &q);
    printf("layout %d", lrc);
    for (int t = 0; t <= (npairs > 0 && npairs <= records ? npairs : 0); ++t) printf(" %lld", (long long)offsets[t]);
    printf("\nlayoutmsg %s\n", q.msg);
    if (rc) return 0;
    printf("top %lld %lld %lld %.17g %d %d\n", (long long)p.blocks, (long long)p.sum_blocks, (long long)p.slab, p.flops, p.a.npairs, p.a.accumulate);
    for (int t = 0; t < npairs; ++t) {
        const OpClosePair &T = p.a.t[t];
        OpClosePlan one;
        op_close_layout(dims.data() + 7 * t, &one);
        printf("pair %d %d %d %d %d %d %d %lld %lld %lld %lld %lld %d %d %d\n", T.a.jchunks, T.a.jper, T.a.ptiles, T.a.gtiles, T.a.cblocks, T.block0,
               T.sum0, (long long)(T.a.work - &cell), (long long)T.slice, (long long)T.ldw, (long long)T.a.sNk, (long long)one.slab, one.a.jchunks,
               one.a.jper, (int)one.blocks);
    }
    if (enumerate)
        for (int b = 0; b < (int)p.blocks; ++b) {
            const int t = op_close_pair_of(p.a, b);
            const OpCloseTile w = op_close_tile_of(p.a.t[t].a, b - p.a.t[t].block0);
            printf("blk %d %d %d %d %d\n", t, w.jc, w.pt, w.gt, w.cb);
        }
    for (int b = 0; enumerate && b < (int)p.sum_blocks; ++b) printf("sum %d\n", op_close_sum_pair_of(p.a, b));
    return 0;
}
"""


def _packed_strides(d):
    """element strides over (gamma, j, i, gamma') of a contiguous (S, n_out, n_in, S') array, then those of a contiguous Y"""
    S, S1, s, s1, n_in, n_out, P = d
    return (n_out * n_in * S1, S1, n_in * S1, 1, n_in * s1, s1, 1)


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "op_close_batch_plan", DRIVER)

    def run(dims, strides=None, ldw=None, npairs=None, accumulate=0, work=2 ** 62, null=(), null_element=None, enumerate_=False):
        """dims: a list of (S, S', s, s', n_in, n_out, P); strides: per pair those of N and Y, of packed cores unless given;
        ldw: per pair, P unless given; null: names of ARRAYS passed as NULL; null_element: (pair, name of ELEMENTS)"""
        strides = [_packed_strides(d) for d in dims] if strides is None else strides
        ldw = [d[6] for d in dims] if ldw is None else ldw
        pair, which = (0, -1) if null_element is None else (null_element[0], ELEMENTS.index(null_element[1]))
        words = [len(dims), len(dims) if npairs is None else npairs, accumulate, work, sum(1 << ARRAYS.index(n) for n in null), pair, which,
                 int(enumerate_)]
        for d, s, l in zip(dims, strides, ldw):
            words += list(d) + list(s) + [l]
        out = run_driver(exe, stdin=" ".join(str(w) for w in words)).splitlines()
        p = dict(rc=int(out[0].split()[1]), msg=out[1][4:], pair=[], blk=[], sum=[])
        for line in out[2:]:
            key, *v = line.split()
            if key == "layoutmsg":
                p[key] = line[10:]
                continue
            v = [float(x) if "." in x or "e" in x else int(x) for x in v]
            if key in ("pair", "blk", "sum"):
                p[key].append(v)
            else:
                p[key] = v
        return p
    return run


def _case_strides(case):
    _, N, Y, _ = ref.case_arrays(case)
    return tuple(x // 8 for x in N.strides) + tuple(x // 8 for x in Y.strides)


def test_the_twelve_cases_as_one_batch(plan):
    dims = [ref.dims(c) for c in ref.CASES]
    ldw = [c.P + 3 + k for k, c in enumerate(ref.CASES)]
    p = plan(dims, [_case_strides(c) for c in ref.CASES], ldw, accumulate=1, enumerate_=True)
    assert p["rc"] == 0, p["msg"]
    max_pairs, table_bytes, pair_bytes = p["const"]
    assert len(ref.CASES) <= max_pairs and table_bytes <= 4096 and (max_pairs + 1) * pair_bytes + 8 > 4096      # as many as 4 KB hold
    block0 = sum0 = slab0 = 0
    flops = 0.0
    for k, (case, got) in enumerate(zip(ref.CASES, p["pair"])):
        jchunks, jper, slab, blocks = ref.layout(*dims[k])
        # the pair's cut of j, its tiles and its slab are those of the single call: of op_close_layout and of the restatement
        assert got[:5] == [jchunks, jper, -(-case.P // 16), -(-case.S1 // 16), -(-case.s1 // hadamard_ref.COLS_PER_WORKGROUP)], case.name
        assert got[11:] == [slab, jchunks, jper, blocks], case.name
        assert got[5:8] == [block0, sum0, slab0], case.name                 # running sums: workgroups of both launches, doubles
        assert got[8] == case.P * case.s1 * case.S1 and got[8] * jchunks == slab
        assert got[9] == ldw[k]
        strides = _case_strides(case)
        assert got[10] == (strides[2] if case.n_out > 1 else strides[0])     # the run of (gamma, i), as op_close_plan reads it
        block0 += blocks
        sum0 += min(8192, -(-got[8] // 256))
        slab0 += slab
        flops += 2.0 * case.n_in * case.P * case.S1 * (case.s * case.S * case.n_out + case.s * case.s1)
    assert p["top"] == [block0, sum0, slab0, flops, len(ref.CASES), 1]
    assert p["layout"] == [0] + [g[7] for g in p["pair"]] + [slab0]          # disjoint, one after the other, adding up to the total
    # every workgroup of the launch belongs to one (pair, j chunk, p tile, gamma' tile, c' block), and every such tile to one workgroup
    want = [(k, jc, pt, gt, cb) for k, g in enumerate(p["pair"])
            for jc, pt, gt, cb in itertools.product(range(g[0]), range(g[2]), range(g[3]), range(g[4]))]
    assert len(p["blk"]) == block0 == len(want) and [tuple(b) for b in p["blk"]] == want      # once each, c' block fastest, pairs in order
    assert [s[0] for s in p["sum"]] == [k for k, g in enumerate(p["pair"]) for _ in range(min(8192, -(-g[8] // 256)))]
    short = plan(dims, [_case_strides(c) for c in ref.CASES], ldw, work=slab0 - 1)
    assert short["rc"] == ERR_ARG and "slab" in short["msg"]
    assert plan(dims, [_case_strides(c) for c in ref.CASES], ldw, work=slab0)["rc"] == 0


def test_a_pair_is_planned_the_same_wherever_it_stands(plan):
    a, b, c = (ref.dims(ref.CASES[k]) for k in (2, 6, 10))
    first, second, alone = plan([a, b, c]), plan([c, a, b]), plan([b])
    assert first["rc"] == second["rc"] == alone["rc"] == 0
    assert [g[:5] + g[8:] for g in first["pair"]] == [g[:5] + g[8:] for g in (second["pair"][1], second["pair"][2], second["pair"][0])]
    assert alone["pair"][0][:5] == first["pair"][1][:5] and alone["pair"][0][5:8] == [0, 0, 0]


def test_every_refusal_names_its_status_and_its_pair(plan):
    ok = (2, 3, 4, 5, 6, 7, 8)
    three = [ok, (3, 2, 5, 4, 2, 3, 17), ok]
    assert plan(three)["rc"] == 0 and plan(three, accumulate=1)["rc"] == 0
    for name in ARRAYS:
        p = plan(three, null=(name,))
        assert p["rc"] == ERR_ARG and "NULL" in p["msg"], name
    assert plan(three, null=("dims",))["layout"][0] == ERR_ARG
    for pair in (0, 2):
        for name in ELEMENTS:
            p = plan(three, null_element=(pair, name))
            assert p["rc"] == ERR_ARG and "NULL" in p["msg"] and f"pair {pair}" in p["msg"], (pair, name)
        p = plan(three, ldw=[d[6] - (k == pair) for k, d in enumerate(three)])
        assert p["rc"] == ERR_ARG and "ldw" in p["msg"] and f"pair {pair}" in p["msg"]
        for field, value in itertools.product(range(7), (0, -3)):
            bad = [list(d) for d in three]
            bad[pair][field] = value
            p = plan(bad, ldw=[8, 17, 8])
            assert p["rc"] == ERR_ARG and f"pair {pair}" in p["msg"] and p["layout"][0] == ERR_ARG and f"pair {pair}" in p["layoutmsg"], (pair, field)
        # what op_close_plan refuses for a pair: an N that is not one run (a core as an MPO stores it), an extent of 2^31
        S, S1, s, s1, n_in, n_out, P = three[pair]
        strides = [_packed_strides(d) for d in three]
        strides[pair] = (n_in * n_out * S1, n_out * S1, S1, 1) + strides[pair][4:]
        p = plan(three, strides)
        assert p["rc"] == UNSUPPORTED and "one run" in p["msg"] and f"pair {pair}" in p["msg"]
        assert plan(three, strides, work=0)["rc"] == UNSUPPORTED          # the slab of a refused pair is not known
        assert plan(three, strides, accumulate=2)["rc"] == ERR_ARG          # argument errors come first
        for field in range(6):
            wide = [list(d) for d in three]
            wide[pair][field] = 2 ** 31
            p = plan(wide)
            assert p["rc"] == UNSUPPORTED and "2^31" in p["msg"] and f"pair {pair}" in p["msg"] and p["layout"][0] == UNSUPPORTED, (pair, field)
    for npairs in (0, -1):
        p = plan(three, npairs=npairs)
        assert p["rc"] == ERR_ARG and "pairs" in p["msg"] and p["layout"][0] == ERR_ARG
    for accumulate in (-1, 2):
        p = plan(three, accumulate=accumulate)
        assert p["rc"] == ERR_ARG and "accumulate" in p["msg"]
    assert plan(three, work=0)["rc"] == ERR_ARG and plan(three, work=-1)["rc"] == ERR_ARG
    # the cover: the table holds OP_CLOSE_MAX_PAIRS pairs; 2^31 workgroups in all
    most = plan([ok])["const"][0]
    assert plan([ok] * most)["rc"] == 0
    p = plan([ok] * (most + 1))
    assert p["rc"] == UNSUPPORTED and f"up to {most}" in p["msg"]
    assert plan([ok] * (most + 1), work=0)["rc"] == ERR_ARG              # argument errors come first
    big = (2, 3, 4, 5, 6, 7, 2 ** 31 - 1)                                 # 2^27 workgroups each, the in-index not cut
    assert plan([big] * 15)["rc"] == 0
    p = plan([big] * 16)
    assert p["rc"] == UNSUPPORTED and "workgroups" in p["msg"]


# ---- 2. op_gram on host factors: nothing formed, the device not touched
def _train(rng, shape, rank):
    from tt_sketch_amd import TensorTrain
    rank = (1,) + tuple(rank) + (1,)
    return TensorTrain([rng.standard_normal((rank[k], shape[k], rank[k + 1])) for k in range(len(shape))])


def _dense_apply(mpo, tt):
    A, x = mpo.to_numpy(), tt.to_numpy()
    d = x.ndim
    return np.tensordot(A, x, axes=(list(range(0, 2 * d, 2)), list(range(d))))


@pytest.mark.parametrize("d", [3, 4])
def test_host_op_gram_against_dense(d, monkeypatch):
    from tt_sketch_amd import OperatorProduct, _native as nat, operator_gram as og
    from tt_sketch_amd.tt_gmres import MPO, TTLinearMap
    shape = (3, 5, 2, 4)[:d]
    rng = np.random.default_rng(40 + d)
    rk = lambda r: (1,) + (r,) * (d - 1) + (1,)                                           # noqa: E731
    maps = [MPO([rng.standard_normal((rk(R)[k], shape[k], shape[k], rk(R)[k + 1])) for k in range(d)]) for R in (2, 3, 1)]
    x = _train(rng, shape, (3,) * (d - 1))
    b = _train(rng, shape, (2,) * (d - 1))

    class Twice(TTLinearMap):                                     # a map that is no MPO: applied, enters as a plain train
        in_shape = out_shape = shape

        def __call__(self, t):
            return t * 2.0

    members = [OperatorProduct(m, x) for m in maps] + [Twice()(x), b]
    dense = [_dense_apply(m, x) for m in maps] + [2.0 * x.to_numpy(), b.to_numpy()]
    monkeypatch.setattr(OperatorProduct, "to_tt", lambda self: pytest.fail("a product was formed"))
    monkeypatch.setattr(MPO, "__call__", lambda self, t: pytest.fail("an operator was applied"))
    monkeypatch.setattr(nat, "call", lambda *a: pytest.fail(f"the device was touched: {a[0]}"))
    G = og.op_gram(members)
    assert G.shape == (5, 5) and np.array_equal(G, G.T)
    for p, q in itertools.product(range(5), repeat=2):
        bar = 1e-12 * np.linalg.norm(dense[p]) * np.linalg.norm(dense[q])
        assert abs(G[p, q] - np.vdot(dense[p], dense[q])) <= bar, (p, q)
    two = og.op_gram(members, members)                            # the two-list form computes every entry
    assert np.array_equal(np.triu(two), np.triu(G))
    for p, q in itertools.product(range(5), repeat=2):
        assert abs(two[p, q] - G[p, q]) <= 1e-12 * np.linalg.norm(dense[p]) * np.linalg.norm(dense[q]), (p, q)
    part = og.op_gram(members[:2], members[2:])
    assert part.shape == (2, 3) and np.array_equal(part, two[:2, 2:])
    for route in ("kernel", "composed"):                          # host factors stay on the host whatever the route
        assert np.array_equal(og.op_gram(members, route=route), G)


def test_op_gram_checks_its_members_and_adds_no_name():
    import tt_sketch_amd
    from tt_sketch_amd import DenseTensor, OperatorProduct, operator_gram as og
    from tt_sketch_amd.tt_gmres import MPO
    rng = np.random.default_rng(2)
    shape = (3, 4, 2)
    x, other = _train(rng, shape, (2, 2)), _train(rng, (3, 4, 5), (2, 2))
    h = OperatorProduct(MPO([rng.standard_normal((1, n, n, 1)) for n in shape]), x)
    with pytest.raises(ValueError, match="shapes"):
        og.op_gram([h, x, other])
    with pytest.raises(ValueError, match="shapes"):
        og.op_gram([h], [other])
    with pytest.raises(TypeError, match="DenseTensor"):
        og.op_gram([h, DenseTensor(np.zeros(shape))])
    with pytest.raises(TypeError):
        og.op_gram([h], [np.zeros(shape)])
    with pytest.raises(ValueError, match="empty"):
        og.op_gram([])
    with pytest.raises(ValueError, match="route"):
        og.op_gram([h], route="fastest")
    assert "op_gram" not in tt_sketch_amd.__all__ and "operator_gram" not in tt_sketch_amd.__all__ and not hasattr(tt_sketch_amd, "op_gram")
    assert og.MAX_PAIRS == 23
