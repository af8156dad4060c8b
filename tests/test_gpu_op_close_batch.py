"""Many pairs of operator-times-train products closed in one launch, on the device: ``ttsk_op_close_batch``
(csrc/op_close.hip) against ``ttsk_op_close`` bit for bit, its refusals, ``operator_gram.op_gram`` on resident factors against
dense NumPy on every route, and ``TTLinearMapSum.residual`` through it.

Bars: a pair of the batch holds the floats of ``ttsk_op_close`` on the same operands (``np.array_equal``) and lies inside
``op_close_ref.bound`` of the ``np.longdouble`` restatement; nothing is written outside the outputs and the slab; inner
products within 1e-12 ||a|| ||b|| of the dense ones, the residual within 1e-10 relative.
"""
import ctypes
import itertools

import numpy as np
import pytest

from tests import op_close_ref as ref
from tests.edge_kit import tsa  # noqa: F401

pytestmark = pytest.mark.gpu

UNSUPPORTED = -3
GUARD = 16                     # doubles of NaN on both sides of every output and of the slab
ROUTES = ("kernel", "composed", None)


@pytest.fixture(scope="module")
def truth():
    """per case: the operands, the np.longdouble restatement without and with a prefilled `out` the test draws, and the bounds"""
    out = {}
    for case in ref.CASES:
        Wl, N, Y, _ = ref.case_arrays(case)
        out0 = np.random.default_rng(len(case.name)).standard_normal((case.P, case.s1 * case.S1))
        out[case.name] = dict(Wl=Wl, N=N, Y=Y, out0=out0,
                              exact=(ref.close_term(Wl, N, Y, dtype=np.longdouble), ref.close_term(Wl, N, Y, out0, dtype=np.longdouble)),
                              bound=(ref.bound(Wl, N, Y), ref.bound(Wl, N, Y, out0)))
    return out


def _single(t, accumulate):
    """ttsk_op_close on the operands of one pair"""
    from tests.test_gpu_op_close import c_op_close
    rc, got, _ = c_op_close(t["Wl"], t["N"], t["Y"], t["out0"] if accumulate else None)
    assert rc == 0
    return got


def c_batch(pairs, accumulate, **kw):
    """One direct call of the C entry for the operand dicts `pairs`: every Wl a column slice of ONE wider buffer (so that ldw
    is the width of that buffer, above every P), every out and the slab cut out of buffers of NaN with GUARD doubles on both
    sides.  The outs hold NaN before the call, or their out0 when it accumulates.  Keywords overwrite what the arrays say, for
    the refusals: npairs, accumulate_arg, work_doubles, null (names of arrays), null_element (pair, name), dims, ldw,
    n_strides (pair, strides of its N), strides (of every N and Y).  Returns (status, outs, slab, guards of the outs, guards of the slab, slab size)."""
    from tests.test_gpu_op_close import _upload
    from tt_sketch_amd import _native as nat
    from tt_sketch_amd.device import DevArray
    n = len(pairs)
    width = sum(t["Wl"].shape[2] for t in pairs) + 3
    rows = max(t["Wl"].shape[0] * t["Wl"].shape[1] for t in pairs)
    Wbuf = np.full((rows, width), np.nan)
    at, wcol = 2, []
    for t in pairs:
        W = t["Wl"]
        Wbuf[:W.shape[0] * W.shape[1], at:at + W.shape[2]] = W.reshape(-1, W.shape[2])
        wcol.append(at)
        at += W.shape[2]
    dW = DevArray.from_host(Wbuf)
    dN, dY = [_upload(t["N"]) for t in pairs], [_upload(t["Y"]) for t in pairs]
    dims = [t["N"].shape[0:1] + t["N"].shape[3:4] + t["Y"].shape[0:1] + t["Y"].shape[2:3] + t["N"].shape[1:3] + t["Wl"].shape[2:3] for t in pairs]
    slabs = [ref.layout(*d)[2] for d in dims]
    sizes = [t["out0"].size for t in pairs]
    starts = np.cumsum([GUARD] + [s + GUARD for s in sizes])[:-1]
    obuf = np.full(int(starts[-1] + sizes[-1] + GUARD), np.nan)
    if accumulate:
        for t, o, s in zip(pairs, starts, sizes):
            obuf[o:o + s] = t["out0"].ravel()
    dO = DevArray.from_host(obuf)
    slab = sum(slabs)
    dS = DevArray.from_host(np.full(slab + 2 * GUARD, np.nan))
    ptrs = lambda addresses: (ctypes.c_void_p * len(addresses))(*addresses)                 # noqa: E731
    strides = [tuple(a.strides) + tuple(b.strides) for a, b in zip(dN, dY)]
    if "strides" in kw:
        strides = list(kw["strides"])
    if "n_strides" in kw:
        strides[kw["n_strides"][0]] = tuple(kw["n_strides"][1]) + strides[kw["n_strides"][0]][4:]
    arrays = dict(Wl=[dW.ptr + 8 * c for c in wcol], N=[a.ptr for a in dN], Y=[a.ptr for a in dY], out=[dO.ptr + 8 * int(o) for o in starts])
    if "null_element" in kw:
        arrays[kw["null_element"][1]][kw["null_element"][0]] = None
    args = dict({k: ptrs(v) for k, v in arrays.items()}, dims=nat.i64_array([x for d in kw.get("dims", dims) for x in d]),
                strides=nat.i64_array([x for s in strides for x in s]), ldw=nat.i64_array(kw.get("ldw", [width] * n)),
                work=ctypes.c_void_p(dS.ptr + 8 * GUARD))
    for name in kw.get("null", ()):
        args[name] = None
    rc = nat.lib().ttsk_op_close_batch(kw.get("npairs", n), args["Wl"], args["N"], args["Y"], args["dims"], args["strides"], args["ldw"], args["out"],
                                       kw.get("accumulate_arg", 1 if accumulate else 0), args["work"], kw.get("work_doubles", slab), 0)
    nat.call("ttsk_sync", -1)
    o, w = dO.get(), dS.get()
    outs = [o[a:a + s].reshape(t["out0"].shape) for t, a, s in zip(pairs, starts, sizes)]
    mask = np.ones(o.size, bool)
    for a, s in zip(starts, sizes):
        mask[a:a + s] = False
    return rc, outs, w[GUARD:GUARD + slab], o[mask], np.concatenate([w[:GUARD], w[GUARD + slab:]]), slab


# ---- 1. the kernel against the single call, bit for bit
@pytest.mark.parametrize("accumulate", [0, 1])
def test_the_twelve_cases_as_one_batch_are_twelve_single_calls(tsa, truth, accumulate):
    from tt_sketch_amd import _native as nat
    pairs = [truth[c.name] for c in ref.CASES]
    widths = {t["Wl"].shape[2] for t in pairs}
    rc, outs, slab, og, sg, size = c_batch(pairs, accumulate)
    assert rc == 0, nat.lib().ttsk_last_error()
    assert sum(widths) + 3 > max(widths)                                # ldw differs from every P
    assert np.isnan(og).all() and np.isnan(sg).all()                    # the guards
    assert np.isfinite(slab).all()                                      # every double of the slab is written
    for case, t, got in zip(ref.CASES, pairs, outs):
        want = _single(t, accumulate)
        print(f"{case.name}, accumulate {accumulate}: {np.count_nonzero(got != want)} of {want.size} floats differ from ttsk_op_close; "
              f"max |G' - exact| / bound = {float(np.max(np.abs(got - t['exact'][accumulate]) / np.maximum(t['bound'][accumulate], 1e-300))):.3f}")
        assert np.array_equal(got, want), case.name
        assert (np.abs(got - t["exact"][accumulate]) <= t["bound"][accumulate]).all(), case.name
    rc2, outs2, slab2, _, _, _ = c_batch(pairs, accumulate)
    assert rc2 == 0 and all(np.array_equal(a, b) for a, b in zip(outs, outs2)) and np.array_equal(slab, slab2)      # the same bits on a second call
    offs = nat.i64_array([0] * (len(pairs) + 1))
    nat.call("ttsk_op_close_batch_layout", len(pairs), nat.i64_array([x for c in ref.CASES for x in ref.dims(c)]), offs)
    assert list(offs) == list(np.cumsum([0] + [ref.layout(*ref.dims(c))[2] for c in ref.CASES])) and offs[len(pairs)] == size


def test_the_position_in_the_table_does_not_matter(tsa, truth):
    names = [ref.CASES[k].name for k in (2, 6, 10)]
    a, b, c = (truth[n] for n in names)
    want = {n: _single(truth[n], 0) for n in names}
    for order in ((a, b, c), (c, a, b)):
        rc, outs, _, og, sg, _ = c_batch(list(order), 0)
        assert rc == 0 and np.isnan(og).all() and np.isnan(sg).all()
        for t, got in zip(order, outs):
            name = next(n for n in names if truth[n] is t)
            assert np.array_equal(got, want[name]), name
    rc, outs, _, og, sg, _ = c_batch([b], 0)
    assert rc == 0 and np.array_equal(outs[0], want[names[1]]) and np.isnan(og).all() and np.isnan(sg).all()


# ---- 2. the ABI
def test_refusals_write_nothing(tsa, truth):
    from tt_sketch_amd import _native as nat
    pairs = [truth[ref.CASES[k].name] for k in (7, 2, 9)]              # S, n_out > 1 in the first and the last
    rc, _, _, _, _, slab = c_batch(pairs, 1)
    assert rc == 0
    good = [t["N"].shape[0:1] + t["N"].shape[3:4] + t["Y"].shape[0:1] + t["Y"].shape[2:3] + t["N"].shape[1:3] + t["Wl"].shape[2:3] for t in pairs]
    width = sum(t["Wl"].shape[2] for t in pairs) + 3

    def status(**kw):
        rc, outs, work, og, sg, _ = c_batch(pairs, 1, **kw)
        assert all(np.array_equal(o, t["out0"]) for o, t in zip(outs, pairs)), kw      # refused before anything is launched
        assert np.isnan(work).all() and np.isnan(og).all() and np.isnan(sg).all(), kw
        return rc, nat.lib().ttsk_last_error()

    for name in ("Wl", "N", "Y", "dims", "strides", "ldw", "out", "work"):
        rc, msg = status(null=(name,))
        assert rc == nat.TTSK_ERR_ARG and b"NULL" in msg, name
    for npairs in (0, -1):
        assert status(npairs=npairs)[0] == nat.TTSK_ERR_ARG
    for value in (2, -1):
        rc, msg = status(accumulate_arg=value)
        assert rc == nat.TTSK_ERR_ARG and b"accumulate" in msg
    rc, msg = status(work_doubles=slab - 1)
    assert rc == nat.TTSK_ERR_ARG and b"slab" in msg
    for pair in (0, len(pairs) - 1):
        where = f"pair {pair}".encode()
        for name in ("Wl", "N", "Y", "out"):
            rc, msg = status(null_element=(pair, name))
            assert rc == nat.TTSK_ERR_ARG and b"NULL" in msg and where in msg, (pair, name)
        ldw = [width] * len(pairs)
        ldw[pair] = good[pair][6] - 1
        rc, msg = status(ldw=ldw)
        assert rc == nat.TTSK_ERR_ARG and b"ldw" in msg and where in msg
        S, S1, s, s1, n_in, n_out, P = good[pair]
        assert S > 1 and n_out > 1
        rc, msg = status(n_strides=(pair, (n_in * n_out * S1, n_out * S1, S1, 1)))      # a core as an MPO stores it
        assert rc == UNSUPPORTED and b"one run" in msg and where in msg
        for field in range(6):                                          # refused by arithmetic alone: nothing of that size exists
            dims = [list(d) for d in good]
            dims[pair][field] = 2 ** 31
            rc, msg = status(dims=dims, work_doubles=2 ** 62)
            assert rc == UNSUPPORTED and b"2^31" in msg and where in msg, (pair, field)
        dims = [list(d) for d in good]
        dims[pair][2] = 0
        rc, msg = status(dims=dims)
        assert rc == nat.TTSK_ERR_ARG and where in msg


def test_more_pairs_than_the_table_holds_and_too_many_workgroups(tsa, truth):
    from tt_sketch_amd import _native as nat, operator_gram as og
    t = truth[ref.CASES[0].name]
    rc, outs, work, g1, g2, _ = c_batch([t] * (og.MAX_PAIRS + 1), 1)
    assert rc == UNSUPPORTED and f"up to {og.MAX_PAIRS}".encode() in nat.lib().ttsk_last_error()
    assert all(np.array_equal(o, t["out0"]) for o in outs) and np.isnan(work).all() and np.isnan(g1).all() and np.isnan(g2).all()
    rc, outs, _, g1, g2, _ = c_batch([t] * og.MAX_PAIRS, 0)            # a full table: the outs overlap nowhere, every pair its own
    assert rc == 0 and np.isnan(g1).all() and np.isnan(g2).all() and all(np.array_equal(o, outs[0]) for o in outs)
    big = [[2, 3, 4, 5, 6, 7, 2 ** 31 - 1]] * 16                        # 2^27 workgroups each
    packed = [(7 * 6 * 3, 3, 6 * 3, 1, 6 * 5, 5, 1)] * 16                # of contiguous (S, n_out, n_in, S') and (s, n_in, s') cores
    rc, outs, work, g1, g2, _ = c_batch([t] * 16, 1, dims=big, strides=packed, ldw=[2 ** 31] * 16, work_doubles=2 ** 62)
    assert rc == UNSUPPORTED and b"workgroups" in nat.lib().ttsk_last_error()
    assert all(np.array_equal(o, t["out0"]) for o in outs) and np.isnan(work).all() and np.isnan(g1).all() and np.isnan(g2).all()


# ---- 3. op_gram on resident factors
OUT = {3: (4, 6, 3), 4: (5, 3, 4, 6)}
IN_X = {3: (5, 2, 6), 4: (3, 6, 2, 5)}                                  # x and y live on other mode sizes than the products
IN_Y = {3: (3, 4, 1), 4: (4, 2, 5, 3)}
TRAIN_RANKS = {3: dict(x=(3, 5), y=(4, 2), z=(5, 3), b=(2, 4), w=(3, 3)),
               4: dict(x=(3, 5, 2), y=(2, 4, 5), z=(3, 4, 4), b=(2, 3, 2), w=(4, 3, 2))}
OP_RANKS = {3: dict(M=(3, 2), N=(2, 3), A=((2, 3), (1, 2), (3, 1))),
            4: dict(M=(2, 3, 2), N=(3, 2, 3), A=((2, 3, 2), (1, 1, 2), (3, 2, 1)))}


def _cores(rng, shapes, rank):
    rank = (1,) + tuple(rank) + (1,)
    return [rng.standard_normal((rank[k],) + tuple(sh) + (rank[k + 1],)) for k, sh in enumerate(shapes)]


@pytest.fixture(scope="module")
def resident(tsa):
    """per d: resident trains and operators, the lazy products and every dense tensor, computed once.  h = M x and q = N y map
    other shapes onto the one of z and b; the three A_p, of different ranks, map that shape onto itself and act on w."""
    from tt_sketch_amd.tt_gmres import MPO, TTLinearMapSum
    out = {}
    for d, shape in OUT.items():
        rng = np.random.default_rng(80 + d)
        tr = dict(x=_cores(rng, [(n,) for n in IN_X[d]], TRAIN_RANKS[d]["x"]), y=_cores(rng, [(n,) for n in IN_Y[d]], TRAIN_RANKS[d]["y"]))
        for k in ("z", "b", "w"):
            tr[k] = _cores(rng, [(n,) for n in shape], TRAIN_RANKS[d][k])
        ops = dict(M=_cores(rng, zip(IN_X[d], shape), OP_RANKS[d]["M"]), N=_cores(rng, zip(IN_Y[d], shape), OP_RANKS[d]["N"]))
        As = [_cores(rng, zip(shape, shape), rk) for rk in OP_RANKS[d]["A"]]
        t = {k: tsa.TensorTrain(v).to_device() for k, v in tr.items()}
        mpos = {k: MPO(v) for k, v in ops.items()}
        maps = [MPO(A) for A in As]
        for m in list(mpos.values()) + maps:
            m.dev_views()                                               # uploaded once, before the host is closed
            assert m.resident()
        members = [tsa.OperatorProduct(mpos["M"], t["x"]), tsa.OperatorProduct(mpos["N"], t["y"])] + \
                  [tsa.OperatorProduct(m, t["w"]) for m in maps] + [t["z"], t["b"]]
        dense = [ref.dense_product(ops["M"], tr["x"]), ref.dense_product(ops["N"], tr["y"])] + [ref.dense_product(A, tr["w"]) for A in As] + \
                [tsa.TensorTrain(tr[k]).to_numpy() for k in ("z", "b")]
        out[d] = dict(members=members, dense=dense, A=TTLinearMapSum(maps), w=t["w"], b=t["b"])
    return out


def _assert_gram(G, rows, cols):
    assert G.shape == (len(rows), len(cols))
    worst = 0.0
    for (p, a), (q, b) in itertools.product(enumerate(rows), enumerate(cols)):
        bar = 1e-12 * np.linalg.norm(a) * np.linalg.norm(b)
        worst = max(worst, abs(G[p, q] - np.vdot(a, b)) / bar)
        assert abs(G[p, q] - np.vdot(a, b)) <= bar, (p, q)
    print(f"worst entry at {worst:.3g} of the bar")


def _close_the_host(monkeypatch):
    from tt_sketch_amd import OperatorProduct, operator_gram as og, tensor as tmod
    from tt_sketch_amd.tt_gmres import MPO

    def closed(*a, **k):
        raise AssertionError("host detour: tensor._host, to_tt or an applied operator")
    monkeypatch.setattr(tmod, "_host", closed)
    monkeypatch.setattr(og, "_host", closed)
    monkeypatch.setattr(OperatorProduct, "to_tt", closed)
    monkeypatch.setattr(MPO, "__call__", closed)


@pytest.mark.parametrize("host", ["open", "closed"])
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("d", sorted(OUT))
def test_op_gram_against_dense(tsa, resident, d, route, host, monkeypatch):
    from tt_sketch_amd import operator_gram as og
    e = resident[d]
    if host == "closed":
        _close_the_host(monkeypatch)
    G = og.op_gram(e["members"], route=route)
    assert np.array_equal(G, G.T)
    _assert_gram(G, e["dense"], e["dense"])
    two = og.op_gram(e["members"][:3], e["members"][2:], route=route)   # two lists: trains on the right, products on both sides
    _assert_gram(two, e["dense"][:3], e["dense"][2:])
    swapped = og.op_gram(e["members"][5:], e["members"][:2], route=route)      # trains on the left: the swapped pairs
    _assert_gram(swapped, e["dense"][5:], e["dense"][:2])


@pytest.mark.parametrize("route", ROUTES)
def test_op_gram_of_reversed_members(tsa, resident, route):
    from tt_sketch_amd import operator_gram as og
    e = resident[4]
    G = og.op_gram([m.T for m in e["members"]], route=route)
    _assert_gram(G, e["dense"], e["dense"])                             # <a.T, b.T> = <a, b>


def test_a_small_budget_cuts_a_mode_into_three_slices(tsa, resident, monkeypatch):
    from tt_sketch_amd import _native as nat, hadamard_gram as hg, operator_gram as og
    e = resident[3]
    members = e["members"]
    whole = og.op_gram(members, route="kernel")
    # the second mode of d = 3 has n_out = 6: a budget of two i of the W of all pairs together
    pairs = [(a, b) for p, a in enumerate(members) for b in members[p:] if isinstance(a, tsa.OperatorProduct) or isinstance(b, tsa.OperatorProduct)]
    rows = 0
    for a, b in pairs:
        a, b = (a, b) if isinstance(a, tsa.OperatorProduct) else (b, a)         # a train on the left is the swapped pair
        rows += b.rank[0] * a.rank[1]                                           # l = s S of the right side, P = R' r' of the left
    monkeypatch.setattr(hg, "W_BUDGET_BYTES", 8 * 2 * rows)
    seen, real = [], nat.call
    try:
        nat.call = lambda entry, *args: (seen.append((entry, args)), real(entry, *args))[1]
        cut = og.op_gram(members, route="kernel")
    finally:
        nat.call = real
    closes = [(int(a[4][5]), int(a[8])) for entry, a in seen if entry == "ttsk_op_close_batch"]
    per = -(-len(pairs) // og.MAX_PAIRS)                                # 25 pairs: a list longer than the table is cut into two calls
    assert len(pairs) == 25 and per == 2
    assert closes[:per] == [(4, 0)] * per and closes[per:4 * per] == [(2, 0)] * per + [(2, 1)] * (2 * per), closes
    _assert_gram(cut, e["dense"], e["dense"])
    assert (np.abs(cut - whole) <= 1e-13 * np.abs(whole)).all()


@pytest.mark.parametrize("d", sorted(OUT))
def test_a_pair_of_the_batch_has_the_bits_of_the_pair_alone(tsa, resident, d):
    from tt_sketch_amd import operator_gram as og, paths
    members = resident[d]["members"][:5]                                # the five products
    with paths.forced("kernel"):
        G = og.op_gram(members)
        two = og.op_gram(members[:2], members[1:])
        for p, q in itertools.product(range(5), repeat=2):
            alone = og.op_dot(members[p], members[q])
            if q >= p:
                assert G[p, q] == alone, (p, q)
            if p < 2 and q >= 1:
                assert two[p, q - 1] == alone, (p, q)
        assert np.array_equal(og.op_gram(members), G)                   # the same bits on a second call


def test_launches_and_the_one_read_back(tsa, resident):
    from tt_sketch_amd import _native as nat, operator_gram as og
    e = resident[4]
    members = e["members"][2:5] + [e["b"]]                              # three products of different ranks and a train
    og.op_gram(members, route="kernel")                                 # the operators are packed
    seen, real = [], nat.call
    try:
        nat.call = lambda entry, *args: (seen.append((entry, args)), real(entry, *args))[1]
        G = og.op_gram(members, route="kernel")
    finally:
        nat.call = real
    names = [entry for entry, _ in seen]
    d = len(OUT[4])
    assert names.count("ttsk_op_close_batch") == d                     # once per mode: no mode is cut here
    assert all(int(a[0]) == 9 for entry, a in seen if entry == "ttsk_op_close_batch")      # six product pairs, three against b
    assert names.count("ttsk_op_close") == 0 and names.count("ttsk_gemm") == 0
    # half A: one call per distinct l = s S among the pairs of a mode (the first mode: l = 1 for all)
    at, calls = 0, []
    for entry, a in seen:
        if entry == "ttsk_op_apply":
            calls.append((at, int(a[6])))
        if entry == "ttsk_op_close_batch":
            at += 1
    for mode in range(d):
        ls = [l for m, l in calls if m == mode]
        assert len(ls) == len(set(ls)) and len(ls) >= 1, (mode, ls)
    assert [l for m, l in calls if m == 0] == [1] and any(len([l for m, l in calls if m == k]) > 1 for k in range(1, d))
    assert names.count("ttsk_tt_gram") == 1 and names.count("ttsk_d2h") == 1      # one read-back for all ten scalars
    _assert_gram(G, e["dense"][2:5] + [e["dense"][6]], e["dense"][2:5] + [e["dense"][6]])


# ---- 4. the residual of a sum of operators
@pytest.mark.parametrize("host", ["open", "closed"])
@pytest.mark.parametrize("d", sorted(OUT))
def test_residual_through_op_gram(tsa, resident, d, host, monkeypatch):
    from tt_sketch_amd import operator_gram as og
    e = resident[d]
    A, w, b, D = e["A"], e["w"], e["b"], e["dense"]
    if host == "closed":
        _close_the_host(monkeypatch)
    res = D[6] - sum(D[2:5])
    want, bn = np.linalg.norm(res), np.linalg.norm(D[6])
    assert want / bn >= 0.1                                             # far above the floor of the squares' difference
    got, rel = A.residual(w, b), A.residual(w, b, relative=True)
    print(f"d = {d}: residual {got!r}, dense {want!r}")
    assert abs(got - want) <= 1e-10 * want and abs(rel - want / bn) <= 1e-10 * want / bn
    G = og.op_gram([tsa.OperatorProduct(m, w) for m in A.linear_maps] + [b])
    total = float(G[3, 3]) - 2.0 * float(G[:3, 3].sum()) + float(G[:3, :3].sum())
    assert got == float(np.sqrt(max(total, 0.0))) and rel == got / float(np.sqrt(G[3, 3]))
