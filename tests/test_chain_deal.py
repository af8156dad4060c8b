"""The host-side deal of the fused chain step's work over a workgroup's waves (csrc/chain_deal.h, plain C++): a few
lines of driver compiled with the host compiler print the table -- for the tile structures and the k-blocks the plan
(csrc/chain_plan.h) itself derives from the ranks -- and the table is checked here, before any kernel reads it."""

import pytest

from tests.host_driver import compile_driver, run_driver

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "chain_plan.h"
int main(int argc, char **argv)
{
    if (argc != 5) return 2;
    int v[8], unr;
    for (int i = 0; i < 3; ++i) v[i] = atoi(argv[i + 1]);           // J, A, A2; then K1
    ttsk::chain_tile_split(v[1], v[3], v[4]);
    ttsk::chain_tile_split(v[2], v[5], v[6]);
    ttsk::chain_phase_a_runs(atoi(argv[4]), unr, v[7]);
    printf("split %d %d %d %d %d\n", v[3], v[4], v[5], v[6], v[7]);
    const ttsk::ChainDeal d = ttsk::chain_deal(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7]);
    printf("waves %d pieces %d useful %.6f cap %.6f simd %lld %lld %lld %lld h %d\n", d.waves, d.npieces, d.useful, d.cap(),
           d.simd[0], d.simd[1], d.simd[2], d.simd[3], ttsk::cd_cut(v[3]));
    for (int i = 0; i < d.npieces; ++i)
        printf("piece %d %d %d %d %d %lld\n", d.piece[i].tile, d.piece[i].q0, d.piece[i].nq, d.piece[i].kind, d.piece[i].slot,
               d.piece[i].cycles);
    return 0;
}
"""

WHOLE, FIRST, REST, ROWS4 = 1, 2, 3, 4

# (nb, n, K1, A, A2, J, right, T) of test_gpu_parity.test_fused_chain_step_against_einsum
PARITY_SHAPES = [
    (16, 200, 100, 100, 100, 100, True, False), (16, 200, 100, 50, 50, 100, False, True), (3, 37, 100, 100, 100, 100, True, False),
    (2, 50, 97, 100, 100, 83, True, True), (5, 64, 64, 52, 50, 33, False, True), (1, 30, 100, 98, 100, 100, False, False),
    (4, 40, 52, 36, 36, 40, False, True), (3, 33, 23, 16, 16, 20, True, False), (2, 25, 60, 112, 112, 112, True, True),
    (2, 30, 101, 70, 70, 64, False, True), (6, 30, 100, 90, 90, 100, True, False), (2, 20, 64, 22, 22, 30, True, True),
    (32, 24, 20, 50, 50, 20, False, True),
]
JS = (4, 16, 17, 96, 100, 112)


@pytest.fixture(scope="module")
def deal(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "chain_deal", DRIVER)

    def run(J, A, A2, K1):
        out = run_driver(exe, (J, A, A2, K1)).splitlines()
        nqf, strq, nnf, strn, kb1 = (int(x) for x in out[0].split()[1:])
        h = out[1].split()
        head = dict(waves=int(h[1]), npieces=int(h[3]), useful=float(h[5]), cap=float(h[7]), simd=[int(x) for x in h[9:13]],
                    h=int(h[14]), nqf=nqf, strq=strq, nnf=nnf, strn=strn, kb1=kb1)
        pieces = [dict(zip(("tile", "q0", "nq", "kind", "slot", "cycles"), map(int, l.split()[1:]))) for l in out[2:]]
        assert len(pieces) == head["npieces"]
        return head, pieces
    return run


def model_cycles(head, nfull, nstrip):
    """matrix-pipe cycles per slice: 64 per 16x16x4, 16 per 4x4x4 instruction"""
    colb = 64 * head["nnf"] + 16 * head["strn"]
    return head["kb1"] * (64 * nfull + 16 * nstrip) + (4 * nfull + nstrip) * colb


def check(head, pieces, J):
    nq_all = head["nqf"] + head["strq"]
    tiles = (J + 15) // 16
    # every (row tile with a valid row, Q) exactly once
    seen = {}
    for p in pieces:
        assert 0 <= p["tile"] < tiles and p["nq"] >= 1 and 0 <= p["q0"] and p["q0"] + p["nq"] <= nq_all, p
        for q in range(p["q0"], p["q0"] + p["nq"]):
            assert (p["tile"], q) not in seen, ("covered twice", p["tile"], q)
            seen[(p["tile"], q)] = p["kind"]
    assert set(seen) == {(t, q) for t in range(tiles) for q in range(nq_all)}
    # the kinds the kernel has bodies for, with the cut where the kernel's template puts it
    for p in pieces:
        if p["kind"] == WHOLE:
            assert (p["q0"], p["nq"]) == (0, nq_all)
            assert p["cycles"] == model_cycles(head, head["nqf"], head["strq"])
        elif p["kind"] == FIRST:
            assert (p["q0"], p["nq"]) == (0, head["h"]) and 1 <= head["h"] < head["nqf"]
            assert p["cycles"] == model_cycles(head, head["h"], 0)
        elif p["kind"] == REST:
            assert (p["q0"], p["nq"]) == (head["h"], nq_all - head["h"])
            assert p["cycles"] == model_cycles(head, head["nqf"] - head["h"], head["strq"])
        elif p["kind"] == ROWS4:
            assert (p["q0"], p["nq"]) == (0, nq_all) and p["tile"] == tiles - 1 and 1 <= J - 16 * p["tile"] <= 4
            assert p["cycles"] == 16 * nq_all * (head["kb1"] + 4 * head["nnf"] + head["strn"])
        else:
            raise AssertionError(p)
    # wave slots: distinct, the loader's (the last wave) left free, at most 168 VGPRs' worth of waves per SIMD
    slots = [p["slot"] for p in pieces]
    assert len(set(slots)) == len(slots) and all(0 <= s < head["waves"] - 1 for s in slots)
    assert head["waves"] in (8, 12)
    simd = [0, 0, 0, 0]
    for p in pieces:
        simd[p["slot"] & 3] += p["cycles"]
    assert simd == head["simd"]
    useful = J / 16.0 * model_cycles(head, head["nqf"], head["strq"])
    assert abs(useful - head["useful"]) <= 1e-6 * useful
    assert abs(head["cap"] - useful / (4.0 * max(simd))) < 1e-6
    # the two pieces of a cut row tile meet at the barrier behind the slice loop: both or neither
    assert sorted(p["tile"] for p in pieces if p["kind"] == FIRST) == sorted(p["tile"] for p in pieces if p["kind"] == REST)


@pytest.mark.parametrize("shape", PARITY_SHAPES)
def test_every_row_tile_and_q_dealt_once_parity_shapes(deal, shape):
    _, _, K1, A, A2, J, _, _ = shape
    head, pieces = deal(J, A, A2, K1)
    check(head, pieces, J)


@pytest.mark.parametrize("J", JS)
@pytest.mark.parametrize("ranks", [(100, 100), (50, 50), (52, 50), (36, 36), (16, 16), (112, 112), (22, 22), (90, 90)])
def test_every_row_tile_and_q_dealt_once(deal, J, ranks):
    head, pieces = deal(J, ranks[0], ranks[1], 100)
    check(head, pieces, J)


@pytest.mark.parametrize("J", [1, 4, 16, 17, 20, 33, 40, 48, 49, 52, 64])
@pytest.mark.parametrize("ranks", [(100, 100), (50, 50), (16, 16), (112, 112)])
def test_up_to_four_row_tiles_keep_one_wave_per_row_tile(deal, J, ranks):
    """J <= 64 is level uncut: wave w = row tile w in a workgroup of 8 waves, as before"""
    head, pieces = deal(J, ranks[0], ranks[1], 100)
    nq_all = head["nqf"] + head["strq"]
    assert head["waves"] == 8
    assert [(p["tile"], p["q0"], p["nq"], p["kind"], p["slot"]) for p in pieces] == \
        [(w, 0, nq_all, WHOLE, w) for w in range((J + 15) // 16)]


@pytest.mark.parametrize("ranks", [(100, 100), (50, 50)])
def test_modelled_cap_of_the_headline_shapes(deal, ranks):
    """J = 100: one wave per row tile has a modelled cap of 6.25 / 8 = 0.78; the bar 0.88 is 7 row tiles of 6.25 units
    over four SIMDs (10.94 per SIMD) against 9.77 useful = 0.89, less one unit of granularity"""
    head, pieces = deal(100, ranks[0], ranks[1], 100)
    check(head, pieces, 100)
    print(ranks, "modelled cap", head["cap"], "per SIMD", head["simd"])
    assert head["cap"] >= 0.88
