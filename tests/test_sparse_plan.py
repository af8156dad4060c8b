"""The host-side plan of a sparse pass (csrc/sparse_plan.h, plain C++): a few lines of driver compiled with the host
compiler print what sg_gauss_pass (csrc/sparse_fused.hip) launches sg_pass_kernel (csrc/sparse_pass.h) with, and that is
checked here -- before any kernel reads it.  tests/sparse_cases.py restates the choice of instantiation and assumes a
stretch of 256 records per wave; both are held against the launcher's own code."""

import pytest

from tests import sparse_cases as sc
from tests.host_driver import compile_driver, run_driver

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "sparse_plan.h"
using namespace ttsk;
int main(int argc, char **argv)
{
    if (argc == 2) {                                 // the lane mapping of the table DMA
        for (int units = 1; units <= 16; ++units) {
            int bad = 0;
            for (int i = 0; i < 32 * units; ++i) bad += sg_div_units(i, sg_rcp(units)) != i / units;
            printf("%d %d %d\n", units, sg_rcp(units), bad);
        }
        return 0;
    }
    if (argc != 19) return 2;
    ttsk_sg_factor f[3] = {};
    const ttsk_sg_factor *fp[3];
    for (int i = 0; i < 3; ++i) {
        char **v = argv + 1 + 5 * i;
        f[i].kind = atoi(v[0]); f[i].w = atoi(v[1]); f[i].rank_min = atoi(v[2]); f[i].full = atoi(v[3]); f[i].nnz = atoi(v[4]);
        fp[i] = f[i].kind < 0 ? nullptr : &f[i];
    }
    SgPlan p;
    const int rc = sg_plan(fp[0], fp[1], fp[2], atoi(argv[16]), (size_t)atoll(argv[17]), (size_t)atoll(argv[18]), &p);
    printf("rc %d\nmsg %s\n", rc, p.msg);
    if (rc) return 0;
    for (int i = 0; i < 3; ++i) printf("f%d %d %d %d %d %d\n", i, p.f[i].kind, p.f[i].w, p.f[i].off, p.f[i].units, p.f[i].rcp);
    printf("tile %d %d %d\ninst %d %d %d\n", p.tcols, p.tab, p.qcols, p.NT, p.NS, p.T);
    printf("grid %zu %zu %zu %zu %zu\n", p.lds, p.wg_per_cu, p.chunk, p.waves, p.blocks);
    printf("scratch %d %d %zu %zu %zu %zu\n", p.cellsP, p.cellsO, p.psi_off, p.om_off, p.j_off, p.scratch);
    const SgLds L = sg_lds_layout(p.tcols, p.tab, p.qcols, p.T);
    printf("lds %zu %zu %zu %zu %zu %zu %zu\n", L.tile, L.tabs, L.ro, L.rv, L.rj, L.q, L.total);
    printf("const %zu %zu %zu %d %d\n", SG_LDS_BUDGET, sg_salt_bytes(p.NT), SG_STATIC_SLACK, SG_MIN_TILES, SG_T);
    return 0;
}
"""

ABSENT = sc.Spec(-1, 0, 0, 0)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "sparse_plan", DRIVER)
    return lambda *args: run_driver(exe, args).splitlines()


@pytest.fixture(scope="module")
def plan(driver):
    def run(A, B, C, c_left, N, n_cu):
        args = [x for F in (A, B, C) for x in ((F or ABSENT).kind, (F or ABSENT).w, (F or ABSENT).lo, (F or ABSENT).full, (F or ABSENT).nnz)]
        out = driver(*args, c_left, N, n_cu)
        p = dict(rc=int(out[0].split()[1]), msg=out[1][4:])
        for line in out[2:]:
            key, *v = line.split()
            p[key] = [int(x) for x in v]
        return p
    return run


def check_layout(p):
    """the per-wave LDS regions and the workgroups they let a CU hold"""
    (tcols, tab, qcols), (NT, NS, T) = p["tile"], p["inst"]
    tile, tabs, ro, rv, rj, q, total = p["lds"]                    # offsets in doubles
    budget, salt, slack, _, _ = p["const"]
    assert (budget, salt) == (156 * 1024, 3 * 16 * NT * 8)
    # disjoint and in order: each region ends where the next begins, and is as long as its contents
    assert tile == 0 and tabs - tile == T * tcols and ro - tabs == tab and rv - ro == 3 * T and rj - rv == T
    assert (q - rj) * 8 == T * 4                                   # T ints
    assert total - q == (T * qcols + 3) // 4 and (total - q) * 8 >= T * qcols * 2      # T * qcols 16-bit slots
    # (every offset is in whole doubles from a wave base of `total` doubles: the uint64 row offsets are 8-byte aligned)
    assert total == T * tcols + tab + 4 * T + T // 2 + (T * qcols + 3) // 4
    lds, wg = p["grid"][:2]
    assert lds == total * 4 * 8
    assert 1 <= wg <= (3 if NT == 1 else 2) and wg * (lds + salt + slack) <= budget
    for kind, w, off, units, rcp in (p["f0"], p["f1"], p["f2"]):  # a table block: T rows of 2 units doubles inside the table region
        if kind == 1:
            assert units == (w + 1) // 2 and off % T == 0 and off + 2 * units * T <= tab


def check_grid(p, N):
    _, _, chunk, waves, blocks = p["grid"]
    assert chunk % 32 == 0 and chunk >= 256
    assert (waves - 1) * chunk < N <= waves * chunk
    assert blocks * 4 >= waves


def check_scratch(p):
    cellsP, cellsO, psi, om, jj, total = p["scratch"]
    wtot = 4 * p["grid"][4]
    ends = [(psi, psi + wtot * 2 * cellsP * 8), (om, om + wtot * cellsO * 8), (jj, jj + wtot * 3 * 4)]
    for (b0, e0), (b1, e1) in zip(ends, ends[1:]):
        assert b0 <= e0 <= b1 <= e1
    assert psi == 0 and ends[-1][1] <= total and all(b % 8 == 0 for b, _ in ends)
    assert total == wtot * ((2 * cellsP + cellsO) * 8 + 16) + 256


@pytest.mark.parametrize("cfg", sc.CONFIGS, ids=lambda c: c.name)
def test_instantiation_is_the_one_the_catalogue_restates(plan, cfg):
    p = plan(cfg.A, cfg.B, cfg.C, cfg.c_left, 1281, 256)
    assert p["rc"] == 0, p["msg"]
    assert tuple(p["inst"]) == sc.instantiation(cfg)
    wA, wB, wC = ((F.w if F else 1) for F in (cfg.A, cfg.B, cfg.C))
    assert p["scratch"][:2] == [wA * wB, 0 if cfg.C is None else (wC * wB if cfg.c_left else wA * wC)]
    check_layout(p)
    check_grid(p, 1281)
    check_scratch(p)


def test_threshold_of_the_16_record_tile(plan):
    for widths, T in (((32, 32, 8), 16), ((32, 32, 6), 32)):
        cfg = sc.table_config(widths, "both", "left")
        assert plan(cfg.A, cfg.B, cfg.C, 1, 1000, 256)["inst"] == [2, 0, T]


def test_every_wave_of_the_catalogue_gets_256_records(plan):
    """the assumption at the top of tests/sparse_cases.py"""
    for N in sorted({s.j.size for s in sc.structures()} | {66000}):
        for cfg in sc.CONFIGS:
            assert plan(cfg.A, cfg.B, cfg.C, cfg.c_left, N, 256)["grid"][2] == 256, (N, cfg.name)


@pytest.mark.parametrize("n_cu", [1, 256])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 66000, 10 ** 7])
def test_grid_covers_the_stream(plan, N, n_cu):
    for cfg in (sc.table_config((16, 16, 16), "both", "left"), sc.table_config((32, 32, 32), "both", "right"), sc.SAMPLED_CONFIGS[0]):
        p = plan(cfg.A, cfg.B, cfg.C, cfg.c_left, N, n_cu)
        check_grid(p, N)
        check_layout(p)
        check_scratch(p)


def test_dma_lane_mapping_divides_exactly(driver):
    rows = [[int(x) for x in line.split()] for line in driver("rcp")]
    assert [r[0] for r in rows] == list(range(1, 17))
    for units, rcp, bad in rows:
        assert bad == 0 and all((i * rcp) >> 16 == i // units for i in range(32 * units)), units
        assert 32 * units * rcp < 2 ** 31                          # the product stays an int


def test_plan_refuses_what_the_pass_refuses(plan):
    """the factor fields of test_gpu_sparse_pass.test_pass_refuses_bad_arguments_before_any_launch, each with its own message"""
    ok = sc.Spec(1, 4, 0, 0)
    refused = {"factor 0: kind 1, width 33": (sc.Spec(1, 33, 0, 0), None),
               "factor 1: sign row of 33 entries, 2 non-zero, columns [0, 8)": (ok, sc.Spec(3, 8, 0, 1, 33, 2)),
               "factor 1: sign row of 12 entries, 2 non-zero, columns [5, 13)": (ok, sc.Spec(3, 8, 5, 1, 12, 2))}
    for msg, (A, B) in refused.items():
        p = plan(A, B, None, 0, 40, 256)
        assert p["rc"] == -2 and p["msg"] == "ttsk_sparse_gauss_pass: " + msg, p
    assert plan(ok, sc.Spec(3, 8, 4, 1, 12, 2), None, 0, 40, 256)["rc"] == 0
