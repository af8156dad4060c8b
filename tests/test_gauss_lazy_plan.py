"""The host-side plan of the lazy-Gaussian products (csrc/gauss_lazy_plan.h, plain C++, compiled by the host compiler alone):
grids, LDS, the chunking of the contracted extent, the workspace, the sample count, the refusals -- and that every case of
the table the device test runs (tests/gauss_lazy_cases.py) reaches the plan branch its tag names, every branch by some case."""
import pytest

from tests import gauss_lazy_cases as glc
from tests.host_driver import compile_driver, run_driver

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "gauss_lazy_plan.h"
using namespace ttsk;
static double dummy;
// one call per line of stdin: side lo hi cols x N ldx d ldd (x, d: 1 for a pointer, 0 for NULL)
int main()
{
    printf("const %d %d %d %d %d %d %d %lld %lld %lld %zu\n", GL_THREADS, GL_W_MAX, GL_KB, GL_NT, GL_GP, GL_XP, GL_XPK, (long long)GL_KCH,
           (long long)GL_SPLIT_TILES, (long long)GL_WG_TARGET, GL_LDS_LIMIT);
    long long side, lo, hi, cols, x, N, ldx, d, ldd;
    while (scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld", &side, &lo, &hi, &cols, &x, &N, &ldx, &d, &ldd) == 9) {
        GlPlan p;
        const int rc = gauss_lazy_plan((int)side, lo, hi, cols, x ? &dummy : nullptr, N, ldx, d ? &dummy : nullptr, ldd, &p);
        printf("%d %d %d %d %d %lld %lld %lld %lld %lld %lld %lld %zu %.17g %.17g %.17g|%s\n", rc, p.side, p.branch, p.w, p.mt, (long long)p.K,
               (long long)p.N, (long long)p.tiles, (long long)p.chunk, (long long)p.nchunks, (long long)p.ws_elems, (long long)p.close_blocks, p.lds,
               p.samples, p.flops, p.bytes, p.msg);
    }
    return 0;
}
"""
FIELDS = "rc side branch w mt K N tiles chunk nchunks ws_elems close_blocks lds".split()
NOTHING, DIRECT, SPLIT = 0, 1, 2
LEFT, RIGHT = 0, 1


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    exe = compile_driver(tmp_path_factory, "gauss_lazy_plan", DRIVER)

    def run(calls):
        """calls: dicts of side lo hi cols x N ldx d ldd -> (the constants, one dict per call)"""
        lines = []
        for c in calls:
            side, w_min = c["side"], c["hi"] - c["lo"]
            ldx = c.get("ldx", c["N"] if side == LEFT else c["cols"])
            ldd = c.get("ldd", c["N"] if side == LEFT else w_min)
            lines.append(" ".join(str(v) for v in (side, c["lo"], c["hi"], c["cols"], c.get("x", 1), c["N"], ldx, c.get("d", 1), ldd)))
        out = run_driver(exe, stdin="\n".join(lines) + "\n").splitlines()
        assert len(out) == len(calls) + 1
        const = [int(v) for v in out[0].split()[1:]]
        res = []
        for line in out[1:]:
            nums, msg = line.split("|", 1)
            v = nums.split()
            p = {k: int(x) for k, x in zip(FIELDS, v)}
            p.update(samples=float(v[13]), flops=float(v[14]), bytes=float(v[15]), msg=msg)
            res.append(p)
        return const, res
    return run


def _call(side, lo, w, K, N, **kw):
    return dict(side=LEFT if side in (LEFT, "left") else RIGHT, lo=lo, hi=lo + w, cols=K, N=N, **kw)


def test_constants_and_lds(plans):
    const, (p,) = plans([_call("left", 0, 64, 64, 64)])
    threads, w_max, kb, nt, gp, xp, xpk, kch, split_tiles, wg_target, lds_limit = const
    assert (threads, w_max, kb, nt) == (256, 64, 16, 256)
    assert gp % 32 == 16 and xp % 32 == 16 and xpk % 2 == 1            # LDS pitches: 16 modulo 32 doubles, or odd
    assert gp >= w_max and xp >= nt and xpk >= kb
    assert nt == 4 * 4 * 16 and kb % 4 == 0                           # four waves x four 16-column tiles; whole 16x16x4 steps
    assert p["lds"] == 8 * kb * gp + 8 * max(kb * xp, nt * xpk) + 2 * kb * gp + 4
    assert p["lds"] <= lds_limit == 64 * 1024
    assert kb * gp <= 65536                                           # a slot of the tail queue is an unsigned short
    assert kch % kb == 0 and wg_target <= 65535                       # chunks are whole steps; gridDim.y


def test_every_case_of_the_device_table_reaches_its_branch(plans):
    _, res = plans([_call(c.side, c.lo, c.w, c.K, c.N) for c in glc.ALL])
    seen = set()
    for c, p in zip(glc.ALL, res):
        assert p["rc"] == 0, (c, p)
        tag = {DIRECT: "direct", SPLIT: "split"}[p["branch"]] + str(p["mt"])
        assert tag == c.tag, (c, p)
        assert p["side"] == (c.side == "right") and (p["w"], p["K"], p["N"]) == (c.w, c.K, c.N)
        seen.add(tag)
    assert sorted(seen) == glc.TAGS and len(seen) == 8


def _cdiv(a, b):
    return -(-a // b)


def _expected(w, K, N, const):
    kch, split_tiles, wg_target = const[7:10]
    tiles = _cdiv(N, 256)
    if tiles >= split_tiles or K <= kch:
        chunk, nchunks = K, 1
    else:
        chunk = kch * _cdiv(_cdiv(K, kch), _cdiv(wg_target, tiles))
        nchunks = _cdiv(K, chunk)
    split = nchunks > 1
    return dict(tiles=tiles, chunk=chunk, nchunks=nchunks, branch=SPLIT if split else DIRECT, ws_elems=nchunks * w * N if split else 0,
                close_blocks=min(_cdiv(w * N, 256), 4096) if split else 0, mt=_cdiv(w, 16))


@pytest.mark.parametrize("side", ["left", "right"])
def test_grids_chunks_workspace_and_counts(plans, side):
    shapes = [(w, K, N) for w in (1, 16, 17, 33, 64) for K in (1, 255, 256, 257, 512, 513, 4096, 10 ** 6, 2 ** 24, 2 ** 31 - 1)
              for N in (1, 64, 256, 257, 65 * 256, 255 * 256, 255 * 256 + 1, 2 ** 24, 2 ** 31 - 1)]
    const, res = plans([_call(side, 3, w, K, N) for w, K, N in shapes])
    for (w, K, N), p in zip(shapes, res):
        assert p["rc"] == 0, (w, K, N, p)
        want = _expected(w, K, N, const)
        assert {k: p[k] for k in want} == want, (w, K, N, p, want)
        # every k belongs to exactly one chunk, whole steps of 16 but for the last chunk's end; the grid fits
        assert (p["nchunks"] - 1) * p["chunk"] < K <= p["nchunks"] * p["chunk"]
        assert p["nchunks"] == 1 or p["chunk"] % 256 == 0
        assert p["tiles"] * p["nchunks"] <= max(p["tiles"], 2 * 512) and p["nchunks"] <= 65535 and p["tiles"] < 2 ** 31
        assert p["ws_elems"] * 8 <= 2 ** 28                            # the workspace stays below 256 MB
        # a sample once per (column tile, k) and row; flops; X and D once, the workspace written and read
        assert p["samples"] == p["tiles"] * w * K
        assert p["flops"] == 2.0 * w * K * N
        assert abs(p["bytes"] - 8 * (K * N + w * N + 2 * p["ws_elems"])) <= 1e-14 * p["bytes"]
    # the C2 levels (64^5, rank 20): the left product of level 0 samples w N / 256 values
    _, (p,) = plans([_call("left", 0, 20, 64, 64 ** 4)])
    assert p["branch"] == DIRECT and p["samples"] == 20 * 64 ** 5 / 256


def test_nothing_to_do(plans):
    _, res = plans([_call("left", 4, 0, 7, 9, x=0, d=0), _call("right", 0, 5, 7, 0, x=0, d=0)])
    for p in res:
        assert p["rc"] == 0 and p["branch"] == NOTHING and p["tiles"] == 0 and p["msg"] == "", p


@pytest.mark.parametrize("side", ["left", "right"])
def test_refusals(plans, side):
    who = "ttsk_gauss_lazy_" + side
    big = 2 ** 31
    calls = [
        (_call(side, 0, 65, 8, 8), -3, "%s: 65 rows of G, up to 64 are covered" % who),
        (_call(side, 0, 4, big, 8), -3, "%s: extents %d and 8, below 2^31 are covered" % (who, big)),
        (_call(side, 0, 4, 8, big), -3, "%s: extents 8 and %d, below 2^31 are covered" % (who, big)),
        (_call(side, 2 ** 40, 1, 2 ** 30, 8), -3, "%s: the flat index of row %d and %d columns passes 2^63" % (who, 2 ** 40, 2 ** 30)),
        (_call(side, 0, 4, 8, 8, x=0), -2, "%s: NULL operand or output" % who),
        (_call(side, 0, 4, 8, 8, d=0), -2, "%s: NULL operand or output" % who),
        (_call(side, -1, 4, 8, 8), -2, None), (_call(side, 0, 4, 0, 8), -2, None), (_call(side, 0, 4, 8, -1), -2, None),
        (dict(side=LEFT if side == "left" else RIGHT, lo=5, hi=4, cols=8, N=8), -2, None),
        (_call(side, 0, 4, 8, 9, ldx=7), -2, None), (_call(side, 0, 4, 8, 9, ldd=3), -2, None),
    ]
    _, res = plans([c for c, _, _ in calls])
    for (c, rc, msg), p in zip(calls, res):
        assert p["rc"] == rc and (msg is None or p["msg"] == msg) and p["msg"], (c, p)
        assert p["branch"] == NOTHING and p["tiles"] == 0 and p["ws_elems"] == 0
    # the last index that is covered: row_hi * cols == 2^63 exactly
    _, (p,) = plans([_call(side, 2 ** 33 - 1, 1, 2 ** 30, 8)])
    assert p["rc"] == 0 and p["branch"] == SPLIT and p["msg"] == ""
