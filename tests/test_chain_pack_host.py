"""The packed E image of the fused chain step (csrc/chain_plan.h: e_image_unit, e_image_at, e_frag_lane, e_strip_lane,
chain_e_image, e_pack_bytes), checked by the host compiler alone: a short driver packs a core E[a][k][a'] of distinct values
as csrc/chain_pack.hip does -- unit U of slice k from e_image_unit -- and then reads it as phase B of chain_step_kernel
does.

For every (A, A2) of the list: the verdict of chain_fused_plan, and where chain_e_image has an image
  - the plan (where accepted) uses exactly chain_e_image's row length and unit count;
  - E[a][a'] sits at e_image_at(a, a') of its slice, for every a < A, a' < A2;
  - every fragment read of phase B -- lane (x16, kq), k-block kap, column tile nn or strip q -- that stands for a row a < A
    and a column a' < A2 finds exactly that element; a read for a row beyond A (the padding of the last k-block) finds row
    A - 1 of the same column (it meets an exact zero of T);
  - a unit whose row lies beyond A holds row A - 1, one whose second column would lie beyond A2 holds columns 0, 1
    (restated here with a division, not the kernel's reciprocal);
  - a slice is a whole number of 64-unit pieces and the last piece of the last slice ends where the allocation ends
    (every store of the driver's pack loop is bounds-checked).

A second driver does the same for the image chain_wide_kernel's loader gathers with e_image_unit_from: a chunk of rows from
a row origin on, and odd A2 (WIDE_CASES below)."""

import pytest

from tests.host_driver import compile_driver, run_driver

RANKS = ((100, 100), (50, 50), (52, 50), (112, 112), (16, 16), (18, 2), (4, 100))
# what chain_fused_plan says (force = 1, K1 = 32, J = 40): A2 = 2 is below the kernel's 4, A = 4 has no full tile
PLAN_VERDICT = (1, 1, 1, 1, 1, 0, 0)
HAS_IMAGE = (1, 1, 1, 1, 1, 0, 1)

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "chain_plan.h"
using namespace ttsk;

#define REQUIRE(c) do { if (!(c)) { printf("FAIL %s line %d (A=%d A2=%d)\n", #c, __LINE__, A, A2); return 1; } } while (0)

int main(int argc, char **argv)
{
    for (int i = 1; i + 1 < argc; i += 2) {
        const int A = atoi(argv[i]), A2 = atoi(argv[i + 1]), n = 3, K1 = 32, J = 40, nb = 2;
        const double *W[2] = {(const double *)0x30000000ull, (const double *)0x30100000ull};
        const double *X[2] = {(const double *)0x20000000ull, (const double *)0x20100000ull};
        double *Out[2] = {(double *)0x50000000ull, (double *)0x50100000ull};
        ChainStepArgs c{nb, n, K1, A, A2, J, W, A, X, (int64_t)n * K1, K1, 1, (int64_t)J * n * K1, (const double *)0x10000000ull, nullptr, Out};
        ChainFusedPlan p;
        const int rc = chain_fused_plan(c, 256, true, p);
        int A2P = 0, eunits = 0;
        const bool img_ok = chain_e_image(A, A2, A2P, eunits);
        long checked = 0;
        if (rc) REQUIRE(img_ok && p.a.A2P == A2P && p.a.eunits == eunits && p.a.Epk == nullptr);
        if (img_ok) {
            int nq, sq;
            chain_tile_split(A, nq, sq);
            int nn, sn;
            chain_tile_split(A2, nn, sn);
            const int KB2 = 4 * nq + sq;
            REQUIRE(A2P >= A2 && A2P % 2 == 0 && eunits % 64 == 0 && eunits >= 2 * KB2 * A2P && eunits - 2 * KB2 * A2P < 64 && eunits < (1 << 16));
            REQUIRE(e_pack_bytes(n, eunits) == (int64_t)n * eunits * 16);
            std::vector<double> E((size_t)A * n * A2), img((size_t)(e_pack_bytes(n, eunits) / 8), -1.0);
            for (size_t e = 0; e < E.size(); ++e) E[e] = (double)(e + 1);
            auto el = [&](int a, int k, int a2) { return E.at(((size_t)a * n + k) * A2 + a2); };
            // the pack kernel's loop (chain_pack.hip), every store bounds-checked; the loader's pieces: NI of 64 units
            const uint32_t inv = e_image_inv(A2P);
            const int NI = eunits >> 6;
            for (int k = 0; k < n; ++k)
                for (int m = 0; m < NI; ++m)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int U = 64 * m + lane;
                        const EUnit un = e_image_unit((uint32_t)U, inv, A, A2, A2P);
                        REQUIRE(un.row >= 0 && un.row < A && un.col >= 0 && un.col + 1 < A2);
                        img.at(((size_t)k * eunits + U) * 2) = el(un.row, k, un.col);
                        img.at(((size_t)k * eunits + U) * 2 + 1) = el(un.row, k, un.col + 1);
                        // restated with a division: rows beyond A repeat row A - 1, a last odd column maps to 0
                        const int sec = U / A2P, u = U % A2P, row = 2 * sec + (u & 1), col = 2 * (u >> 1);
                        REQUIRE(un.row == (row < A ? row : A - 1) && un.col == (col + 1 < A2 ? col : 0));
                        ++checked;
                    }
            REQUIRE(((size_t)(n - 1) * eunits + (size_t)(NI - 1) * 64 + 63) * 2 + 1 == img.size() - 1);   // the last store is the last element
            for (double v : img) REQUIRE(v >= 1.0);                                                       // nothing left unwritten
            for (int k = 0; k < n; ++k) {
                const double *sl = img.data() + (size_t)k * eunits * 2;
                for (int a = 0; a < A; ++a)
                    for (int a2 = 0; a2 < A2; ++a2, ++checked) REQUIRE(sl[e_image_at(a, a2, A2P)] == el(a, k, a2));
                // phase B of cf_piece: k-block kap of T meets rows 4 kap + kq of E_k
                for (int kap = 0; kap < KB2; ++kap)
                    for (int lane = 0; lane < 64; ++lane) {
                        const int x16 = lane & 15, kq = lane >> 4, a = 4 * kap + kq, ac = a < A ? a : A - 1;
                        for (int t = 0; t < nn; ++t) {
                            const int col = 16 * t + x16, pos = e_frag_lane(x16, kq, A2P) + kap * 4 * A2P + 32 * t;
                            if (col >= A2) continue;                    // a zero-padded column tile: never stored
                            REQUIRE(pos >= 0 && pos < 2 * eunits && sl[pos] == el(ac, k, col));
                            ++checked;
                        }
                        for (int q = 0; q < sn; ++q) {
                            const int es_col = 16 * nn + (x16 & 3), col = es_col + 4 * q;
                            const int pos = e_strip_lane(kq, A2P) + e_image_at(0, es_col, A2P) + kap * 4 * A2P + 8 * q;
                            if (col >= A2) continue;
                            REQUIRE(pos >= 0 && pos < 2 * eunits && sl[pos] == el(ac, k, col));
                            ++checked;
                        }
                        // cf_rows4 (a last row tile of at most 4 rows): block beta of tile pq meets row 16 pq + 4 beta + kq, column 4 c + n4
                        const int n4 = x16 & 3, beta = x16 >> 2;
                        for (int pq = 0; pq < nq; ++pq)
                            for (int cc = 0; cc < 4 * nn + sn; ++cc) {
                                const int r = 16 * pq + 4 * beta + kq, col = 4 * cc + n4, pos = e_image_at(4 * beta + kq, n4, A2P) + pq * 16 * A2P + 8 * cc;
                                if (kap || col >= A2) continue;
                                REQUIRE(pos < 2 * eunits && sl[pos] == el(r < A ? r : A - 1, k, col));
                                ++checked;
                            }
                        for (int q = 0; q < sq; ++q)
                            for (int cc = 0; cc < 4 * nn + sn; ++cc) {
                                const int r = 16 * nq + 4 * q + kq, col = 4 * cc + n4, pos = e_image_at(kq, n4, A2P) + (8 * nq + 2 * q) * 2 * A2P + 8 * cc;
                                if (kap || col >= A2) continue;
                                REQUIRE(pos < 2 * eunits && sl[pos] == el(r < A ? r : A - 1, k, col));
                                ++checked;
                            }
                    }
            }
        }
        printf("A=%d A2=%d plan=%d image=%d A2P=%d eunits=%d checked=%ld\n", A, A2, rc, (int)img_ok, A2P, eunits, checked);
    }
    return 0;
}
"""


# The loader of chain_wide_kernel (chain_stages.h: chain_e_fill_gather<true>) builds the image of a CHUNK of rows [a0, a0 + ac)
# of E_k with e_image_unit_from: a row origin, and for odd A2 the unit behind a row's last column reaching into the next
# slice -- in the last slice it holds columns 0, 1 instead and column A2 - 1 is patched in element by element.
# (A, A2, a0, ac); each with n = 1 (every slice is the last one) and n = 2 (an ordinary odd slice, then the last one).
WIDE_CASES = ((20, 7, 0, 20), (57, 21, 40, 20), (33, 10, 16, 24))

DRIVER_WIDE = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "chain_plan.h"
using namespace ttsk;

#define REQUIRE(c) do { if (!(c)) { printf("FAIL %s line %d (A=%d A2=%d a0=%d ac=%d n=%d)\n", #c, __LINE__, A, A2, a0, ac, n); return 1; } } while (0)

int main(int argc, char **argv)
{
    for (int i = 1; i + 4 < argc; i += 5) {
        const int A = atoi(argv[i]), A2 = atoi(argv[i + 1]), a0 = atoi(argv[i + 2]), ac = atoi(argv[i + 3]), n = atoi(argv[i + 4]);
        // the chunk structure chain_wide_plan picks for `ac` rows, its image and the output structure
        int ci = -1;
        for (int c = 0; c < 7 && ci < 0; ++c)
            if (16 * CW_NQ[c] + 4 * CW_SQ[c] >= (ac + 3) / 4 * 4) ci = c;
        REQUIRE(ci >= 0);
        const int nq = CW_NQ[ci], sq = CW_SQ[ci], AP = 16 * nq + 4 * sq, KB2 = 4 * nq + sq;
        const int A2P = A2 + (A2 & 1), eunits = (int)cdiv((int64_t)2 * (AP / 4) * A2P, 64) * 64, NI = eunits >> 6;
        int nn, sn;
        chain_tile_split(A2, nn, sn);
        const int cnt = A - a0 < ac ? A - a0 : ac;
        REQUIRE(a0 >= 0 && a0 < A && cnt >= 1 && AP >= cnt && eunits < (1 << 16));
        std::vector<double> E((size_t)A * n * A2);
        for (size_t e = 0; e < E.size(); ++e) E[e] = (double)(e + 1);
        auto el = [&](int a, int k, int a2) { return E.at(((size_t)a * n + k) * A2 + a2); };
        const uint32_t inv = e_image_inv(A2P);
        const int64_t rowstride = (int64_t)n * A2;
        long checked = 0, spilled = 0, patched = 0;
        for (int k = 0; k < n; ++k) {
            std::vector<double> img((size_t)eunits * 2, -1.0);
            const bool tail = (A2 & 1) && k == n - 1;
            // the loader's loop: unit U = 16 bytes from E_k + row rowstride + col, every read inside the core
            for (int m = 0; m < NI; ++m)
                for (int lane = 0; lane < 64; ++lane) {
                    const int U = 64 * m + lane;
                    const EUnit un = e_image_unit_from((uint32_t)U, inv, a0, A, A2, A2P, tail);
                    REQUIRE(un.row >= a0 && un.row < A && un.col >= 0 && un.col < A2 && (un.col & 1) == 0);
                    const size_t src = (size_t)k * A2 + (size_t)(un.row * rowstride) + un.col;
                    img.at((size_t)U * 2) = E.at(src);
                    img.at((size_t)U * 2 + 1) = E.at(src + 1);                      // odd A2, not the last slice: may be E_{k+1}[row][0]
                    if (un.col + 1 == A2) { REQUIRE((A2 & 1) && !tail); ++spilled; }
                    // restated with a division
                    const int sec = U / A2P, u = U % A2P, row = a0 + 2 * sec + (u & 1), col = 2 * (u >> 1);
                    REQUIRE(un.row == (row < A ? row : A - 1));
                    REQUIRE(un.col == ((col + 1 < A2 || ((A2 & 1) && !tail && col < A2)) ? col : 0));
                }
            if (tail)
                for (int lane = 0; lane < AP; ++lane, ++patched) {
                    const int row = a0 + lane < A ? a0 + lane : A - 1;
                    img.at(e_image_at(lane, A2 - 1, A2P)) = el(row, k, A2 - 1);
                }
            for (double v : img) REQUIRE(v >= 1.0);
            // phase B: k-block kap of the chunk's T meets rows a0 + 4 kap + kq of E_k (beyond the chunk: zeros of T meet
            // whatever finite row the image holds -- the next rows of E, clamped to A - 1)
            for (int kap = 0; kap < KB2; ++kap)
                for (int lane = 0; lane < 64; ++lane) {
                    const int x16 = lane & 15, kq = lane >> 4, a = 4 * kap + kq, row = a0 + a < A ? a0 + a : A - 1;
                    for (int t = 0; t < nn; ++t) {
                        const int col = 16 * t + x16, pos = e_frag_lane(x16, kq, A2P) + kap * 4 * A2P + 32 * t;
                        if (col >= A2) continue;                            // a zero-padded column tile: never stored
                        REQUIRE(pos >= 0 && pos < 2 * eunits && img[pos] == el(row, k, col));
                        ++checked;
                    }
                    for (int q = 0; q < sn; ++q) {
                        const int es_col = 16 * nn + (x16 & 3), col = es_col + 4 * q;
                        const int pos = e_strip_lane(kq, A2P) + e_image_at(0, es_col, A2P) + kap * 4 * A2P + 8 * q;
                        REQUIRE(pos >= 0 && pos < 2 * eunits);              // read even where the column is never stored
                        if (col >= A2) continue;
                        REQUIRE(img[pos] == el(row, k, col));
                        ++checked;
                    }
                }
            for (int a = 0; a < cnt; ++a)
                for (int a2 = 0; a2 < A2; ++a2, ++checked) REQUIRE(img[e_image_at(a, a2, A2P)] == el(a0 + a, k, a2));
        }
        printf("A=%d A2=%d a0=%d ac=%d n=%d cnt=%d AP=%d eunits=%d checked=%ld spilled=%ld patched=%ld\n", A, A2, a0, ac, n, cnt, AP,
               eunits, checked, spilled, patched);
    }
    return 0;
}
"""


def _run_driver(tmp_path_factory, name, text, args):
    exe = compile_driver(tmp_path_factory, name, text)
    out = run_driver(exe, args)
    print(out)
    return [dict(x.split("=") for x in line.split()) for line in out.splitlines()]


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    return _run_driver(tmp_path_factory, "chain_pack", DRIVER, [x for pair in RANKS for x in pair])


@pytest.fixture(scope="module")
def wide_report(tmp_path_factory):
    return _run_driver(tmp_path_factory, "chain_wide_image", DRIVER_WIDE, [x for c in WIDE_CASES for n in (1, 2) for x in c + (n,)])


def test_wide_loader_image_holds_what_phase_b_reads(wide_report):
    """every case ran, every element of the chunk and every fragment read was compared, and the two odd-A2 rules occurred
    where they must: the unit reaching into the next slice only in a slice that is not the last, the patch only in the last"""
    assert [tuple(int(r[k]) for k in ("A", "A2", "a0", "ac", "n")) for r in wide_report] == [c + (n,) for c in WIDE_CASES for n in (1, 2)]
    for r in wide_report:
        A2, n, cnt, AP = int(r["A2"]), int(r["n"]), int(r["cnt"]), int(r["AP"])
        assert int(r["checked"]) >= n * (cnt * A2 + AP * A2), r
        assert int(r["patched"]) == (AP if A2 & 1 else 0), r
        # one such unit per row of the image and slice that is not the last (the padding of the last 1 KB piece may add some)
        assert int(r["spilled"]) >= AP * (n - 1) if A2 & 1 else int(r["spilled"]) == 0, r
        assert n > 1 or int(r["spilled"]) == 0, r
    assert [int(r["cnt"]) for r in wide_report] == [20, 20, 17, 17, 17, 17]


def test_every_rank_pair_was_checked(report):
    assert [(int(r["A"]), int(r["A2"])) for r in report] == list(RANKS)
    assert tuple(int(r["plan"]) for r in report) == PLAN_VERDICT
    assert tuple(int(r["image"]) for r in report) == HAS_IMAGE


def test_phase_b_finds_every_element_in_the_packed_slice(report):
    for r, has in zip(report, HAS_IMAGE):
        A, A2 = int(r["A"]), int(r["A2"])
        if not has:
            assert int(r["checked"]) == 0
            continue
        # at least: every unit of three slices, every element of three slices, every fragment read of a full k-block
        assert int(r["checked"]) >= 3 * (int(r["eunits"]) + A * A2), r


def test_slices_are_whole_loader_pieces(report):
    for r, has in zip(report, HAS_IMAGE):
        if has:
            A, A2, eunits = int(r["A"]), int(r["A2"]), int(r["eunits"])
            nf, rem = divmod(A, 16)
            kb2 = 4 * nf + (0 if rem == 0 else 1 if rem <= 4 else 2 if rem <= 8 else 4)
            assert int(r["A2P"]) == A2 and eunits % 64 == 0 and 0 <= eunits - 2 * kb2 * A2 < 64, r


def test_headline_image_sizes(report):
    """rank 100: 80 KB per slice in LDS, 82 KB packed (the padding of the last k-block); n = 200 slices: 16.4 MB"""
    r = {(int(x["A"]), int(x["A2"])): int(x["eunits"]) for x in report}
    assert r[(100, 100)] == 5056 and 200 * r[(100, 100)] * 16 == 16179200
    assert r[(50, 50)] == 1344 and r[(52, 50)] == 1344
