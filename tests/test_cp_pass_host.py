"""The one-pass CP sketch kernels without a GPU: the NumPy restatement of ``ttsk_cp_chain_step`` / ``ttsk_cp_psi_omega``
(tests/cp_pass_ref.py) against np.longdouble and against today's ``contract`` compositions, the host-side plan of the two
entries (csrc/cp_pass_plan.h, plain C++) compiled with the host compiler -- once more under the address and undefined-
behaviour sanitizers, as a stand-alone program -- the oracle against the recorded runs of the reference
(tests/golden/cp_cases.npz), and the routing switch of ``cp_fused``."""
import os

import numpy as np
import pytest

from tests import cp_pass_ref as ref
from tests.host_driver import ROOT, compile_driver, run_driver

ERR_ARG, UNSUPPORTED = -2, -3


def _wide():
    if np.finfo(np.longdouble).eps >= np.finfo(np.float64).eps:
        pytest.fail("np.longdouble is no wider than float64 on this host: the bounds cannot be checked")


# ---- 1. the restatement
@pytest.mark.parametrize("case", ref.CHAIN_CASES, ids=lambda c: c.name)
def test_chain_restatement_against_longdouble_and_the_composition(case):
    _wide()
    a = ref.chain_arrays(case)
    L, V, D = a["L"], a["V"], a["D"]
    out, tol = ref.chain_step(L, V, D), ref.chain_bound(L, V, D)
    assert out.shape == (case.N, case.rho1) and (tol > 0).all()
    exact = ref.chain_step(L, V, D, dtype=np.longdouble)
    ratio = float(np.max(np.abs(out - exact) / (tol / 2)))              # against the undoubled, first-order bound
    print(f"{case.name}: float64 against longdouble at {ratio:.2f} of the first-order bound")
    assert ratio <= 1.0
    assert (np.abs(out - ref.chain_step_composed(L, V, D)) <= tol).all()
    assert (ref.chain_step(L, V, D, absolute=True) >= np.abs(out)).all()
    if case.v != "plain":
        assert not V.flags.c_contiguous
    if case.pad:
        assert np.isnan(a["L_base"][:, case.rho:]).all() and a["L_base"].shape[1] == case.rho + case.pad


@pytest.mark.parametrize("case", ref.PSI_CASES, ids=lambda c: c.name)
def test_psi_omega_restatement_against_longdouble_and_the_composition(case):
    _wide()
    a = ref.psi_arrays(case)
    L, R, V = a["L"], a["R"], a["V"]
    if case.n:
        P, tol = ref.psi(L, R, V), ref.psi_bound(L, R, V)
        assert P.shape == (case.l, case.n, case.r) and (tol > 0).all()
        exact = ref.psi(L, R, V, dtype=np.longdouble)
        ratio = float(np.max(np.abs(P - exact) / (tol / 2)))
        print(f"{case.name}: Psi, float64 against longdouble at {ratio:.2f} of the first-order bound")
        assert ratio <= 1.0
        assert (np.abs(P - ref.psi_composed(L, R, V)) <= tol).all()
    if case.omega is not None:
        Ro = a["R_om"] if case.omega else R
        O, tol = ref.omega(L, Ro, case.N), ref.omega_bound(L, Ro, case.N)
        assert O.shape == (case.l, case.omega or case.r)
        exact = ref.omega(L, Ro, case.N, dtype=np.longdouble)
        ratio = float(np.max(np.abs(O - exact) / (tol / 2)))
        print(f"{case.name}: Omega, float64 against longdouble at {ratio:.2f} of the first-order bound")
        assert ratio <= 1.0
        ones = np.ones((case.N, 1))
        assert (np.abs(O - ref.omega_composed(ones if L is None else L, ones if Ro is None else Ro)) <= tol).all()


def test_case_lists_reach_the_edges_they_name():
    ch, ps = ref.CHAIN_CASES, ref.PSI_CASES
    assert {1, 15, 16, 17, 33, ref.ROWS_PER_WORKGROUP - 1, ref.ROWS_PER_WORKGROUP, ref.ROWS_PER_WORKGROUP + 1,
            ref.SMALL_N - 1, ref.SMALL_N, ref.SMALL_N + 1} <= {c.N for c in ch}
    assert {1, 3, 16, 17} <= {c.rho for c in ch} and {1, 3, 4, 5, 33} <= {c.n for c in ch}
    assert {ref.ROW_CHUNK - 1, ref.ROW_CHUNK, ref.ROW_CHUNK + 1, 2 * ref.ROW_CHUNK, 2 * ref.ROW_CHUNK + 1} <= {c.rho * c.n for c in ch}
    assert {1, 15, 16, 17, 33, 128} <= {c.rho1 for c in ch}
    assert any(c.no_L for c in ch) and {"plain", "transposed", "slice"} == {c.v for c in ch} and any(c.pad for c in ch)
    for side in ("l", "r"):
        assert {1, 15, 16, 17, 33, 128} <= {getattr(c, side) for c in ps}
    assert {1, 3, 17} <= {c.n for c in ps}
    assert {1, 3, 4, 5, ref.N_CHUNK - 1, ref.N_CHUNK, ref.N_CHUNK + 1, 2 * ref.N_CHUNK + 1} <= {c.N for c in ps}
    assert any(c.no_L and not c.no_R for c in ps) and any(c.no_R and not c.no_L for c in ps) and any(c.no_L and c.no_R for c in ps)
    assert any(c.omega is None for c in ps) and any(c.omega == 0 for c in ps) and any(c.omega for c in ps)
    assert {ref.PSI_COLS - 1, ref.PSI_COLS, ref.PSI_COLS + 1} <= {c.n * c.r for c in ps}
    assert ref.PSI_COLS in {c.n * c.r + (c.omega or c.r) for c in ps if c.omega is not None}


# ---- 2. the host-side plan
# one request per line of standard input, one answer per line: the sanitized build reads the same lines
DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "cp_pass_plan.h"
using namespace ttsk;
int main()
{
    static double cell;
    char kind[16];
    long long v[12];
    printf("const %d %d %d %d %d %d %d %zu %d %d %d %d %zu %zu\n", CP_MAX_RANK, CP_WAVES, CP_ROW_TILES, CP_SMALL_N, CP_COL_TILES, CP_KC,
           CP_D_PITCH, CP_CHAIN_LDS, CP_PSI_COL_TILES, CP_PSI_COLS, CP_PSI_ROW_TILES, CP_N_CHUNK, sizeof(CpChainArgs), sizeof(CpPsiArgs));
    while (scanf("%15s", kind) == 1) {
        const int want = strcmp(kind, "chain") == 0 ? 9 : 12;
        for (int i = 0; i < want; ++i)
            if (scanf("%lld", &v[i]) != 1) return 2;
        if (want == 9) {          // flags ldl v_k v_j ldo N rho n rho1; flags: 1 no L, 2 no V, 4 no D, 8 no out
            const int f = (int)v[0];
            static CpChainPlan p;
            const int rc = cp_chain_plan(f & 1 ? nullptr : &cell, v[1], f & 2 ? nullptr : &cell, v[2], v[3], f & 4 ? nullptr : &cell,
                                         f & 8 ? nullptr : &cell, v[4], v[5], v[6], v[7], v[8], &p);
            if (rc) { printf("rc %d %s\n", rc, p.msg); continue; }
            printf("rc 0 %d %d %lld %zu %.17g %.17g %d %d %d %d\n", p.row_tiles, p.rows_per_block, (long long)p.blocks, p.lds, p.flops, p.bytes,
                   p.a.K, p.a.q4, p.a.r4, p.a.L ? 1 : 0);
        } else {                  // flags ldl ldr v_k v_j ld_om r_om N l n r _; flags: 1 no L, 2 no R, 4 no V, 8 no psi, 16 no omega, 32 own R_om
            const int f = (int)v[0];
            static CpPsiPlan p;
            const int rc = cp_psi_plan(f & 1 ? nullptr : &cell, v[1], f & 2 ? nullptr : &cell, v[2], f & 4 ? nullptr : &cell, v[3], v[4],
                                       f & 8 ? nullptr : &cell, f & 32 ? &cell : nullptr, v[5], v[6], f & 16 ? nullptr : &cell, v[7], v[8], v[9],
                                       v[10], &p);
            if (rc) { printf("rc %d %s\n", rc, p.msg); continue; }
            printf("rc 0 %lld %d %d %zu %lld %lld %lld %d %.17g %.17g %d\n", (long long)p.blocks, p.a.cblocks, p.a.chunks, p.ws_bytes,
                   (long long)p.reduce_blocks, (long long)p.a.cols, (long long)p.a.psi_cols, p.a.r_om, p.flops, p.bytes, p.a.Ro ? 1 : 0);
        }
    }
    return 0;
}
"""


def _compile(tmp_path_factory, name, extra):
    return compile_driver(tmp_path_factory, name, DRIVER, ["-g", *extra])


def _ask(exe, requests, env=None):
    """requests: ("chain", flags, ldl, v_k, v_j, ldo, N, rho, n, rho1) or ("psi", flags, ldl, ldr, v_k, v_j, ld_om, r_om, N, l, n, r)"""
    text = "\n".join(" ".join(str(x) for x in (q if q[0] == "chain" else q + (0,))) for q in requests) + "\n"
    stdout, stderr = run_driver(exe, stdin=text, env=env, with_stderr=True)
    assert stderr == "", stderr[-2000:]                                  # a sanitizer report goes there
    lines = stdout.splitlines()
    assert len(lines) == len(requests) + 1
    const = [int(x) for x in lines[0].split()[1:]]
    out = []
    for line in lines[1:]:
        w = line.split(None, 2)
        rc = int(w[1])
        if rc:
            out.append(dict(rc=rc, msg=w[2] if len(w) > 2 else ""))
        else:
            out.append(dict(rc=0, v=[float(x) if ("." in x or "e" in x) else int(x) for x in line.split()[2:]]))
    return const, out


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    exe = _compile(tmp_path_factory, "cp_pass_plan", [])
    return lambda requests: _ask(exe, requests)


def chain_request(c, flags=0):
    v_k, v_j = {"plain": (c.N, 1), "transposed": (1, c.n), "slice": (c.N + 5, 1)}[c.v]
    return ("chain", flags | (1 if c.no_L else 0), c.rho + c.pad, v_k, v_j, c.rho1 + c.pad, c.N, c.rho, c.n, c.rho1)


def psi_request(c, flags=0):
    v_k, v_j = {"plain": (c.N, 1), "transposed": (1, c.n), "slice": (c.N + 5, 1)}[c.v]
    f = flags | (1 if c.no_L else 0) | (2 if c.no_R else 0) | (12 if not c.n else 0) | (16 if c.omega is None else 0) | (32 if c.omega else 0)
    return ("psi", f, c.l + c.pad, c.r + c.pad, v_k, v_j, (c.omega or 0) + c.pad, c.omega or 0, c.N, c.l, c.n, c.r)


REFUSALS = [
    # (request, status, a word of the message)
    (("chain", 0, 4, 9, 1, 5, 9, 4, 3, 5), 0, ""),
    (("chain", 2, 4, 9, 1, 5, 9, 4, 3, 5), ERR_ARG, "NULL"),
    (("chain", 4, 4, 9, 1, 5, 9, 4, 3, 5), ERR_ARG, "NULL"),
    (("chain", 8, 4, 9, 1, 5, 9, 4, 3, 5), ERR_ARG, "NULL"),
    (("chain", 0, 4, 9, 1, 5, 0, 4, 3, 5), ERR_ARG, "N = 0"),
    (("chain", 0, 4, 9, 1, 5, 9, 0, 3, 5), ERR_ARG, "rho = 0"),
    (("chain", 0, 4, 9, 1, 5, 9, 4, 0, 5), ERR_ARG, "n = 0"),
    (("chain", 0, 4, 9, 1, 5, 9, 4, 3, 0), ERR_ARG, "rho' = 0"),
    (("chain", 1, 4, 9, 1, 5, 9, 4, 3, 5), ERR_ARG, "rho = 1"),                      # no L with rho = 4
    (("chain", 0, 3, 9, 1, 5, 9, 4, 3, 5), ERR_ARG, "leading dimension 3 of L"),
    (("chain", 0, 4, 9, 1, 4, 9, 4, 3, 5), ERR_ARG, "leading dimension 4 of out"),
    (("chain", 0, 129, 9, 1, 5, 9, 129, 3, 5), UNSUPPORTED, "rank 129"),
    (("chain", 0, 4, 9, 1, 129, 9, 4, 3, 129), UNSUPPORTED, "rank 129"),
    (("chain", 0, 128, 9, 1, 128, 9, 128, 3, 128), 0, ""),
    (("chain", 0, 4, 1, 1, 5, 2 ** 31, 4, 3, 5), UNSUPPORTED, "2^31"),
    (("chain", 0, 4, 1, 1, 5, 2 ** 31 - 1, 4, 3, 5), 0, ""),
    (("chain", 1, 0, 1, 1, 5, 9, 1, 2 ** 31, 5), UNSUPPORTED, "2^31"),
    (("chain", 1, 0, 1, 1, 5, 9, 1, 2 ** 31 - 65, 5), 0, ""),
    (("chain", 1, 0, 1, 1, 5, 9, 1, 2 ** 31 - 64, 5), UNSUPPORTED, "rho n"),
    (("chain", 0, 64, 1, 1, 5, 9, 64, 2 ** 25, 5), UNSUPPORTED, "rho n"),
    (("psi", 0, 4, 5, 9, 1, 0, 0, 9, 4, 3, 5), 0, ""),
    (("psi", 24, 4, 5, 9, 1, 0, 0, 9, 4, 3, 5), ERR_ARG, "NULL output"),
    (("psi", 4, 4, 5, 9, 1, 0, 0, 9, 4, 3, 5), ERR_ARG, "NULL factor"),
    (("psi", 0, 4, 5, 9, 1, 0, 0, 0, 4, 3, 5), ERR_ARG, "N = 0"),
    (("psi", 0, 4, 5, 9, 1, 0, 0, 9, 0, 3, 5), ERR_ARG, "l = 0"),
    (("psi", 0, 4, 5, 9, 1, 0, 0, 9, 4, 0, 5), ERR_ARG, "n = 0"),
    (("psi", 0, 4, 5, 9, 1, 0, 0, 9, 4, 3, 0), ERR_ARG, "r = 0"),
    (("psi", 1, 4, 5, 9, 1, 0, 0, 9, 4, 3, 5), ERR_ARG, "l = 1"),
    (("psi", 2, 4, 5, 9, 1, 0, 0, 9, 4, 3, 5), ERR_ARG, "r = 1"),
    (("psi", 0, 3, 5, 9, 1, 0, 0, 9, 4, 3, 5), ERR_ARG, "of L"),
    (("psi", 0, 4, 4, 9, 1, 0, 0, 9, 4, 3, 5), ERR_ARG, "of R"),
    (("psi", 32, 4, 5, 9, 1, 6, 0, 9, 4, 3, 5), ERR_ARG, "Omega's right operand"),
    (("psi", 32, 4, 5, 9, 1, 6, 7, 9, 4, 3, 5), ERR_ARG, "Omega's right operand"),
    (("psi", 32, 4, 5, 9, 1, 7, 7, 9, 4, 3, 5), 0, ""),
    (("psi", 48, 4, 5, 9, 1, 0, 0, 9, 4, 3, 5), 0, ""),                              # no omega: its operand is not looked at
    (("psi", 0, 129, 5, 9, 1, 0, 0, 9, 129, 3, 5), UNSUPPORTED, "rank 129"),
    (("psi", 0, 4, 129, 9, 1, 0, 0, 9, 4, 3, 129), UNSUPPORTED, "rank 129"),
    (("psi", 32, 4, 5, 9, 1, 129, 129, 9, 4, 3, 5), UNSUPPORTED, "rank 129"),
    (("psi", 0, 128, 128, 9, 1, 0, 0, 9, 128, 3, 128), 0, ""),
    (("psi", 0, 4, 5, 1, 1, 0, 0, 2 ** 31, 4, 3, 5), UNSUPPORTED, "2^31"),
    (("psi", 0, 4, 5, 1, 1, 0, 0, 9, 4, 2 ** 31, 5), UNSUPPORTED, "2^31"),
    (("psi", 0, 4, 5, 1, 1, 0, 0, 2 ** 31 - 1, 4, 3, 5), 0, ""),
    (("psi", 0, 4, 128, 1, 1, 0, 0, 9, 4, 2 ** 31 - 1, 128), UNSUPPORTED, "column blocks"),        # 2^31 column blocks
    (("psi", 0, 4, 128, 1, 1, 0, 0, 2 ** 20, 4, 2 ** 20, 128), UNSUPPORTED, "workgroups"),         # 2^20 blocks x 2^11 chunks
    (("psi", 12, 4, 5, 0, 0, 0, 0, 9, 4, 0, 5), 0, ""),                              # Omega alone: n is not read
]


def _check_const(const):
    (max_rank, waves, row_tiles, small_n, col_tiles, kc, pitch, chain_lds, psi_col_tiles, psi_cols, psi_row_tiles, n_chunk,
     chain_arg_bytes, psi_arg_bytes) = const
    assert (max_rank, small_n, 16 * row_tiles * waves, kc, pitch, chain_lds, psi_cols, n_chunk) == (
        ref.MAX_RANK, ref.SMALL_N, ref.ROWS_PER_WORKGROUP, ref.ROW_CHUNK, ref.D_PITCH, ref.CHAIN_LDS, ref.PSI_COLS, ref.N_CHUNK)
    assert small_n == 16 * waves and row_tiles > 1                      # more than one row tile per wave where N allows
    assert 16 * col_tiles == max_rank == 16 * psi_row_tiles and psi_cols == 16 * psi_col_tiles * waves
    # a staged row of D holds every column tile; the two rows that a half-wave's 64-bit LDS read touches are `pitch` doubles
    # apart: 16 modulo 32 puts their 2 x 32 dwords on 64 different banks
    assert pitch >= 16 * col_tiles and pitch % 32 == 16
    assert chain_lds == 2 * kc * pitch * 8 <= 160 * 1024 and 2 * chain_lds <= 160 * 1024      # two workgroups per compute unit
    assert kc % 4 == 0 and (kc * 16 * col_tiles) % (64 * waves) == 0    # whole k-blocks; the staging loop has no remainder
    assert chain_arg_bytes <= 4096 and psi_arg_bytes <= 4096


def _check_chain(case, p):
    assert p["rc"] == 0, p
    row_tiles, rows, blocks, lds, flops, nbytes, K, q4, r4, has_L = p["v"]
    print(f"{case.name}: grid {blocks} x 256 threads, {row_tiles} row tile(s) per wave, {rows} rows per workgroup, LDS {lds} B, "
          f"K = {K} in {-(-K // ref.ROW_CHUNK)} stage(s), flops {flops:.0f}, bytes {nbytes:.0f}")
    assert row_tiles == (2 if case.N > ref.SMALL_N else 1) and rows == 64 * row_tiles
    assert lds == ref.CHAIN_LDS <= 160 * 1024
    # every 16-row tile of out exactly once: workgroup b, wave w, tile t owns rows 16 (b 4 row_tiles + w row_tiles + t)
    tiles = [b * 4 * row_tiles + w * row_tiles + t for b in range(blocks) for w in range(4) for t in range(row_tiles)]
    need = -(-case.N // 16)
    assert sorted(tiles) == list(range(len(tiles))) and len(tiles) >= need and (blocks - 1) * rows < case.N
    assert K == case.rho * case.n and 4 == q4 * case.n + r4 and 0 <= r4 < case.n
    assert has_L == (0 if case.no_L else 1)
    assert flops == 2.0 * case.N * K * case.rho1
    assert nbytes == 8.0 * (case.N * (0 if case.no_L else case.rho) + case.N * case.n + K * case.rho1 + case.N * case.rho1)


def _check_psi(case, p):
    assert p["rc"] == 0, p
    blocks, cblocks, chunks, ws_bytes, reduce_blocks, cols, psi_cols, r_om, flops, nbytes, has_ro = p["v"]
    print(f"{case.name}: grid {blocks} = {cblocks} column block(s) x {chunks} chunk(s), no LDS, workspace {ws_bytes} B, "
          f"closing grid {reduce_blocks}, columns {psi_cols} + {r_om}, flops {flops:.0f}, bytes {nbytes:.0f}")
    want_om = 0 if case.omega is None else (case.omega or case.r)
    assert psi_cols == case.n * case.r and r_om == want_om and cols == psi_cols + want_om
    # every column once: block cb covers [128 cb, 128 cb + 128), the last one reaches past the end and none starts there
    assert (cblocks - 1) * ref.PSI_COLS < cols <= cblocks * ref.PSI_COLS
    # every term of the sum over N in exactly one chunk
    edges = [(c * ref.N_CHUNK, min((c + 1) * ref.N_CHUNK, case.N)) for c in range(chunks)]
    assert edges[0][0] == 0 and edges[-1][1] == case.N and all(a < b for a, b in edges)
    assert all(e0[1] == e1[0] for e0, e1 in zip(edges, edges[1:]))
    assert blocks == cblocks * chunks
    assert -(-case.l // 16) <= ref.MAX_RANK // 16                       # the row tiles one wave accumulates
    if chunks == 1:
        assert ws_bytes == 0 and reduce_blocks == 0                     # the one launch writes the outputs itself
    else:
        assert ws_bytes == 8 * chunks * case.l * cols and reduce_blocks == -(-(case.l * cols) // 256)
    assert flops == 2.0 * case.l * case.N * cols
    assert has_ro == (1 if case.omega is not None and (case.omega or not case.no_R) else 0)


def test_plan_constants_are_the_ones_the_restatement_mirrors(plan):
    const, _ = plan([chain_request(ref.CHAIN_CASES[0])])
    _check_const(const)


def test_plan_of_every_case(plan):
    _, res = plan([chain_request(c) for c in ref.CHAIN_CASES] + [psi_request(c) for c in ref.PSI_CASES])
    for c, p in zip(ref.CHAIN_CASES, res):
        _check_chain(c, p)
    for c, p in zip(ref.PSI_CASES, res[len(ref.CHAIN_CASES):]):
        _check_psi(c, p)


def test_plan_at_the_shapes_of_the_reference_experiments(plan):
    """forest: d = 8, n = 12, N = 25 000, l = 50, r = 100; plot_cp_tensor: d = 5, n = 10, N = 100, l = 30, r = 60"""
    forest_chain = ref.ChainCase("forest_chain", 25000, 50, 12, 50)
    forest_psi = ref.PsiCase("forest_psi", 25000, 50, 12, 100, omega=100)
    small_chain = ref.ChainCase("cp_tensor_chain", 100, 30, 10, 30)
    small_psi = ref.PsiCase("cp_tensor_psi", 100, 30, 10, 60, omega=60)
    _, res = plan([chain_request(forest_chain), psi_request(forest_psi), chain_request(small_chain), psi_request(small_psi)])
    _check_chain(forest_chain, res[0])
    _check_psi(forest_psi, res[1])
    _check_chain(small_chain, res[2])
    _check_psi(small_psi, res[3])
    assert res[0]["v"][2] == 196 and res[1]["v"][:3] == [11 * 49, 11, 49] and res[1]["v"][3] == 8 * 49 * 50 * 1300
    assert res[2]["v"][2] == 1 and res[3]["v"][:5] == [6, 6, 1, 0, 0]


def test_plan_argument_errors_and_refusals(plan):
    _, res = plan([q for q, _, _ in REFUSALS])
    for (q, status, word), p in zip(REFUSALS, res):
        assert p["rc"] == status, (q, p)
        if status:
            assert word in p["msg"] and p["msg"].startswith("ttsk_cp_"), (q, p)


def test_plan_under_the_address_and_undefined_behaviour_sanitizers(tmp_path_factory):
    """The stand-alone driver again, built with -fsanitize=address,undefined: every case and every refusal, the same answers,
    nothing on standard error."""
    # the sanitizer runtime linked into the program itself: it needs nothing from the environment it is started in
    exe = _compile(tmp_path_factory, "cp_pass_plan_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                                                          "-static-libasan", "-static-libubsan"])
    plain = _compile(tmp_path_factory, "cp_pass_plan_plain", [])
    requests = [chain_request(c) for c in ref.CHAIN_CASES] + [psi_request(c) for c in ref.PSI_CASES] + [q for q, _, _ in REFUSALS]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    assert _ask(exe, requests, env=env) == _ask(plain, requests)


# ---- 3. the oracle against the recorded runs of the reference
def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "cp_cases.npz"))


@pytest.mark.parametrize("method", ["streaming", "orthogonal", "hmt"])
def test_oracle_matches_the_recorded_reference_runs(method):
    from oracle import ttsk_oracle as orc
    z = _golden()
    d = int(z["d"])
    factors = [z[f"factor{k}"] for k in range(d)]
    shape = tuple(f.shape[0] for f in factors)
    right = orc.TTDrm([z[f"right_core{k}"] for k in range(d - 1)], shape, True)
    left = None if method == "hmt" else orc.TTDrm([z[f"left_core{k}"] for k in range(d - 1)], shape, False)
    assert right.rank[::-1] == tuple(z["right_rank"]) and (left is None or left.rank == tuple(z["left_rank"]))
    Psis, Omegas = orc.general_sketch("cp", factors, left, right, method)
    for k, P in enumerate(Psis):
        want = z[f"{method}_psi{k}"]
        assert P.shape == want.shape and np.linalg.norm(P - want) <= 1e-11 * np.linalg.norm(want), (method, k)
    n_om = 0 if method == "hmt" else d - 1
    assert len(Omegas) == n_om
    for k, O in enumerate(Omegas):
        want = z[f"{method}_omega{k}"]
        assert np.linalg.norm(O - want) <= 1e-11 * np.linalg.norm(want), (method, k)


# ---- 4. the routing switch
class _Reached(Exception):
    """the call got as far as this"""


def _reach(name):
    def stop(*args, **kwargs):
        raise _Reached(name)
    return stop


def test_route_switch_of_cp_fused():
    """no device behind it: what the switch does before any call"""
    from tt_sketch_amd import cp_fused, paths
    assert cp_fused.forced is paths.forced and paths.ROUTES == (None, "kernel", "composed")
    assert paths._forced is None
    with cp_fused.forced("composed"):
        assert paths.resolve(None) == "composed" and paths.resolve("kernel") == "kernel"
        assert cp_fused.chain_step(None, None, None) is None and cp_fused.psi_omega(None, None, None) is None
        with cp_fused.forced("kernel"):
            assert paths.resolve(None) == "kernel"
        assert paths._forced == "composed"
    assert paths._forced is None
    with pytest.raises(ValueError):
        paths.resolve("fastest")
    with pytest.raises(ValueError):
        with cp_fused.forced("fastest"):
            pass
    assert paths._forced is None
    assert cp_fused.try_cp_sketch(object(), None, None, None, route="composed") is None
    # a route that is set is taken, None is the cost rule: the composition only where it is expected to be strictly faster
    assert paths.taken("kernel", 2.0, 1.0) == "kernel" and paths.taken("composed", 1.0, 2.0) == "composed"
    assert paths.taken(None, 2.0, 1.0) == "composed" and paths.taken(None, 1.0, 2.0) == "kernel" and paths.taken(None, 1.0, 1.0) == "kernel"


def test_route_switch_through_op_apply(monkeypatch):
    """the keyword, the context, their nesting and the rejection of an unknown route, all before any device call"""
    import types
    from tt_sketch_amd import _native as nat, operator_product as opm, paths
    from tt_sketch_amd.device import DevArray, c_strides
    fake = lambda *shape: DevArray(types.SimpleNamespace(ptr=4096), 0, shape, c_strides(shape))      # never dereferenced
    L, M, C = fake(2, 3, 4), fake(2, 5, 6, 2), fake(3, 5, 3)
    monkeypatch.setattr(opm, "_composed", _reach("composed"))
    monkeypatch.setattr(nat, "call", lambda name, *a: _reach(name)())
    run = lambda **kw: opm.op_apply([L], [M], [C], **kw)
    with pytest.raises(ValueError, match="'kernel', 'composed' or None"):
        opm.op_apply(None, None, None, route="fastest")
    with pytest.raises(_Reached, match="composed"):
        run(route="composed")
    with pytest.raises(_Reached, match="ttsk_"):
        run(route="kernel")
    with paths.forced("composed"):
        with pytest.raises(_Reached, match="composed"):
            run()
        with pytest.raises(_Reached, match="ttsk_"):
            run(route="kernel")                     # the keyword goes before the context
        with paths.forced("kernel"):
            with pytest.raises(_Reached, match="ttsk_"):
                run()
        with pytest.raises(_Reached, match="composed"):
            run()
        with pytest.raises(ValueError, match="'kernel', 'composed' or None"):
            run(route="fastest")
    assert paths.resolve(None) is None
    with pytest.raises(_Reached, match="composed"):          # the rule again: one small term is composed
        run()


def test_route_switch_through_tt_gram(monkeypatch):
    from tt_sketch_amd import TensorTrain, _native as nat, paths, tensor_gram as tmod, tt_gram
    tts = [TensorTrain([np.ones((1, 3, 2)), np.ones((2, 4, 1))]) for _ in range(2)]
    monkeypatch.setattr(tmod, "_gram_composed", _reach("composed"))
    monkeypatch.setattr(nat, "call", lambda name, *a: _reach(name)())
    with pytest.raises(ValueError, match="'kernel', 'composed' or None"):
        tt_gram([], route="fastest")                # before the lists are looked at
    with pytest.raises(_Reached, match="composed"):
        tt_gram(tts, route="composed")
    with pytest.raises(_Reached, match="ttsk_"):
        tt_gram(tts, route="kernel")
    with paths.forced("composed"):
        with pytest.raises(_Reached, match="composed"):
            tt_gram(tts)
        with pytest.raises(_Reached, match="ttsk_"):
            tt_gram(tts, route="kernel")
        with paths.forced("kernel"):
            with pytest.raises(_Reached, match="ttsk_"):
                tt_gram(tts, tts)
        with pytest.raises(_Reached, match="composed"):
            tt_gram(tts, tts)
    assert paths.resolve(None) is None
    with pytest.raises(_Reached, match="ttsk_"):    # None: the rule is asked once the cores are on the device
        tt_gram(tts)


def test_general_sketch_asks_the_fused_paths_in_order(monkeypatch):
    """TT streaming, sparse one-pass, operator product, CP: the first that returns a pair wins, and only when all four
    decline does the generic driver run"""
    from tt_sketch_amd import cp_fused, operator_fused, sketch_dispatch as sd, sparse_fused, tt_fused
    assert sd.FUSED_PATHS == (tt_fused.try_stream_sketch, sparse_fused.try_sparse_gauss_sketch,
                              operator_fused.try_operator_sketch, cp_fused.try_cp_sketch)
    args = (object(), object(), object(), sd.SketchMethod.streaming)
    pair = ([np.ones((1, 2, 1))], [])
    for winner in range(5):
        asked = []

        def recorder(k):
            def path(*a):
                assert all(x is y for x, y in zip(a, args)) and len(a) == 4
                asked.append(k)
                return pair if k == winner else None
            return path
        monkeypatch.setattr(sd, "FUSED_PATHS", tuple(recorder(k) for k in range(4)))
        monkeypatch.setattr(sd, "general_sketch_device", lambda *a: asked.append("generic") or pair)
        out = sd.general_sketch(*args)
        assert asked == (list(range(winner + 1)) if winner < 4 else [0, 1, 2, 3, "generic"])
        assert type(out) is sd.SketchContainer and len(out.Psi_cores) == 1


# ---- 5. the routing rule of the chain step
MEASURED_CHAIN = [
    # N, rho = rho', n, the faster path as measured (profiles/cp_sketch_bench.json)
    (25000, 50, 12, "kernel"), (25000, 100, 12, "kernel"), (100, 30, 10, "composed"), (100, 60, 10, "composed"),
]


@pytest.mark.parametrize("N,rho,n,winner", MEASURED_CHAIN)
def test_chain_routing_rule_picks_the_measured_winner(N, rho, n, winner):
    from tt_sketch_amd import cp_fused
    kernel_ms, composed_ms = cp_fused.chain_route_ms(N, rho, n, rho)
    print(f"N = {N}, rho = {rho}, n = {n}: the rule expects {kernel_ms:.3f} ms of the kernel, {composed_ms:.3f} ms of the composition")
    assert ("composed" if composed_ms < kernel_ms else "kernel") == winner
