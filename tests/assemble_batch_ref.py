"""Cases, guarded operands, truth and checks for ttsk_tt_assemble_batch (csrc/assemble_batch.hip, behind to_tt_batch).
Plain module, no GPU: tests/test_assemble_batch_cover.py runs the table through the host plan (csrc/assemble_batch_plan.h)
and tests the checker on seeded defects, tests/test_gpu_assemble_batch_edges.py runs every case on the device.

A case is ONE call of the C entry point: (count, d, n, lr, rr, direction) and a layout of its operands.  Per pair (tensor b,
mode k) the call computes P = pinv(Omega) (r x l, into `work`) and the refined product
    right:  C = X P,  R = X - C Omega,  C += R P        X = Psi_k unfolded (m x r), m = l_{k-1} n_k
    left:   C = P X,  R = X - Omega C,  C += P R        X = Psi_{k+1} unfolded (l x m), m = n_{k+1} r_{k+1}
Everything below works on the NORMALISED pair: Xn (m x a), Pn (a x b), On (b x a), Cn (m x b) with Cn = Xn Pn refined --
the right form as it is, the left form transposed (Xn = X^T, Pn = P^T, On = Omega^T, Cn = C^T).  a, b are the kernel's.

Layout.  Every kind of operand (psi, om, c, work) of every core / mode has an arena of its own; tensor b's matrix lies in
slot `slots[kind][b]` of it, the slots `pitch` apart: PRE guard words, the matrix, POST guard words, `pad[kind]` more.  All
guards are the sentinel -1/3 (finite, no dyadic number), and so are C and `work` before a call.  The slots are what make
the groups of the plan: [0, 1, 2, 4] is a group of 3 and a group of 1, a descending list gives negative strides, a slot
used twice for `om` is an Omega shared by two tensors (stride 0).  The copied core always aliases its Psi.

Passes of a case.
  integer   Omega = D S (l <= r) or S D: S selects min(l, r) distinct columns (rows) with signs, D = diag(2^e), e in
            {-1, 0, 1} -- diag(R) spread 1/4, inside CHOL_GATE.  X integers in -8 .. 8.  Then G = D^2, P = Omega^T D^-2 is
            dyadic, X P has one term per element, R is an integer matrix, R P is exactly 0: on the covered path P read
            back from `work` and C must EQUAL the truth bit for bit.  On the fallback path (ttsk_pinv, ttsk_gemm) the
            integer pass is held to the two bounded rules below.
  gaussian  Omega with singular values 1 .. 1 / 10 (solve_ref.prescribed; one singular value where min(l, r) = 1), X N(0, 1).
            P: the one rule of tests/test_gpu_solve_edges.py, col_err(P, pinv_full(Omega)) <= 32 kappa e_lapack with
            e_lapack = col_err(numpy's pinv, pinv_full) floored at 4 eps.
            C: with P AS READ BACK, T = C1 + (Xn - C1 On) Pn, C1 = Xn Pn in long double, and per element
                |C - T| <= C_BOUND (2 a + b + 5) 2^-53 B,    B = (|Xn| + A |On|) |Pn| + A,   A = |Xn| |Pn|.
            Derivation: the device rounds three products, C1' = C1 + d1 (a terms), R' = Xn - C1' On + d2 (b + 1 terms),
            C' = C1' + R' Pn + d3 (a + 1 terms), so C' - T = d1 (I - On Pn) + d2 Pn + d3 and, with gamma_k = k u / (1 - k u),
            |d1| <= gamma_a A, |d2| <= gamma_{b+1} (|Xn| + |C1'| |On|), |d3| <= gamma_{a+1} (|C1'| + |R'| |Pn|), |C1'| <=
            (1 + gamma_a) A: every term of B collects at most gamma_a + gamma_{b+1} + gamma_{a+1} ~ (2 a + b + 2) u.  The
            + 3 and C_BOUND = 2 are those of tests/dense_pass_ref.py (second-order terms, an MFMA's own order of its
            four products).  A is the magnitude product, not |C1|: only that is an a-priori bound.  The fallback's three
            ttsk_gemm calls round the same three sums.
  refine    (cases tagged so, in place of gaussian) Omega with kappa = 100.  Truth Xn pinv_full(On) in long double; bar
            col_err(C, truth) <= 8 e_lapack, e_lapack = col_err(Xn numpy.pinv(On), truth).  The float64 restatement of
            the kernel (Cholesky normal equations, then the three products) sits at 0.15 - 1.3 e_lapack per pair, the
            unrefined first product at 26 - 195 for the worst pair of a group of 3 and 7.8 - 43 for its best (host, seeds
            1, 2, 3, 11; tests/test_assemble_batch_cover.py holds both sides: every pair of the restatement within 2, one
            pair of the unrefined beyond 16).
  robust    (the case tagged so) a group of 4: tensor 1 has an Omega of exact rank k < min(l, r) (solve_ref.int_factors,
            truth pinv_rank_k), tensor 2 one with kappa = 1e6 (truth: Newton-Schulz in long double to 2^-40; its noise
            0.2 kappa 2^-63 = 2e-14 lies four digits below e_lapack).  Both are rejected by the Cholesky gate and must come
            out of the Jacobi kernel at the stable bar 32 e_lapack; the normal equations would miss it by a factor kappa.

Poison.  Before every call the GPU test runs POISON through the same entry point: at least as many pairs and as many
doubles in every staging region as any case, every region written in full (no padding: the cover test shows it), its
operands scaled by 2^300 -- Os then holds 2^300, Gm 2^600, Rinv / Ginv / Ps 2^-300 .. 2^-600: a stale read is off by
hundreds of binary orders.
"""
from collections import namedtuple

import numpy as np

from tests import solve_ref as sr
from tests.edge_kit import C_BOUND, SENT, SENT_F, assert_guards, assert_untouched  # noqa: F401

LD, EPS = sr.LD, sr.EPS
MARGIN = 32.0                # the one rule of tests/test_gpu_solve_edges.py
REFINE_MARGIN = 8.0
KAPPA, KAPPA_REFINE, KAPPA_ILL = 10, 100, 10 ** 6
INT_KAPPA = 4                # integer pass: the singular values of D S are 1/2, 1, 2
PRE = POST = 16
TM, TILES_PER_WG, MAXG, COVER_MIN, COVER_MAX = 32, 16, 16, 56, 112      # the cover test holds them against the header
CHOL_GATE = 1.0 / 300.0
POISON_SCALE = 2.0 ** 300
KINDS = ("psi", "om", "c", "work")

Case = namedtuple("Case", "id count d n lr rr direction layout opts")


# ------------------------------------------------------------------------------------------------ the table
def _both(id, count, d, n, lr, rr, layout=None, swap=True, **opts):
    """the case in both directions; d = 2 cases give n as (m, other): m is the extent that makes the rows"""
    out = []
    for direction in (0, 1):
        nn = list(n)
        if d == 2 and swap and direction == 1:
            nn = nn[::-1]
        out.append(Case("%s-%s" % (id, "RL"[direction]), count, d, tuple(nn), tuple(lr), tuple(rr), direction, layout or {}, opts))
    return out


PAD_SHAPES = [(1, 1), (1, 3), (3, 1), (3, 5), (4, 16), (15, 17), (16, 16), (17, 33), (33, 17),
              (56, 56), (56, 112), (112, 56), (55, 110), (1, 112), (112, 1)]
ROWS = [1, 31, 32, 33, 511, 512]
CHUNKED = [513, 1025]
OUTSIDE = [(57, 57), (57, 112), (56, 113)]


def cases():
    c = []
    # padding of a and b: one full and one one-row tile, two tensors
    for l, r in PAD_SHAPES:
        c += _both("pad-%dx%d" % (l, r), 2, 2, (33, 3), [l], [r])
    # rows: one chunk up to 512 rows (16 tiles) ...
    for m in ROWS:
        c += _both("rows-%d" % m, 2, 2, (m, 2), [17], [33])
    # ... 2 chunks at 513 (17 tiles), 3 at 1025 (33 tiles, the last of one row), narrow and wide
    for m in CHUNKED:
        c += _both("rows-%d-narrow" % m, 2, 2, (m, 2), [3], [5])
        c += _both("rows-%d-wide" % m, 2, 2, (m, 2), [56], [112])
        c += _both("rows-%d-tall" % m, 2, 2, (m, 2), [112], [56])
    # groups
    c += _both("g-d18", 2, 18, (2,) * 18, [3] * 17, [3] * 17)                          # 17 groups: two launches
    c += _both("g-three-m", 3, 4, (5, 40, 7, 3), [3] * 3, [5] * 3)                     # three m in one table
    c += _both("g-3+1", 4, 2, (33, 3), [5], [9], {"slots": {k: [0, 1, 2, 4] for k in KINDS}})
    c += _both("g-descending", 3, 2, (40, 3), [5], [9], {"slots": {k: [2, 1, 0] for k in KINDS}})
    c += _both("g-shared-omega", 2, 2, (40, 3), [5], [9], {"slots": {"om": [0, 0]}})
    c += _both("g-count33", 33, 2, (33, 3), [3], [5])
    c += _both("g-count1", 1, 2, (33, 3), [3], [5])
    c += _both("g-spacings", 3, 2, (40, 3), [5], [9], {"pad": {"psi": 7, "om": 1, "c": 24, "work": 3}})
    c += _both("g-psi-breaks", 3, 2, (40, 3), [5], [9], {"slots": {"psi": [0, 1, 3]}})   # one operand alone off the spacing
    # shapes in one call: the later one in the (l, r) order needs more staging; one covered and one fallback
    c += _both("s-two-covered", 2, 3, (9, 7, 5), [3, 5], [5, 40])
    c += _both("s-covered+fallback", 2, 3, (9, 4, 5), [3, 57], [5, 57])
    # just outside the cover
    for l, r in OUTSIDE:
        c += _both("out-%dx%d" % (l, r), 2, 2, (33, 3), [l], [r])
    # the robust path inside a group of 4
    c += _both("robust", 4, 2, (40, 3), [12], [20], robust=5)
    c += _both("robust-tall", 4, 2, (40, 3), [20], [12], robust=5)
    # refinement: kappa = 100, where Omega' has full row rank (right: l <= r, left: l >= r), and at the C3 shape
    c += [x for x in _both("refine-13x29", 3, 2, (40, 3), [13], [29], refine=1) if x.direction == 0]
    c += [x for x in _both("refine-29x13", 3, 2, (40, 3), [29], [13], refine=1) if x.direction == 1]
    c += _both("refine-50x100", 3, 2, (40, 3), [50], [100], refine=1)
    return c


def by_id(id):
    return next(c for c in cases() if c.id == id)


# at least as large as any case in every staging region, every region without padding (34 * 56 * 112 and 34 * 56 * 56 are
# multiples of 32)
POISON = Case("poison", 34, 2, (4, 4), (56,), (112,), 0, {}, {})

# argument errors: (id, what changes in a good d = 2 call); nothing may be written
ARG_ERRORS = ["count0", "null-psi", "null-omega", "direction2", "d1", "d65", "zero-rank", "null-work"]

BRANCHES = {"path": "covered fallback", "side": "le gt", "chunks": "1 2 3", "groups": "1 >1 >16", "strides": "- 0 +",
            "nbc": "1 7", "nba": "1 7", "npre": "2 14", "last": "partial full"}


# ------------------------------------------------------------------------------------------------ shapes and layout
def core_shape(c, j):
    """Psi_j: (l_{j-1}, n_j, r_j)"""
    return (c.lr[j - 1] if j else 1, c.n[j], c.rr[j] if j < c.d - 1 else 1)


def out_core_shape(c, j):
    if c.direction == 0:
        return (c.lr[j - 1] if j else 1, c.n[j], c.lr[j])
    return (c.rr[j - 1], c.n[j], c.rr[j] if j < c.d - 1 else 1)


def pair_list(c):
    """the entry point's pairs, mode-major: (k, b, psi core, m)"""
    out = []
    for k in range(c.d - 1):
        for b in range(c.count):
            if c.direction == 0:
                out.append((k, b, k, (c.lr[k - 1] if k else 1) * c.n[k]))
            else:
                out.append((k, b, k + 1, c.n[k + 1] * (c.rr[k + 1] if k + 1 < c.d - 1 else 1)))
    return out


def arena_names(c):
    """name -> (kind, elements of one matrix)"""
    a = {}
    for j in range(c.d):
        a["psi%d" % j] = ("psi", int(np.prod(core_shape(c, j))))
    for k in range(c.d - 1):
        a["om%d" % k] = ("om", c.lr[k] * c.rr[k])
        a["work%d" % k] = ("work", c.lr[k] * c.rr[k])
        j = k if c.direction == 0 else k + 1
        a["c%d" % j] = ("c", int(np.prod(out_core_shape(c, j))))
    return a


OUT_KINDS = ("c", "work")


def slots_of(c, kind):
    return list(c.layout.get("slots", {}).get(kind, range(c.count)))


def pitch_of(c, name):
    kind, size = arena_names(c)[name]
    return PRE + size + POST + c.layout.get("pad", {}).get(kind, 0)


def place(c, name, b):
    """(first element, elements) of tensor b's matrix in its arena"""
    kind, size = arena_names(c)[name]
    return slots_of(c, kind)[b] * pitch_of(c, name) + PRE, size


def arena_size(c, name):
    kind, _ = arena_names(c)[name]
    return (max(slots_of(c, kind)) + 1) * pitch_of(c, name)


def pair_arenas(c, k, j):
    return "psi%d" % j, "om%d" % k, "c%d" % j, "work%d" % k


def plan_input(c):
    """what the host driver reads: per Omega shape, in the (l, r) order of the entry point's map, its pairs with element
    offsets (arena a starts at a 2^36: arenas are separate allocations)"""
    base = {name: i << 36 for i, name in enumerate(sorted(arena_names(c)))}
    shapes = {}
    for k, b, j, m in pair_list(c):
        offs = [base[a] + place(c, a, b)[0] for a in pair_arenas(c, k, j)]
        shapes.setdefault((c.lr[k], c.rr[k]), []).append((k, m) + tuple(offs))
    text = "case %s %d %d\n" % (c.id, c.direction, len(shapes))
    for (l, r) in sorted(shapes):
        text += "shape %d %d %d\n" % (l, r, len(shapes[(l, r)]))
        text += "".join("%d %d %d %d %d %d\n" % p for p in shapes[(l, r)])
    return text


def covered(l, r):
    return min(l, r) <= COVER_MIN and max(l, r) <= COVER_MAX


def tags_of_plan(c, shapes):
    """a case's plan (the parsed output of the driver: a list of shapes) as its tag string"""
    out = []
    for s in shapes:
        l, r = s["l"], s["r"]
        t = "path=%s side=%s" % ("covered" if s["covered"] else "fallback", "le" if l <= r else "gt")
        if s["covered"]:
            signs = set()
            for g in s["groups"]:
                if g["count"] > 1:
                    signs |= {"-0+"[(v > 0) - (v < 0) + 1] for v in (g["s_psi"], g["s_om"], g["s_c"], g["s_work"])}
            ng = len(s["groups"])
            chunks = sorted({ch for la in s["apply"] for ch in la["chunks"]})
            last = sorted({"full" if g["m"] % TM == 0 else "partial" for g in s["groups"]})
            a16, b16 = (s["a"] + 15) // 16, (s["b"] + 15) // 16
            t += " chunks=%s groups=%s launches=%d strides=%s nbc=%d nba=%d npre=%d last=%s" % (
                "+".join(map(str, chunks)), "1" if ng == 1 else ">1" if ng <= MAXG else ">16", len(s["apply"]),
                "".join(x for x in "-0+" if x in signs) or ".", b16, a16, 2 * a16, "+".join(last))
        out.append(t)
    return " | ".join(out)


def _p(side, nbc, nba, last="partial", chunks="1", groups="1", launches=1, strides="+"):
    return "path=covered side=%s chunks=%s groups=%s launches=%d strides=%s nbc=%d nba=%d npre=%d last=%s" % (
        side, chunks, groups, launches, strides, nbc, nba, 2 * nba, last)


def _fb(side):
    return "path=fallback side=%s" % side


def _ab(l, r, direction):
    """(nbc, nba): 16-column blocks of C (b) and of the Psi tile (a)"""
    a, b = (r, l) if direction == 0 else (l, r)
    return (b + 15) // 16, (a + 15) // 16


def _tags():
    """What each case is meant to reach, written from the kernel's rules (not from the plan): the cover test compares this
    with what assemble_batch_plan.h decides."""
    t = {}
    side = lambda l, r: "le" if l <= r else "gt"
    for dr, D in enumerate("RL"):
        for l, r in PAD_SHAPES:
            t["pad-%dx%d-%s" % (l, r, D)] = _p(side(l, r), *_ab(l, r, dr))
        for m in ROWS:
            t["rows-%d-%s" % (m, D)] = _p("le", *_ab(17, 33, dr), last="full" if m % 32 == 0 else "partial")
        for m, ch in ((513, "2"), (1025, "3")):
            t["rows-%d-narrow-%s" % (m, D)] = _p("le", *_ab(3, 5, dr), chunks=ch)
            t["rows-%d-wide-%s" % (m, D)] = _p("le", *_ab(56, 112, dr), chunks=ch)
            t["rows-%d-tall-%s" % (m, D)] = _p("gt", *_ab(112, 56, dr), chunks=ch)
        t["g-d18-" + D] = _p("le", 1, 1, groups=">16", launches=2)
        t["g-three-m-" + D] = _p("le", 1, 1, groups=">1")
        t["g-3+1-" + D] = _p("le", 1, 1, groups=">1")
        t["g-descending-" + D] = _p("le", 1, 1, strides="-")
        t["g-shared-omega-" + D] = _p("le", 1, 1, strides="0+")
        t["g-count33-" + D] = _p("le", 1, 1)
        t["g-count1-" + D] = _p("le", 1, 1, strides=".")
        t["g-spacings-" + D] = _p("le", 1, 1)
        t["g-psi-breaks-" + D] = _p("le", 1, 1, groups=">1")
        t["s-two-covered-" + D] = _p("le", 1, 1) + " | " + _p("le", *_ab(5, 40, dr))
        t["s-covered+fallback-" + D] = _p("le", 1, 1) + " | " + _fb("le")
        for l, r in OUTSIDE:
            t["out-%dx%d-%s" % (l, r, D)] = _fb(side(l, r))
        t["robust-" + D] = _p("le", *_ab(12, 20, dr))
        t["robust-tall-" + D] = _p("gt", *_ab(20, 12, dr))
        t["refine-50x100-" + D] = _p("le", *_ab(50, 100, dr))
    t["refine-13x29-R"] = _p("le", *_ab(13, 29, 0))
    t["refine-29x13-L"] = _p("gt", *_ab(29, 13, 1))
    return t


TAGS = _tags()


# ------------------------------------------------------------------------------------------------ operands
def _prescribed(l, r, kappa, rng):
    A = sr.prescribed(max(l, r), min(l, r), kappa if min(l, r) > 1 else 1, rng)
    return np.ascontiguousarray(A if l >= r else A.T)


def _int_omega(l, r, rng):
    """D S (l <= r) or S D: exact in fp64, Gram matrix D^2"""
    n, K = min(l, r), max(l, r)
    S = np.zeros((n, K))
    S[np.arange(n), rng.permutation(K)[:n]] = rng.choice([-1.0, 1.0], n)
    D = 2.0 ** rng.integers(-1, 2, n)
    W = D[:, None] * S
    return np.ascontiguousarray(W if l <= r else W.T)


def chol_spread(A):
    G = A @ A.T if A.shape[0] <= A.shape[1] else A.T @ A
    try:
        dg = np.diag(np.linalg.cholesky(G))
    except np.linalg.LinAlgError:
        return 0.0
    return float(dg.min() / dg.max())


def values(c, mode, seed, scale=1.0):
    """arena name -> {slot: matrix} for the inputs; mode: integer | gaussian | refine | robust | benign (robust's batch
    without the two)"""
    rng = np.random.default_rng([seed, sum(map(ord, c.id)), ("integer", "gaussian", "refine", "robust", "benign").index(mode)])
    v, truthP = {}, {}
    for name, (kind, size) in sorted(arena_names(c).items()):
        if kind not in ("psi", "om"):
            continue
        j = int(name[len(kind):])
        v[name] = {}
        for slot in sorted(set(slots_of(c, kind))):
            if kind == "psi":
                shp = core_shape(c, j)
                M = rng.integers(-8, 9, shp).astype(np.float64) if mode == "integer" else rng.standard_normal(shp)
            else:
                l, r = c.lr[j], c.rr[j]
                if mode == "integer":
                    M = _int_omega(l, r, rng)
                elif mode == "refine":
                    M = _prescribed(l, r, KAPPA_REFINE, rng)
                elif mode == "robust" and slot == 1:
                    B, Cf = sr.int_factors(l, r, c.opts["robust"], rng)
                    M = B @ Cf
                    truthP[(name, slot)] = sr.pinv_rank_k(B, Cf)
                elif mode == "robust" and slot == 2:
                    M = _prescribed(l, r, KAPPA_ILL, rng)
                else:
                    M = _prescribed(l, r, KAPPA, rng)
            v[name][slot] = np.ascontiguousarray(M * scale)
    v["_truthP"] = truthP
    return v


def arenas_in(c, v):
    """host images of the input arenas"""
    out = {}
    for name, (kind, size) in arena_names(c).items():
        if kind in ("psi", "om"):
            a = np.full(arena_size(c, name), SENT_F)
            for b in range(c.count):
                o, sz = place(c, name, b)
                a[o:o + sz] = v[name][slots_of(c, kind)[b]].ravel()
            out[name] = a
    return out


def arenas_out(c):
    return {name: np.full(arena_size(c, name), SENT_F) for name, (kind, _) in arena_names(c).items() if kind in OUT_KINDS}


def pointer_table(c, ptr):
    """(psi, omega, cores_out, work): the entry point's four pointer lists; ptr: arena name -> address of its element 0.
    The copied core aliases its Psi."""
    at = lambda name, b: ptr[name] + 8 * place(c, name, b)[0]
    psi = [at("psi%d" % j, b) for b in range(c.count) for j in range(c.d)]
    om = [at("om%d" % k, b) for b in range(c.count) for k in range(c.d - 1)]
    work = [at("work%d" % k, b) for b in range(c.count) for k in range(c.d - 1)]
    e = c.d - 1 if c.direction == 0 else 0
    cores = [at(("psi%d" if j == e else "c%d") % j, b) for b in range(c.count) for j in range(c.d)]
    return psi, om, cores, work


# ------------------------------------------------------------------------------------------------ truth and checks
def norm_pair(c, k, X, Om, P=None, C=None):
    """the pair's matrices in the normalised form (Xn, On, Pn, Cn)"""
    l, r = c.lr[k], c.rr[k]
    if c.direction == 0:
        return (X.reshape(-1, r), Om.reshape(l, r), None if P is None else P.reshape(r, l), None if C is None else C.reshape(-1, l))
    return (X.reshape(l, -1).T, Om.reshape(l, r).T, None if P is None else P.reshape(r, l).T, None if C is None else C.reshape(r, -1).T)


def pairs_of(c, ins, outs=None):
    """(k, b, Xn, On, Pn, Cn) of every pair from the arenas' host images"""
    for k, b, j, m in pair_list(c):
        names = pair_arenas(c, k, j)
        get = lambda img, name: img[name][place(c, name, b)[0]:place(c, name, b)[0] + place(c, name, b)[1]]
        X, Om = get(ins, names[0]), get(ins, names[1])
        C, P = (get(outs, names[2]), get(outs, names[3])) if outs is not None else (None, None)
        yield (k, b) + norm_pair(c, k, X, Om, P, C)


def int_pinv(On):
    """the exact (dyadic) pseudo-inverse of the normalised integer Omega D S / S D: On^T with every entry over its square"""
    P = On.T.copy()
    nz = P != 0
    P[nz] = 1.0 / P[nz]
    return P


def refined(Xn, On, Pn, dtype=LD):
    """(C1, C): the three products in `dtype`"""
    Xn, On, Pn = (np.asarray(x, dtype=dtype) for x in (Xn, On, Pn))
    C1 = Xn @ Pn
    return C1, C1 + (Xn - C1 @ On) @ Pn


def c_bound(Xn, On, Pn):
    a, b = Pn.shape
    A = np.abs(Xn) @ np.abs(Pn)
    B = (np.abs(Xn) + A @ np.abs(On)) @ np.abs(Pn) + A
    return C_BOUND * (2 * a + b + 5) * 2.0 ** -53 * B


def float64_pinv(On):
    """the kernel's pseudo-inverse restated in float64: Gram matrix of the short side, Cholesky inverse, solve"""
    b, a = On.shape
    if b <= a:
        G = On @ On.T
        Ri = np.linalg.inv(np.linalg.cholesky(G).T)
        return On.T @ (Ri @ Ri.T) + 0.0
    G = On.T @ On
    Ri = np.linalg.inv(np.linalg.cholesky(G).T)
    return (Ri @ Ri.T) @ On.T + 0.0


def float64_result(c, v, mode, refine=True):
    """the output arenas as a correct kernel would leave them, in float64 (robust Omegas: numpy's pinv)"""
    ins, outs = arenas_in(c, v), arenas_out(c)
    for k, b, j, m in pair_list(c):
        names = pair_arenas(c, k, j)
        sl = lambda name: slice(place(c, name, b)[0], place(c, name, b)[0] + place(c, name, b)[1])
        Xn, On, _, _ = norm_pair(c, k, ins[names[0]][sl(names[0])], ins[names[1]][sl(names[1])])
        Pn = float64_pinv(On) if chol_spread(On) > CHOL_GATE else np.linalg.pinv(On, rcond=1e-10)
        C1, C = refined(Xn, On, Pn, np.float64)
        Cn = (C if refine else C1) + 0.0
        outs[names[3]][sl(names[3])] = (Pn if c.direction == 0 else Pn.T).ravel()
        outs[names[2]][sl(names[2])] = (Cn if c.direction == 0 else Cn.T).ravel()
    return outs


def check_guards(c, outs, what=""):
    for name, img in outs.items():
        assert_guards(img, [(place(c, name, b)[0], (place(c, name, b)[1],), (1,)) for b in range(c.count)], "%s %s %s" % (c.id, what, name))


def _accept(what, got, ref, lapack, kappa, worst, key, turn=False):
    """the one rule, on P as the entry point stores it (r x l); turn: the normalised matrices are its transposes"""
    if turn:
        got, ref, lapack = got.T, ref.T, lapack.T
    e_lapack = max(sr.col_err(lapack, ref), 4 * EPS)
    err = sr.col_err(got, ref)
    worst[key] = max(worst.get(key, 0.0), err / (MARGIN * kappa * e_lapack))
    assert np.all(np.isfinite(got)), what
    assert err <= MARGIN * kappa * e_lapack, "%s: col_err %.3g beyond %g x %g x e_lapack %.3g" % (what, err, MARGIN, kappa, e_lapack)


_TRUTH = {}


def _pinv_truth(On, agree):
    key = (On.tobytes(), On.shape, agree)
    if key not in _TRUTH:
        _TRUTH[key] = sr.pinv_full(On, agree=agree) if agree < 1e-13 else sr.newton_schulz(*_ns_start(On), max_steps=6, agree=agree)[0]
    return _TRUTH[key]


def _ns_start(On):
    A = np.asarray(On, dtype=LD)
    X0 = np.linalg.pinv(On).astype(LD)
    b, a = On.shape
    return A, (A.T @ (X0.T @ X0) if b <= a else (X0 @ X0.T) @ A.T)


def refine_err(Xn, On, Cn):
    """(col_err(C, truth), e_lapack) of a refine case's pair: truth Xn pinv_full(On) in long double"""
    Ct = np.asarray(Xn, dtype=LD) @ _pinv_truth(On, sr.NS_AGREE_ILL)
    return sr.col_err(Cn, Ct), sr.col_err(Xn @ np.linalg.pinv(On), Ct)


def check_results(c, v, outs, mode, what=""):
    """every rule of the module's docstring for one call; -> {name: largest err / bar}"""
    what = what or "%s %s" % (c.id, mode)
    check_guards(c, outs, what)
    ins = arenas_in(c, v)
    worst = {}
    for k, b, Xn, On, Pn, Cn in pairs_of(c, ins, outs):
        at = "%s pair (k %d, b %d)" % (what, k, b)
        l, r = c.lr[k], c.rr[k]
        assert np.all(np.isfinite(Pn)) and np.all(np.isfinite(Cn)), at
        om_slot = slots_of(c, "om")[b]
        if mode == "integer" and covered(l, r):
            Pt = int_pinv(On)
            assert np.array_equal(Pn.view(np.uint64), Pt.view(np.uint64)), "%s: P differs from the dyadic inverse at %s" % (
                at, np.argwhere(Pn != Pt)[:4].tolist())
            Ct = (Xn @ Pt) + 0.0                      # one term per element: exact
            assert np.array_equal(Cn.view(np.uint64), Ct.view(np.uint64)), "%s: C differs at %s (largest %.3g)" % (
                at, np.argwhere(Cn != Ct)[:4].tolist(), np.max(np.abs(Cn - Ct)))
            continue
        # ---- the pseudo-inverse
        if mode == "integer":
            # (the orientation without a zero column: D S has min(l, r) non-zeros)
            _accept(at + " P", Pn, int_pinv(On).astype(LD), np.linalg.pinv(On), INT_KAPPA, worst, "P", turn=Pn.shape[1] > Pn.shape[0])
        elif mode == "robust" and om_slot in (1, 2):
            if om_slot == 1:
                Pt = v["_truthP"][("om%d" % k, 1)]
                Pt = Pt if c.direction == 0 else Pt.T
                lap = np.linalg.pinv(On, rcond=1e-10)
            else:
                Pt, lap = _pinv_truth(On, 2.0 ** -40), np.linalg.pinv(On)
            _accept(at + " P (Jacobi)", Pn, Pt, lap, 1.0, worst, "P robust", turn=c.direction == 1)
        else:
            kap = 1 if min(l, r) == 1 else {"refine": KAPPA_REFINE}.get(mode, KAPPA)
            Pt = _pinv_truth(On, sr.NS_AGREE if kap <= 10 else sr.NS_AGREE_ILL)
            _accept(at + " P", Pn, Pt, np.linalg.pinv(On), kap, worst, "P", turn=c.direction == 1)
        # ---- C against the three products of the P read back
        _, T = refined(Xn, On, Pn)
        err, bound = np.abs(Cn.astype(LD) - T).astype(np.float64), c_bound(Xn, On, Pn)
        ratio = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300))     # a zero bound (integer pass) admits zero only
        worst["C"] = max(worst.get("C", 0.0), float(ratio.max()))
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        assert ratio.max() <= 1.0, "%s: C%s is %.3g bounds from the refined product" % (at, tuple(int(x) for x in i), ratio.max())
        if mode == "refine":
            err, e_lapack = refine_err(Xn, On, Cn)
            worst["refine"] = max(worst.get("refine", 0.0), err / e_lapack)
            assert err <= REFINE_MARGIN * e_lapack, "%s: col_err(C) %.3g is %.1f e_lapack (bar %g)" % (at, err, err / e_lapack, REFINE_MARGIN)
    return worst


def check_untouched(outs, what):
    assert_untouched(outs, what)


def gaussian_mode(c):
    return "refine" if c.opts.get("refine") else "robust" if c.opts.get("robust") else "gaussian"
