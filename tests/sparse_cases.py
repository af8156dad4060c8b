"""What tests/test_gpu_sparse_pass.py, tests/test_gpu_sparse_stream.py and the host-side coverage test in
tests/test_host_logic.py share: the catalogue of slice structures, the factor configurations of the pass kernel, the
launcher's choice of kernel instantiation restated on the host, and the plain segmented sum both references use.
Nothing here needs a device."""
from collections import namedtuple

import numpy as np

# ------------------------------------------------------------------ slice structures
# Streams are ascending in j.  Every structure here has N <= 2^17, fewer than 256 records per resident wave, so sg_plan
# (csrc/sparse_plan.h; held to this by tests/test_sparse_plan.py) gives each wave a stretch (`chunk`) of 256 records:
# 8 staged tiles of 32 records (16 tiles of 16 in the T = 16 instantiations), a tile being 8 (4) k-blocks of 4 records.
# Wave w holds records 256 w .. 256 w + 255; waves up to the next multiple of four are padding.
Structure = namedtuple("Structure", "name j n null_j")


def _st(name, j, n, null_j=False):
    j = np.asarray(j, dtype=np.int32)
    assert j.size and np.all(np.diff(j) >= 0) and j[0] >= 0 and j[-1] < n
    return Structure(name, j, int(n), null_j)


def structures():
    S = [_st("one", [1], 3)]                                                   # one record, an empty slice on either side
    for N in (255, 256, 257):                                                  # one slice: a wave short of one record, full, one record into the next
        S.append(_st(f"single{N}-nullj", np.zeros(N), 1, True))                # dev_j = NULL, n = 1
        S.append(_st(f"single{N}-equal", np.zeros(N), 1))                      # dev_j given, all equal
    S.append(_st("inside", np.full(1281, 3), 7))                               # waves wholly inside slice 3, empty slices around, padding waves
    S.append(_st("arange", np.arange(1100), 1100))                             # four slice changes in every k-block, n = N
    S.append(_st("runs256", np.repeat(np.arange(5), 256), 5))                  # boundaries on wave boundaries
    S.append(_st("runs32", np.repeat(np.arange(40), 32), 40))                  # on tile boundaries
    S.append(_st("runs4", np.repeat(np.arange(160), 4), 160))                  # on k-block boundaries
    S.append(_st("runs57", np.repeat(np.arange(64), np.tile([5, 7], 32)), 64))  # off every boundary
    singles = 4 + np.arange(40) + np.arange(40) // 3                           # 40 singletons with gaps in j: 4 .. 56
    S.append(_st("skewed", np.concatenate([np.full(700, 2), singles, np.full(300, 60)]), 64))  # first used slice 2, last 60 of 64
    S.append(_st("bign", np.sort(np.random.default_rng(71).integers(0, 5000, 6000)), 5000))    # sg_psi_reduce_kernel's grid-stride loop repeats
    tail = np.arange(513) // 60                                                # N = 256 * 2 + 1: the last wave holds one record
    S.append(_st("tail-continues", tail, 9))                                   # ... of the slice the wave before ends in
    S.append(_st("tail-opens", np.concatenate([tail[:-1], [9]]), 11))          # ... of a new slice (slice 10 stays empty)
    return S


# ------------------------------------------------------------------ factor configurations
# One factor of a pass: kind (1 table, 2 normals, 3 sign rows), its columns, first column of the DRM row (rank_min), the
# source of its flat index, and for sign rows their whole length and +-1 entries.
Spec = namedtuple("Spec", "kind w lo src full nnz", defaults=(0, 0))
# A, B, C: Spec or None (absent); c_left; exact: integer data compared with array_equal, else normals against the summation bound
Config = namedtuple("Config", "name A B C c_left exact")

WIDTHS = ((1, 1, 1), (3, 5, 7), (16, 16, 16), (17, 4, 9), (20, 20, 20), (5, 21, 1), (24, 24, 24), (25, 16, 3), (16, 32, 16),
          (32, 32, 8), (32, 32, 32))
ROLES = ("first", "last", "both")            # A absent (first mode), B absent (last mode), both present
OMEGAS = (None, "left", "right")             # no C; C with c_left = 1, src = 2; C with c_left = 0, src = 3


def table_config(widths, role, om):
    wA, wB, wC = widths
    A = None if role == "first" else Spec(1, wA, 0, 0)
    B = None if role == "last" else Spec(1, wB, 0, 1)
    C = None if om is None else Spec(1, wC, 0, 2 if om == "left" else 3)
    return Config("t%d-%d-%d-%s-%s" % (wA, wB, wC, role, om or "noC"), A, B, C, int(om == "left"), True)


def _sign_configs():
    out = []
    for nnz in (0, 1, 32):     # a whole sign row of 32 makes NT = 2 beside factors of at most 16 columns
        out.append(Config(f"sign32-B-nnz{nnz}", Spec(1, 16, 0, 0), Spec(3, 8, 5, 1, 32, nnz), Spec(1, 9, 0, 2), 1, True))
    for nnz in (0, 1, 30):
        out.append(Config(f"sign30-A-nnz{nnz}", Spec(3, 20, 7, 0, 30, nnz), Spec(1, 5, 0, 1), Spec(1, 3, 0, 3), 0, True))
    out.append(Config("sign32-C-nnz3", Spec(1, 4, 0, 0), Spec(1, 16, 0, 1), Spec(3, 8, 5, 2, 32, 3), 1, True))
    return out


TABLE_CONFIGS = [table_config(w, role, om) for w in WIDTHS for role in ROLES for om in OMEGAS]
SIGN_CONFIGS = _sign_configs()
SAMPLED_CONFIGS = [
    Config("normal20", Spec(2, 20, 0, 0), Spec(2, 20, 0, 1), Spec(2, 20, 0, 2), 1, False),
    Config("normal13-16-5-lo", Spec(2, 13, 3, 0), Spec(2, 16, 1, 1), Spec(2, 5, 2, 3), 0, False),
    Config("mixed", Spec(1, 9, 0, 0), Spec(2, 17, 2, 1), Spec(3, 6, 3, 2, 24, 4), 1, False),
]
# more than 256 waves: sg_om_reduce_kernel's `w += 256` loop repeats, sg_psi_reduce_kernel adds hundreds of partial blocks
LONG_CONFIGS = [table_config((4, 4, 4), "both", "left"), table_config((4, 4, 4), "both", "right")]
CONFIGS = TABLE_CONFIGS + SIGN_CONFIGS + SAMPLED_CONFIGS + LONG_CONFIGS

INSTANTIATIONS = ((1, 0, 32), (2, 0, 32), (2, 1, 32), (2, 2, 32), (2, 0, 16), (2, 1, 16), (2, 2, 16))


def _per_wave(tcols, tab, qcols, T):
    """sg_lds_layout(...).total of csrc/sparse_plan.h: doubles of LDS per wave"""
    return T * tcols + tab + 4 * T + T // 2 + (T * qcols + 3) // 4


def instantiation(cfg):
    """(NT, NS, T) of sg_pass_kernel as sg_plan (csrc/sparse_plan.h) chooses it for the factors of ``cfg``; restated here on
    purpose: tests/test_sparse_plan.py holds it against the plan itself"""
    cols = tab = qcols = 0
    widest = wmax = 1
    for F in (cfg.A, cfg.B, cfg.C):
        if F is None:
            continue
        if F.kind == 3:                    # the whole sign row is staged
            cols += F.full
            widest = max(widest, F.full)
        elif F.kind == 2:
            cols += F.w
            qcols += F.w
        else:                              # a table block of ceil(w / 2) 16-byte units per nonzero
            tab += 2 * ((F.w + 1) // 2)
        widest, wmax = max(widest, F.w), max(wmax, F.w)
    NT = 2 if widest > 16 else 1
    NS = (1 if wmax <= 20 else 2) if NT == 2 and 16 < wmax <= 24 else 0
    tcols = max(cols, 1)
    fixed = 16 * NT * 24 + 64
    T = 32
    if NT == 2 and (156 * 1024) // (_per_wave(tcols, 32 * tab, qcols, 32) * 32 + fixed) < 2:
        T = 16
    return NT, NS, T


# ------------------------------------------------------------------ the plain sum
def segmented_outer(j, n, VA, B):
    """out[a, k, c] = sum_{e: j_e = k} VA[e, a] B[e, c] in the dtype of the operands (int64 or longdouble), any order of j"""
    j = np.asarray(j)
    out = np.zeros((VA.shape[1], n, B.shape[1]), dtype=np.result_type(VA, B))
    if j.size == 0:
        return out
    order = np.argsort(j, kind="stable")
    js = j[order]
    starts = np.flatnonzero(np.r_[True, js[1:] != js[:-1]])
    terms = VA[order][:, :, None] * B[order][:, None, :]
    out[:, js[starts], :] = np.add.reduceat(terms, starts, axis=0).transpose(1, 0, 2)
    return out
