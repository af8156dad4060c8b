"""The family table of ttsk_gemm: one case per dispatch edge of every kernel family behind it, with the family it is meant to
reach and its coverage tags.  tests/test_gpu_gemm_families.py runs every case on the device; tests/test_gemm_plan.py puts the
same descriptors through gemm_route and the plans of csrc/gemm_plan.h on the host and derives the tags from the plans' fields.
No GPU and no library needed to import it."""
import re
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np

PRE = POST = 64                     # guard elements before / after every buffer (even: keeps 16-byte alignment)
DESC = "bmoi,boin->bmn"             # the descriptor form: A[b,m,ko,ki], B[b,ko,ki,n], C[b,m,n]


@dataclass(frozen=True)
class V:
    """A strided view inside a buffer of its own: element offset after the leading guard, shape, strides."""
    shape: Tuple[int, ...]
    strides: Tuple[int, ...]
    off: int = 0

    @property
    def nelem(self):
        if any(n == 0 for n in self.shape):
            return self.off
        return self.off + 1 + sum((n - 1) * s for n, s in zip(self.shape, self.strides))


def dense(*shape, pad=0, off=0):
    """Row-major view; `pad` extra elements at the end of every row of the last index."""
    st, acc = [], 1
    for i, n in enumerate(reversed(shape)):
        st.append(acc)
        acc *= n + (pad if i == 0 else 0)
    return V(tuple(shape), tuple(reversed(st)), off)


def sliced(storage, starts, shape, off=0):
    """View shape[i] elements from starts[i] of a row-major `storage` array."""
    base = dense(*storage)
    return V(tuple(shape), base.strides, off + sum(a * s for a, s in zip(starts, base.strides)))


def framed(*shape, g=2, perm=None):
    """C inside a frame of g guard rows / columns on every side of every index (batch slices g + g apart).
    `perm`: the storage order of the indices (a transposed C); the view keeps the logical order."""
    perm = perm or tuple(range(len(shape)))
    st_shape = [shape[p] + 2 * g for p in perm]
    base = dense(*st_shape)
    strides = [0] * len(shape)
    for i, p in enumerate(perm):
        strides[p] = base.strides[i]
    return V(tuple(shape), tuple(strides), sum(g * s for s in base.strides))


def mat_rows(M, K, row=None, off=0, batch=1, bstride=None):
    """A[b, m, 0, k] = X[m, k]: k contiguous, rows `row` apart (descriptor form)."""
    row = K if row is None else row
    return V((batch, M, 1, K), (M * row if bstride is None else bstride, row, 0, 1), off)


def mat_cols(M, K, ld=None, off=0, batch=1, bstride=None):
    """A[b, m, 0, k] = X[k, m]: m contiguous (descriptor form)."""
    ld = M if ld is None else ld
    return V((batch, M, 1, K), (K * ld if bstride is None else bstride, 1, 0, ld), off)


def bmat_cols(K, N, ld=None, off=0, batch=1, bstride=None):
    """B[b, 0, k, n] = Y[k, n]: n contiguous."""
    ld = N if ld is None else ld
    return V((batch, 1, K, N), (K * ld if bstride is None else bstride, 0, ld, 1), off)


def bmat_rows(K, N, row=None, off=0):
    """B[0, 0, k, n] = Y[n, k]: k contiguous, rows `row` apart."""
    row = K if row is None else row
    return V((1, 1, K, N), (N * row, 0, 1, row), off)


@dataclass
class Case:
    id: str
    fam: Optional[str]             # regex matched at the start of the recorded kernel name; None: no bracketed launch
    spec: str
    A: V
    B: V
    C: V
    alpha: float = 1.0
    acc: int = 0
    ks: bool = False               # k_scale (descriptor form only)
    split_k: int = 0
    via: str = "contract"          # "contract": device.contract on DevArray views; "desc": ttsk_gemm with a GemmDesc
    launches: Optional[int] = None  # bracketed launches (default: 1, or 0 when fam is None)
    tags: Tuple[str, ...] = field(default_factory=tuple)


RL = "rows_longk_kernel"


def SR(nmt, nnt):
    return rf"skinny_r_kernel<{nmt}, {nnt}, 4>"


def SS(ring, strips):
    return rf"skinny_s_kernel<\d+, \d+, {ring}, {strips}>"


SM = "small_gemm_kernel"
G0, G1, G2 = r"gemm_f64_kernel<2, 2, 2, 2, ", r"gemm_f64_kernel<1, 4, ", r"gemm_f64_kernel<4, 1, "


def _c2(M, N):
    return framed(1, M, N)


# The family each case reaches is what gemm_route and the plans of csrc/gemm_plan.h decide (rows_longk_plan, skinny_r_plan,
# skinny_s_plan, small_gemm_plan, gemm_tile_plan); tests/test_gemm_plan.py derives it, and the tags the kernel name does not
# show, from the plans' fields on the host.  A device with 256 CUs is assumed for the chunk
# counts of skinny_r (want_chunks = 256 / m_tiles); the chunk is at least 64, so any K % 64 != 0 leaves a ragged last one.
# The first run on an MI355X reached every family as read, without corrections.
CASES = [
    # ---------------------------------------------------------------- rows_longk (gemm_plan.h rows_longk_plan)
    # (M = 1 or N = 1 through contract would give that index stride 0, which fails a_m >= K: descriptor form)
    Case("rl_n1_ragged_rows", RL, DESC, mat_rows(200, 4096), bmat_rows(4096, 1), _c2(200, 1), via="desc",
         tags=("rl:N=1", "rl:ragged_rows")),
    Case("rl_rows1_n33", RL, DESC, mat_rows(1, 8192), bmat_rows(8192, 33), _c2(1, 33), alpha=2.0, via="desc",
         tags=("rl:rows=1", "rl:N=33")),
    Case("rl_n48_acc", RL, "mk,nk->mn", dense(130, 4160), dense(48, 4160), framed(130, 48), alpha=-0.5, acc=1,
         tags=("rl:N=48", "rl:acc", "rl:ragged_rows")),
    Case("rl_padded_rows", RL, "mk,nk->mn", dense(65, 4096, pad=64), dense(16, 4096), framed(65, 16), alpha=2.0,
         tags=("rl:padded_rows",)),
    Case("rl_n33_odd_c", RL, "mk,nk->mn", dense(64, 4096), dense(33, 4096), framed(64, 33), acc=1,
         tags=("rl:N=33",)),
    # just outside its cover: skinny_r.  K % 64 != 0: gk variant (k contiguous on both sides, SkinnyRPlan.gk, r.a_gen = 2),
    # no swap (.swap), 7 x 2 tiles > SKR_KSPLIT_TILES: nsub 1 (.nsub); 65 chunks of 64 (.r.chunks, .r.chunk), the last one 4 long
    Case("rlx_k_not_64", SR(7, 2), "mk,nk->mn", dense(100, 4100), dense(20, 4100), framed(100, 20),
         tags=("rl-out:K%64", "sr:gk", "sr:nsub1", "sr:chunks_ragged", "sr:noswap")),
    # A one element into its buffer (8-byte aligned): rows_longk and gk refuse it, generic variant (.a_pair = 0, r.a_gen = 1); nsub 8
    Case("rlx_off8", SR(4, 1), "mk,nk->mn", dense(64, 4096, off=1), dense(16, 4096), framed(64, 16),
         tags=("rl-out:off8", "sr:gen_off8", "sr:nsub8")),
    Case("rlx_n49", SR(6, 4), "mk,nk->mn", dense(90, 4096), dense(49, 4096), framed(90, 49), alpha=-3.0, acc=1,
         tags=("rl-out:N=49", "sr:gk")),
    # ---------------------------------------------------------------- skinny_r (gemm_plan.h skinny_r_plan)
    # m / n contiguous, even extents and strides, aligned: the pair variant (.a_pair, .b_pair, r.a_gen = 0); no swap; nsub 8
    Case("sr_pair_noswap", SR(4, 2), "kp,kq->pq", dense(4160, 64), dense(4160, 32), framed(64, 32), alpha=0.5, acc=1,
         tags=("sr:pair", "sr:noswap", "sr:nsub8", "red:paired")),
    # 6 N tiles > 2 M tiles: swap (.swap); 6 x 2 = SKR_KSPLIT_TILES: still nsub 8 (.nsub)
    Case("sr_pair_swap", SR(6, 2), "kp,kq->pq", dense(5000, 32), dense(5000, 96), framed(32, 96), alpha=-3.0, acc=1,
         tags=("sr:pair", "sr:swap", "sr:nsub8")),
    # M = 300: three row tiles of 128, the last 44 rows; K = 4097 just above the limit, last chunk 1 long; nsub 1
    Case("sr_ragged_tile_k4097", SR(8, 2), "kp,kq->pq", dense(4097, 300), dense(4097, 20), framed(300, 20),
         tags=("sr:pair", "sr:ragged_tile", "sr:big>128", "sr:K4097", "sr:chunks_ragged", "sr:nsub1")),
    # odd M: not pairable (.a_pair = 0), generic variant for both sides (r.a_gen = r.b_gen = 1), swap (4 N tiles > 3 M tiles)
    Case("sr_gen_odd_m", SR(4, 3), "kp,kq->pq", dense(6000, 33), dense(6000, 64), framed(33, 64),
         tags=("sr:gen_oddM", "sr:swap")),
    # odd row stride of A (65): not pairable (.a_pair = 0), generic variant (r.a_gen = 1)
    Case("sr_gen_odd_stride", SR(4, 1), "kp,kq->pq", dense(4200, 64, pad=1), dense(4200, 16), framed(64, 16),
         alpha=2.0, acc=1, tags=("sr:gen_oddstride",)),
    Case("sr_gen_odd_nmt7", SR(7, 1), "kp,kq->pq", dense(4500, 111), dense(4500, 9), framed(111, 9),
         tags=("sr:gen_oddM",)),
    # (q, k) with k a slice of a longer axis: Ko = 9, Ki = 600 do not merge, r.rebase = 0; swap
    Case("sr_ko_nonuniform", SR(4, 3), "qkp,qkm->pm", sliced((9, 700, 34), (0, 3, 0), (9, 600, 34)),
         sliced((9, 650, 50), (0, 10, 0), (9, 600, 50)), framed(34, 50), alpha=0.5, acc=1,
         tags=("sr:ko_nonuniform", "sr:pair", "sr:swap")),
    # Ko = 4 x Ki = 1100 with uniform strides: gemm_collapse merges them into one K before skinny_r_plan, r.rebase = 1
    Case("sr_ko_uniform_desc", SR(3, 3), DESC, V((1, 48, 4, 1100), (0, 1, 1100 * 48, 48)),
         V((1, 4, 1100, 40), (0, 1100 * 40, 40, 1)), _c2(48, 40), via="desc", tags=("sr:rebase", "sr:pair")),
    # k contiguous on both sides, big side 130 > 128 (two row tiles, the second 2 rows): gk variant (.gk, r.a_gen = 2), swap
    Case("sr_gk_swap_big", SR(8, 3), "pk,qk->pq", dense(40, 6000), dense(130, 6000), framed(40, 130), alpha=0.5,
         acc=1, tags=("sr:gk", "sr:swap", "sr:ragged_tile", "sr:big>128", "sr:rebase")),
    # a transposed C (c_n != 1) through the scalar slab reduce, nmt 5
    Case("sr_pair_ct", SR(5, 1), DESC, mat_cols(80, 4608), bmat_cols(4608, 6), framed(1, 80, 6, perm=(0, 2, 1)),
         alpha=-0.5, acc=1, via="desc", tags=("sr:pair", "red:scalar")),
    # 8 x 4 tiles: nsub 1, 64 chunks of 64 (SkinnyRPlan.r.chunks, .chunk); 64 chunks of a 128 x 64 result with an aligned, even C:
    # the slab sum with 64 element pairs per chunk group (r_reduce_plan's paired-wide variant)
    Case("sr_reduce_wide", SR(8, 4), "kp,kq->pq", dense(4096, 128), dense(4096, 64), framed(128, 64),
         tags=("sr:pair", "sr:noswap", "sr:nsub1", "red:paired_wide")),
    # ---------------------------------------------------------------- skinny_s (gemm_plan.h skinny_s_plan)
    # A small (P = 5: P % 16 = 5 -> 2 strips), K = 128: 32 k-blocks, ring 4
    Case("ss_a_str2_k128", SS(4, 2), "mk,kn->mn", dense(5, 128), dense(128, 3000), framed(5, 3000),
         tags=("ss:a_small", "ss:str2", "ss:ring4", "ss:K128")),
    # B small (P = 20: 1 strip), K = 77 odd: 20 k-blocks, ring 5
    Case("ss_b_str1_k77", SS(5, 1), "mk,kn->mn", dense(4001, 77), dense(77, 20), framed(4001, 20), alpha=-0.5, acc=1,
         tags=("ss:b_small", "ss:str1", "ss:ring5", "ss:Kodd")),
    # K = 1 (contract gives the size-1 index stride 0), P = 32: no strips, 1 k-block: ring 4
    Case("ss_str0_k1", SS(4, 0), "mk,kn->mn", dense(32, 1), dense(1, 2500), framed(32, 2500),
         tags=("ss:a_small", "ss:str0", "ss:K1", "ss:ring4")),
    # a batch that shares the small operand (a_b = 0: contract moves b into the batch), P = 24 -> 2 strips, ring 5
    Case("ss_batch_shared", SS(5, 2), "mk,bkn->bmn", dense(24, 20), dense(3, 20, 700), framed(3, 24, 700),
         alpha=2.0, acc=1, tags=("ss:batch_shared", "ss:a_small", "ss:str2", "ss:ring5")),
    # odd K = 13 (4 k-blocks: ring 4), B small with P = 127 (P % 16 = 15: no strips)
    Case("ss_b_k13_p127", SS(4, 0), "mk,kn->mn", dense(2300, 13), dense(13, 127), framed(2300, 127),
         tags=("ss:b_small", "ss:Kodd", "ss:str0")),
    Case("ss_a_str1_ring5", SS(5, 1), "mk,kn->mn", dense(100, 100), dense(100, 2100), framed(100, 2100),
         tags=("ss:a_small", "ss:str1", "ss:ring5")),
    # ---------------------------------------------------------------- small_gemm (gemm_plan.h small_gemm_plan)
    Case("sm_b1", SM, "ij,jk->ik", dense(37, 29), dense(29, 53), framed(37, 53), tags=("sm:b1",)),
    Case("sm_batch3_acc", SM, "bij,bjk->bik", dense(3, 40, 30), dense(3, 30, 50), framed(3, 40, 50), alpha=-3.0,
         acc=1, tags=("sm:bN",)),
    Case("sm_k1024", SM, "ij,jk->ik", dense(20, 1024), dense(1024, 21), framed(20, 21), tags=("sm:K1024",)),
    Case("sm_512_k91", SM, "ij,jk->ik", dense(512, 91), dense(91, 512), framed(512, 512),     # 47.7 MFLOP
         tags=("sm:512x512x91",)),
    # one step past each limit: 48.2 MFLOP, K = 1025, M = 513, batch 33 > SK_MAXB
    Case("smx_flops", G0, "ij,jk->ik", dense(512, 92), dense(92, 512), framed(512, 512), tags=("sm-out:flops",)),
    Case("smx_k1025", G1, "ij,jk->ik", dense(20, 1025), dense(1025, 21), framed(20, 21),      # 1 tile: split-K 9
         tags=("sm-out:K", "g:autosplit")),
    Case("smx_m513", G2, "ij,jk->ik", dense(513, 30), dense(30, 20), framed(513, 20), tags=("sm-out:M",)),
    Case("smx_batch33", G1, "bij,bjk->bik", dense(33, 10, 12), dense(33, 12, 14), framed(33, 10, 14),
         tags=("sm-out:batch", "g:batch_strideC")),
    # ---------------------------------------------------------------- batched long-K (gemm_route GEMM_LONGK_BATCH, skinny_r_plan per group)
    # A shared by the batch (a_b = 0), K >= 32768: up to SK_MAXB problems per skinny_r launch, pair variant
    Case("lb_2", SR(1, 1), DESC, mat_cols(8, 32768, batch=2, bstride=0), bmat_cols(32768, 4, batch=2),
         framed(2, 8, 4), via="desc", tags=("lb:2", "lb:noacc")),
    Case("lb_32_acc", SR(1, 1), DESC, mat_cols(8, 32768, batch=32, bstride=0), bmat_cols(32768, 4, batch=32),
         framed(32, 8, 4), alpha=0.5, acc=1, via="desc", tags=("lb:32", "lb:acc")),
    # 33 problems: a launch of 32, then one of 1; N = 5 odd (generic variant), K = 33000 (last chunk ragged)
    Case("lb_33", SR(1, 1), DESC, mat_cols(8, 33000, batch=33, bstride=0), bmat_cols(33000, 5, batch=33),
         framed(33, 8, 5), alpha=-3.0, via="desc", launches=2, tags=("lb:33", "lb:noacc")),
    Case("lb_33_acc", SR(1, 1), DESC, mat_cols(6, 32768, batch=34, bstride=0), bmat_cols(32768, 4, batch=34),
         framed(34, 6, 4), alpha=2.0, acc=1, via="desc", launches=2, tags=("lb:33", "lb:acc")),
    # ---------------------------------------------------------------- gemm_f64_kernel (gemm_plan.h gemm_tile_plan)
    # family 0, 16 tiles < 192 and K >= 4 BK: automatic split-K (16 slabs) + splitk_reduce_kernel
    Case("g_fam0_autosplit", G0, "ij,jk->ik", dense(200, 2000), dense(2000, 200), framed(200, 200), alpha=0.5, acc=1,
         tags=("g:fam0", "g:autosplit")),
    Case("g_split1", G0, "ij,jk->ik", dense(200, 2000), dense(2000, 200), framed(200, 200), split_k=1,
         tags=("g:split1",)),
    Case("g_split3_odd", G0, "ij,jk->ik", dense(201, 1999), dense(1999, 203), framed(201, 203), split_k=3, alpha=-3.0,
         acc=1, tags=("g:split3",)),
    # split_k 5 > cdiv(40, BK) = 2: the chunk rounds up to BK, 2 slabs
    Case("g_split_big", G0, "ij,jk->ik", dense(600, 40), dense(40, 200), framed(600, 200), split_k=5,
         tags=("g:split_big",)),
    Case("g_fam1", G1, "ij,jk->ik", dense(100, 300), dense(300, 700), framed(100, 700), tags=("g:fam1",)),
    Case("g_fam2_acc", G2, "ij,jk->ik", dense(700, 300), dense(300, 100), framed(700, 100), alpha=-0.5, acc=1,
         tags=("g:fam2",)),
    # k_scale keeps every shape on the generic tiles: a skinny_s shape, a small shape, a rows_longk shape and a
    # non-merging (ko, ki) walk
    Case("g_kscale_skinny", G1, DESC, mat_rows(5, 128), bmat_cols(128, 3000), _c2(5, 3000), ks=True, via="desc",
         tags=("g:kscale_skinny",)),
    Case("g_kscale_small", G1, DESC, mat_rows(37, 29), bmat_cols(29, 53), _c2(37, 53), ks=True, alpha=2.0, acc=1,
         via="desc", tags=("g:kscale_small",)),
    Case("g_kscale_longk", G2, DESC, mat_rows(200, 4096), bmat_rows(4096, 16), _c2(200, 16), ks=True, via="desc",
         tags=("g:kscale_skinny",)),
    Case("g_kscale_ko", G1, DESC, V((1, 40, 3, 50), (0, 1, 64 * 40, 40)), V((1, 3, 50, 150), (0, 60 * 150, 150, 1)),
         _c2(40, 150), ks=True, alpha=-0.5, acc=1, via="desc", tags=("g:kscale_skinny",)),
    # batch > 1, C slices apart by a gap, transposed C (c_m = 1, c_n = 604)
    Case("g_batch_ct", G0, "bij,bjk->bik", dense(3, 600, 50), dense(3, 50, 130), framed(3, 600, 130, perm=(0, 2, 1)),
         alpha=2.0, acc=1, tags=("g:batch_strideC", "g:cT", "g:fam0")),
    Case("g_batch40_fam2", G2, "bij,bjk->bik", dense(40, 300, 64), dense(40, 64, 40), framed(40, 300, 40),
         tags=("g:batch_strideC", "g:fam2")),
    # ---------------------------------------------------------------- K == 0 (fill3_kernel, not bracketed) and empty
    Case("k0_acc0", None, DESC, mat_rows(5, 0), bmat_cols(0, 7), _c2(5, 7), via="desc", tags=("k0:acc0",)),
    Case("k0_acc1", None, DESC, mat_rows(6, 0), bmat_cols(0, 3), _c2(6, 3), alpha=2.0, acc=1, via="desc",
         tags=("k0:acc1",)),
    Case("empty_batch", None, DESC, mat_rows(4, 8, batch=0), bmat_cols(8, 4, batch=0), framed(0, 4, 4), via="desc",
         tags=("empty:batch",)),
    Case("empty_m", None, DESC, mat_rows(0, 8), bmat_cols(8, 4), _c2(0, 4), via="desc", tags=("empty:M",)),
    Case("empty_n", None, DESC, mat_rows(4, 8), bmat_cols(8, 0), _c2(4, 0), acc=1, via="desc", tags=("empty:N",)),
]

REQUIRED = {
    "rows_longk": ["rl:N=1", "rl:N=33", "rl:N=48", "rl:rows=1", "rl:ragged_rows", "rl:padded_rows", "rl:acc",
                   "rl-out:K%64", "rl-out:off8", "rl-out:N=49"],
    "skinny_r": ["sr:swap", "sr:noswap", "sr:pair", "sr:gen_oddM", "sr:gen_oddstride", "sr:gen_off8", "sr:gk",
                 "sr:rebase", "sr:ko_nonuniform", "sr:nmt<=4", "sr:nmt5-6", "sr:nmt7", "sr:nmt8", "sr:ragged_tile",
                 "sr:big>128", "sr:nsub8", "sr:nsub1", "sr:K4097", "sr:chunks_ragged"],
    "skinny_s": ["ss:str0", "ss:str1", "ss:str2", "ss:ring4", "ss:ring5", "ss:a_small", "ss:b_small",
                 "ss:batch_shared", "ss:K1", "ss:K128", "ss:Kodd"],
    "small_gemm": ["sm:b1", "sm:bN", "sm:K1024", "sm:512x512x91", "sm-out:flops", "sm-out:K", "sm-out:M",
                   "sm-out:batch"],
    "batched long-K": ["lb:2", "lb:32", "lb:33", "lb:acc", "lb:noacc"],
    "gemm_f64": ["g:fam0", "g:fam1", "g:fam2", "g:autosplit", "g:split1", "g:split3", "g:split_big",
                 "g:kscale_skinny", "g:kscale_small", "g:batch_strideC", "g:cT"],
    "slab reduce": ["red:scalar", "red:paired", "red:paired_wide"],
    "K == 0 / empty": ["k0:acc0", "k0:acc1", "empty:batch", "empty:M", "empty:N"],
}


def _family(c: Case) -> str:
    if c.fam is None:
        return "none"
    if c.fam.startswith("skinny_r") and c.A.shape[0] > 1 and c.via == "desc":
        return "batched long-K"
    return c.fam.split("<")[0].replace("_kernel", "")


def _derived_tags(c: Case):
    """Tags that follow from the expected kernel name itself (checked against the recorded name at run time)."""
    out = set()
    m = re.match(r"skinny_r_kernel<(\d+), (\d+), 4>", c.fam or "")
    if m and _family(c) == "skinny_r":
        nmt = int(m.group(1))
        out.add("sr:nmt<=4" if nmt <= 4 else "sr:nmt5-6" if nmt <= 6 else "sr:nmt7" if nmt == 7 else "sr:nmt8")
    if c.fam in (G0, G1, G2):
        out.add({G0: "g:fam0", G1: "g:fam1", G2: "g:fam2"}[c.fam])
    return out


def _sizes(c: Case):
    ia, ib_co = c.spec.split(",")
    ib, co = ib_co.split("->")
    size = dict(zip(ia, c.A.shape))
    size.update(zip(ib, c.B.shape))
    K = int(np.prod([size[x] for x in ia if x in ib and x not in co], dtype=np.int64))
    return size, K
