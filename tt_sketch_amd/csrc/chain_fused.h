// One step of a TensorTrainDRM chain with the intermediate kept on chip.
//
//   reference: tensor_train_drm.py:81-87   L_mu[l,m] = sum_{i,j,k} L_{mu-1}[i,j] X_mu[i,k,l] D_mu[j,k,m]
//   (right sketches run the same line on the transposed tensor, drm_base.py:122-145)
//
// In the names used here, for one tensor of the batch and one mode:
//   W [c][a]      the carried matrix L_{mu-1} / R  (K1 x A), c = TT bond contracted with X, a = DRM rank in
//   X             the TT core, addressed by strides as G_k[j][c] (k = mode index, j = the other TT bond)
//   E [a][k][a']  the DRM core (A x n x A2), shared by all tensors of the batch
//   Out[j][a']    = sum_k ( G_k W ) E_k          (J x A2)
// The two-launch form (skinny.h) writes T[a][k][j] = sum_c W[c][a] G_k[j][c] to HBM and reads it back
// for the second product: ~55 % of the bytes a chain step moves.  Here a workgroup owns a range of
// slices k of one tensor; per slice
//   phase A   T_k^T[a][j] = sum_c W[c][a] G_k[j][c]      W from LDS, G_k fragments straight from memory
//   phase B   Out[j][a'] += sum_a T_k[j][a] E_k[a][a']   E_k from LDS
// and T_k never leaves the registers: with mfma(A = W^T fragment, B = G fragment) register t of the
// 16x16 accumulator tile Q holds T^T[16 Q + 4 t + (lane >> 4)][lane & 15], which IS the A-operand
// fragment of k-block 4 Q + t for phase B (lane (x, kq) holds T[j0 + x][4 (4 Q + t) + kq]).
// Up to four row tiles wave w owns the 16 rows j0 = 16 w of the output; beyond that the host deals pieces (row tile,
// range of Q) over 12 waves so that the four SIMDs are level (chain_deal.h).  A further wave -- every wave without a
// piece -- does nothing but bring E_k into LDS (global_load_lds, 1 KB per instruction) while the others are in
// phase A.  The left chain also needs
// T in memory for Psi_mu = T_mu R_mu (tensor_train_sketch.py:28-34): it is stored from the phase-A
// registers on the way (WT).
//
// Partial tiles (rank 100 = 6 x 16 + 4, rank 50 = 3 x 16 + 2) are 4-wide strips computed with
// v_mfma_f64_4x4x4 (4 blocks): 16 instead of 64 cycles of the matrix pipe.
//
// Two workgroup-level stages -- the XCD mapping and the gathering E loader -- are defined in chain_stages.h, for this
// kernel and chain_wide.h; the launchers' slab request and slab reduce at the end of this file, for all three.
#pragma once
#include "chain_stages.h"

namespace ttsk {

// Timing experiments (TTSK_CF_DIAG / TTSK_CF_STAMPS) exist in a lab build only (-DTTSK_LAB): the shipped code object carries
// neither the run-time switches nor the stamp stores in its hot loop.
#ifdef TTSK_LAB
#define CF_DIAG(bit) (a.diag & (bit))
#define CF_STAMP(i) do { if (a.stamps && blockIdx.x == 0 && lane == 0 && k - k_beg < 8) a.stamps[((k - k_beg) * CD_WAVES + w) * 8 + (i)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define CF_DIAG(bit) 0
#define CF_STAMP(i) do { } while (0)
#endif
#define CF_BARRIER() do { if (!CF_DIAG(4)) lds_barrier(); } while (0)

// One piece of a row tile (chain_deal.h): rows 16 tile .. + 15, the NQF full tiles of a from tile q0 on and the STRQ
// strips behind them -- both counts static, the origin a run-time offset into the two LDS images and into T.  KIND
// says how the partial result reaches the slab.  APC: the row length of the W image where it is static (levelled
// workgroups: every k-block's fragment address is then an immediate offset, not a register held across the slice
// loop -- the whole-range body would not fit three waves per SIMD otherwise), 0 = a.AP.
template <int NQF, int STRQ, int NNF, int STRN, int D, bool WT, int EBUF, int UNR, int KIND, int APC = 0>
__device__ __forceinline__ void cf_piece(const ChainStep &a, const double *Wl, const double *El, int tile, int q0, int prob,
                                         int g, int k_beg, int k_end, int KB1, int w, int lane)
{
    const int x16 = lane & 15, kq = lane >> 4;
    const int AP = APC ? APC : a.AP, A2P = a.A2P;
    const int j0 = 16 * tile;
    const bool jok = j0 + x16 < a.J;
    const uint32_t xlane = !CF_DIAG(1) ? (uint32_t)(((int64_t)(j0 + x16) * a.x_j + (int64_t)kq * a.x_c) * 8) : OOB_OFF;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(uniform_ptr(a.X[prob]), a.x_extent * 8);
    // wave-uniform by construction; said so explicitly, or a value the register allocator parks in a
    // vector register turns every load below into a waterfall loop
    const uint32_t xstep = __builtin_amdgcn_readfirstlane((uint32_t)(4 * a.x_c * 8));
    const uint32_t kstep = __builtin_amdgcn_readfirstlane((uint32_t)(a.x_k * 8));
    static_assert(UNR % D == 0, "the unrolled body must keep the ring slots static");
    // k-blocks are issued in straight-line runs of UNR (the compiler's wait counts are exact inside a run;
    // at a loop edge it waits for every load in flight); a slice is padded to whole runs
    const int ITER = KB1 / UNR;
    // fragment kb of slice k: per-lane (row, k) offset fixed, the (slice, k-block) part a scalar offset.  No
    // masks: k beyond K1 meets the zero rows of the W image, rows beyond J give output rows that are never
    // stored, a prefetch past the workgroup's last slice is unused, and whatever lies beyond the core reads
    // as 0 through the descriptor's range check.
    auto xload = [&](uint32_t so) -> double { return ld8(rx, xlane, __builtin_amdgcn_readfirstlane(so)); };
    double ring[D];
#pragma unroll
    for (int d = 0; d < D; ++d) ring[d] = xload((uint32_t)k_beg * kstep + (uint32_t)d * xstep);

    v4d acc2[NNF ? NNF : 1];
    double acc2s[STRN ? STRN : 1];
#pragma unroll
    for (int p = 0; p < NNF; ++p)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc2[p][t] = 0.0;
#pragma unroll
    for (int q = 0; q < STRN; ++q) acc2s[q] = 0.0;

    // LDS addresses of this lane's fragment elements inside a k-block's two sections
    const int wl_lane = (kq >> 1) * 2 * AP + 2 * (16 * q0 + x16) + (kq & 1);
    const int ws_lane = (kq >> 1) * 2 * AP + 2 * (16 * (q0 + NQF) + (x16 & 3)) + (kq & 1);
    const int el_lane = e_frag_lane(x16, kq, A2P);
    const int es_col = 16 * NNF + (x16 & 3);
    const int es_lane = e_strip_lane(kq, A2P);

    __amdgpu_buffer_rsrc_t rt;
    if constexpr (WT) rt = make_rsrc(uniform_ptr(a.T[prob]), a.t_extent * 8);

    for (int k = k_beg; k < k_end; ++k) {
        v4d acc1[NQF ? NQF : 1];
        double acc1s[STRQ ? STRQ : 1];
#pragma unroll
        for (int p = 0; p < NQF; ++p)
#pragma unroll
            for (int t = 0; t < 4; ++t) acc1[p][t] = 0.0;
#pragma unroll
        for (int q = 0; q < STRQ; ++q) acc1s[q] = 0.0;

        CF_STAMP(0);
        // ---- phase A.  Each k-block: the W fragments of the NEXT k-block are requested from LDS before this
        // one's matrix instructions are issued (a wave then covers its own LDS latency -- the matrix pipe
        // serves the older wave of a SIMD first, so the younger one cannot be counted on to fill the gaps),
        // and the ring slot is reloaded AFTER its fragment has been consumed, so that the load can land in the
        // same register (reloading first forces a copy at the loop edge behind an s_waitcnt vmcnt(0)).
        double af[NQF ? NQF : 1], sf[STRQ ? STRQ : 1];
        // fragments of k-block (run base) + u: compile-time offsets from the run's base address (u = UNR, the
        // look-ahead of a run's last k-block, reads the rows behind the W image: finite, unused)
        auto wfetch = [&](const double *wrun, int u, double (&f)[NQF ? NQF : 1], double (&g)[STRQ ? STRQ : 1]) {
#pragma unroll
            for (int p = 0; p < NQF; ++p) f[p] = LDS_UNPAIRED(wrun[wl_lane + u * 4 * AP + 32 * p]);
#pragma unroll
            for (int q = 0; q < STRQ; ++q) g[q] = wrun[ws_lane + u * 4 * AP + 8 * q];
        };
        wfetch(Wl, 0, af, sf);
        uint32_t so = (uint32_t)k * kstep + (uint32_t)D * xstep;      // scalar offset of the next fragment to request
        // k-block (run base) + u with u < UNR static; the reloads of the slice's last D k-blocks are the first
        // fragments of the next slice
        auto kblock = [&](const double *wrun, int u, bool wrap) {
            const int d = u % D;
            double afn[NQF ? NQF : 1], sfn[STRQ ? STRQ : 1];
            wfetch(wrun, u + 1, afn, sfn);
            const double bf = ring[d];
#pragma unroll
            for (int p = 0; p < NQF; ++p) acc1[p] = mfma16(af[p], bf, acc1[p]);
#pragma unroll
            for (int q = 0; q < STRQ; ++q) acc1s[q] = mfma4(sf[q], bf, acc1s[q]);
            if (wrap) so = (uint32_t)(k + 1) * kstep;
            ring[d] = xload(so);
            so += xstep;
#pragma unroll
            for (int p = 0; p < NQF; ++p) af[p] = afn[p];
#pragma unroll
            for (int q = 0; q < STRQ; ++q) sf[q] = sfn[q];
        };
        for (int it = 0; it < ITER; ++it) {
            const double *wrun = Wl + it * UNR * 4 * AP;
            const bool last = it == ITER - 1;
#pragma unroll
            for (int u = 0; u < UNR; ++u) kblock(wrun, u, last && u + D == UNR);
        }
        if constexpr (WT) {
            // T[a][k][j]: register t of tile p is row a = 16 (q0 + p) + 4 t + kq, 16 consecutive j per row
            const int64_t nJ = (int64_t)a.n * a.J;
            const int a0 = 16 * q0;
            const uint32_t tl = jok ? (uint32_t)(((int64_t)(a0 + kq) * nJ + (int64_t)k * a.J + j0 + x16) * 8) : OOB_OFF;
#pragma unroll
            for (int p = 0; p < NQF; ++p)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    st8(rt, (jok && a0 + 16 * p + 4 * t + kq < a.A) ? tl + (uint32_t)((16 * p + 4 * t) * nJ * 8) : OOB_OFF, acc1[p][t]);
#pragma unroll
            for (int q = 0; q < STRQ; ++q)
                st8(rt, (jok && a0 + 16 * NQF + 4 * q + kq < a.A) ? tl + (uint32_t)((16 * NQF + 4 * q) * nJ * 8) : OOB_OFF, acc1s[q]);
        }
        CF_STAMP(1);
        CF_BARRIER();                                  // B1
        CF_STAMP(2);

        // ---- phase B: k-block kap = 4 p + t of T is register t of tile p.  Same look-ahead: the E fragments of
        // k-block kap + 1 are requested before the matrix instructions of kap (left to itself the compiler
        // requests them right in front of their first use and every k-block waits out the LDS latency).
        {
            const double *eb = El + (EBUF == 2 ? (k & 1) * a.eunits * 2 : 0) + q0 * 16 * A2P;   // k-block 4 q0
            double bf[NNF ? NNF : 1], bs[STRN ? STRN : 1];
            // per-slice copies of the lane offsets the compiler cannot see through: it then forms each k-block's
            // address with one add where it is used, instead of keeping 2 x 25 precomputed addresses alive across
            // the slice loop (and spilling them into the phase)
            int el0 = el_lane, es0 = es_lane + e_image_at(0, es_col, A2P);
            asm volatile("" : "+v"(el0), "+v"(es0));
            auto efetch = [&](int kap, double (&f)[NNF ? NNF : 1], double (&g)[STRN ? STRN : 1]) {
#pragma unroll
                for (int nn = 0; nn < NNF; ++nn) f[nn] = LDS_UNPAIRED(eb[el0 + kap * 4 * A2P + 32 * nn]);
#pragma unroll
                for (int q = 0; q < STRN; ++q) g[q] = eb[es0 + kap * 4 * A2P + 8 * q];
            };
            // two fragment sets used in turn (even / odd k-blocks): with one set and a copy the compiler merges the
            // look-ahead registers with the current ones and the requests slide back behind the matrix instructions
            double bf2[NNF ? NNF : 1], bs2[STRN ? STRN : 1];
            efetch(0, bf, bs);
            constexpr int KB2C = 4 * NQF + STRQ;
#pragma unroll
            for (int kap = 0; kap < KB2C; ++kap) {
                const int p = kap >> 2, t = kap & 3;
                const double af2 = p < NQF ? acc1[p < NQF ? p : 0][t] : acc1s[t < STRQ ? t : 0];
                if (kap & 1) {
                    if (kap + 1 < KB2C) efetch(kap + 1, bf, bs);
                    __builtin_amdgcn_sched_barrier(0);      // the requests stay in front of this k-block's matrix instructions
#pragma unroll
                    for (int nn = 0; nn < NNF; ++nn) acc2[nn] = mfma16(af2, bf2[nn], acc2[nn]);
#pragma unroll
                    for (int q = 0; q < STRN; ++q) acc2s[q] = mfma4(af2, bs2[q], acc2s[q]);
                } else {
                    if (kap + 1 < KB2C) efetch(kap + 1, bf2, bs2);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int nn = 0; nn < NNF; ++nn) acc2[nn] = mfma16(af2, bf[nn], acc2[nn]);
#pragma unroll
                    for (int q = 0; q < STRN; ++q) acc2s[q] = mfma4(af2, bs[q], acc2s[q]);
                }
            }
        }
        CF_STAMP(3);
        CF_BARRIER();                                  // B2
        CF_STAMP(4);
    }

    // ---- partial result of this workgroup: slab[problem][g][j][a'].  The two pieces of a cut row tile hold partial
    // sums of the same rows: REST stores its own, FIRST adds its own to that behind a barrier of the workgroup (whole
    // row tiles have left by then: a finished wave leaves the barrier count).
    double *slab = a.slab + ((int64_t)prob * a.wpp + g) * a.J * a.A2;
    if constexpr (KIND == CD_FIRST) __syncthreads();
    // levelled bodies: the lane's coordinates are derived again here, or they are held -- spilled, at three waves
    // per SIMD -- across the slice loop for these few stores
    int ln = lane;
    if constexpr (APC != 0) asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
    const int sx = ln & 15, sk = ln >> 4;
#pragma unroll
    for (int nn = 0; nn < NNF; ++nn)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int j = j0 + 4 * t + sk, col = 16 * nn + sx;
            if (j < a.J && col < a.A2) {
                double *p = slab + (int64_t)j * a.A2 + col;
                *p = KIND == CD_FIRST ? acc2[nn][t] + *p : acc2[nn][t];
            }
        }
#pragma unroll
    for (int q = 0; q < STRN; ++q) {
        // 4x4x4 result: lane (i = l >> 4, beta = (l >> 2) & 3, c = l & 3) holds row 4 beta + i, column c of the strip
        const int j = j0 + 4 * ((ln >> 2) & 3) + sk, col = 16 * NNF + 4 * q + (ln & 3);
        if (j < a.J && col < a.A2) {
            double *p = slab + (int64_t)j * a.A2 + col;
            *p = KIND == CD_FIRST ? acc2s[q] + *p : acc2s[q];
        }
    }
    if constexpr (KIND == CD_REST) {
        __threadfence_block();
        __syncthreads();
    }
}

// A last row tile with at most 4 valid rows j0 .. j0 + 3, by the four blocks of v_mfma_f64_4x4x4 (block beta = bits 2..3
// of the lane within its 16, m / n = bits 0..1, k = lane >> 4):
//   phase A   block beta of tile p:  A = W^T[16 p + 4 beta + m][k]  (the usual W fragment), B = G[j0 + n][k] (the same
//             four rows in every block)  ->  lane l holds T^T[16 p + 4 beta + (l >> 4)][j0 + (l & 3)]
//   phase B   that register IS the A operand of block beta for k = a in 16 p + 4 beta + (0..3); with B = E_k[a][4 c + n]
//             block beta accumulates its quarter of the sum over a for the output columns 4 c .. 4 c + 3.
// One instruction (16 cycles) per tile and k-block in phase A, one per tile and 4 columns in phase B: a quarter of a
// row tile's matrix time, and no move between lanes until the four blocks' partial sums are added once at the end.
// A strip of a is the same 4x4 product in every block; it meets E only in block 0.
template <int NQF, int STRQ, int NNF, int STRN, int D, bool WT, int EBUF, int UNR, int APC>
__device__ __forceinline__ void cf_rows4(const ChainStep &a, const double *Wl, const double *El, int tile, int prob, int g,
                                         int k_beg, int k_end, int KB1, int w, int lane)
{
    constexpr int NC = 4 * NNF + STRN;                 // groups of 4 output columns
    // a short piece whose k-blocks wait out their own LDS latency: served first, its gaps go to the SIMD's other waves
    // (as the youngest wave it would run alone behind them, at a third of the pipe)
    __builtin_amdgcn_s_setprio(2);
    const int x16 = lane & 15, kq = lane >> 4, n4 = x16 & 3, beta = x16 >> 2;
    constexpr int AP = APC;
    const int A2P = a.A2P;
    const int j0 = 16 * tile;
    const bool jok = j0 + n4 < a.J;
    const uint32_t xlane = !CF_DIAG(1) ? (uint32_t)(((int64_t)(j0 + n4) * a.x_j + (int64_t)kq * a.x_c) * 8) : OOB_OFF;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc(uniform_ptr(a.X[prob]), a.x_extent * 8);
    const uint32_t xstep = __builtin_amdgcn_readfirstlane((uint32_t)(4 * a.x_c * 8));
    const uint32_t kstep = __builtin_amdgcn_readfirstlane((uint32_t)(a.x_k * 8));
    const int ITER = KB1 / UNR;
    auto xload = [&](uint32_t so) -> double { return ld8(rx, xlane, __builtin_amdgcn_readfirstlane(so)); };
    double ring[D];
#pragma unroll
    for (int d = 0; d < D; ++d) ring[d] = xload((uint32_t)k_beg * kstep + (uint32_t)d * xstep);

    double acc2[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc2[c] = 0.0;

    const int wl_lane = (kq >> 1) * 2 * AP + 2 * x16 + (kq & 1);
    const int ws_lane = (kq >> 1) * 2 * AP + 2 * (16 * NQF + n4) + (kq & 1);
    // E[row][col] sits at e_image_at(row, col); row = 16 p + 4 beta + kq (a strip: 16 NQF + 4 q + kq in every block),
    // col = 4 c + n
    const int el_lane = e_image_at(4 * beta + kq, n4, A2P);
    const int es_lane = e_image_at(kq, n4, A2P);

    __amdgpu_buffer_rsrc_t rt;
    if constexpr (WT) rt = make_rsrc(uniform_ptr(a.T[prob]), a.t_extent * 8);

    for (int k = k_beg; k < k_end; ++k) {
        double acc1[NQF], acc1s[STRQ ? STRQ : 1];
#pragma unroll
        for (int p = 0; p < NQF; ++p) acc1[p] = 0.0;
#pragma unroll
        for (int q = 0; q < STRQ; ++q) acc1s[q] = 0.0;
        CF_STAMP(0);
        uint32_t so = (uint32_t)k * kstep + (uint32_t)D * xstep;
        for (int it = 0; it < ITER; ++it) {
            const double *wrun = Wl + it * UNR * 4 * AP;
            const bool last = it == ITER - 1;
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int d = u % D;
                const double bf = ring[d];
#pragma unroll
                for (int p = 0; p < NQF; ++p) acc1[p] = mfma4(LDS_UNPAIRED(wrun[wl_lane + u * 4 * AP + 32 * p]), bf, acc1[p]);
#pragma unroll
                for (int q = 0; q < STRQ; ++q) acc1s[q] = mfma4(wrun[ws_lane + u * 4 * AP + 8 * q], bf, acc1s[q]);
                if (last && u + D == UNR) so = (uint32_t)(k + 1) * kstep;
                ring[d] = xload(so);
                so += xstep;
            }
        }
        if constexpr (WT) {
            // T[a][k][j]: tile p holds row a = 16 p + 4 beta + kq, a strip (block 0's copy) row 16 NQF + 4 q + kq
            const int64_t nJ = (int64_t)a.n * a.J;
            const uint32_t tl = (uint32_t)(((int64_t)kq * nJ + (int64_t)k * a.J + j0 + n4) * 8);
#pragma unroll
            for (int p = 0; p < NQF; ++p)
                st8(rt, (jok && 16 * p + 4 * beta + kq < a.A) ? tl + (uint32_t)((16 * p + 4 * beta) * nJ * 8) : OOB_OFF, acc1[p]);
#pragma unroll
            for (int q = 0; q < STRQ; ++q)
                st8(rt, (jok && beta == 0 && 16 * NQF + 4 * q + kq < a.A) ? tl + (uint32_t)((16 * NQF + 4 * q) * nJ * 8) : OOB_OFF,
                    acc1s[q]);
        }
        CF_STAMP(1);
        CF_BARRIER();                                  // B1
        CF_STAMP(2);
        {
            const double *eb = El + (EBUF == 2 ? (k & 1) * a.eunits * 2 : 0);
            int el0 = el_lane, es0 = es_lane;
            asm volatile("" : "+v"(el0), "+v"(es0));
#pragma unroll
            for (int p = 0; p < NQF; ++p)
#pragma unroll
                for (int c = 0; c < NC; ++c) acc2[c] = mfma4(acc1[p], eb[el0 + p * 16 * A2P + 8 * c], acc2[c]);
#pragma unroll
            for (int q = 0; q < STRQ; ++q)
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    const double e = eb[es0 + (8 * NQF + 2 * q) * 2 * A2P + 8 * c];
                    acc2[c] = mfma4(acc1s[q], beta == 0 ? e : 0.0, acc2[c]);
                }
        }
        CF_STAMP(3);
        CF_BARRIER();                                  // B2
        CF_STAMP(4);
    }

    // lane l holds block beta's part of Out[j0 + (l >> 4)][4 c + (l & 3)]: add the four blocks, block 0 stores
    double *slab = a.slab + ((int64_t)prob * a.wpp + g) * a.J * a.A2;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        double v = acc2[c];
        v += __shfl_xor(v, 4);
        v += __shfl_xor(v, 8);
        const int j = j0 + kq, col = 4 * c + n4;
        if (beta == 0 && j < a.J && col < a.A2) slab[(int64_t)j * a.A2 + col] = v;
    }
}

// NQF / NNF full 16-wide tiles of a / a', STRQ / STRN 4-wide strips behind them; D ring depth of the
// G fragments; WT: T is also written to memory; OCC workgroups per CU the register budget allows.
// NWV waves per workgroup: 8 = wave w runs row tile w, CD_WAVES = every wave runs the piece the host dealt it.
template <int NQF, int STRQ, int NNF, int STRN, int D, bool WT, int OCC, int EBUF, int UNR = 5 * D, int NWV = 8>
__global__ __launch_bounds__(64 * NWV, NWV == 8 ? 2 * OCC : 1) void chain_step_kernel(ChainStep a)
{
    extern __shared__ double cf_lds[];
    double *Wl = cf_lds;
    double *El = cf_lds + a.ebase;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    constexpr int NT = 64 * NWV;
    int prob, g;                                       // the unit of a problem: its slice range g
    chain_block_unit(a.xcd_map, a.wpp, prob, g);
    const int k_beg = (int)((int64_t)g * a.n / a.wpp), k_end = (int)((int64_t)(g + 1) * a.n / a.wpp);
    // k-blocks of phase A, padded to whole runs of UNR (the padded ones meet zero rows of the W image)
    const int KB1 = ((a.K1 + 3) / 4 + UNR - 1) / UNR * UNR;
    const int AP = a.AP, A2P = a.A2P;

    // ---- stage W: Wl[(c >> 1) * 2 AP + 2 a + (c & 1)], zero beyond (K1, A).  A pair of k rows interleaved:
    // the 32 lanes (kq in {0, 1}, x) of a fragment read 32 consecutive doubles = all 64 banks once.
    {
        const double *Wp = uniform_ptr(a.W[prob]);
        const __amdgpu_buffer_rsrc_t rw = make_rsrc(Wp, ((int64_t)(a.K1 - 1) * a.w_c + a.A) * 8);
        const int total = 4 * KB1 * AP;
        constexpr int BATCH = 10;
        for (int e0 = tid; e0 < total; e0 += NT * BATCH) {
            double v[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int e = e0 + NT * u;
                const int c = e / AP, col = e - c * AP;
                v[u] = ld8(rw, (e < total && c < a.K1 && col < a.A) ? (uint32_t)(((int64_t)c * a.w_c + col) * 8) : OOB_OFF, 0);
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int e = e0 + NT * u;
                const int c = e / AP, col = e - c * AP;
                if (e < total) Wl[(c >> 1) * 2 * AP + 2 * col + (c & 1)] = v[u];
            }
        }
    }

    // the wave's piece (levelled workgroups): wave-uniform, fetched once.  Every wave the deal left without a piece is a
    // loader: loader li of nl brings every nl-th KB of E_k (one wave alone needs longer for all of E_k at rank 100 than a
    // levelled phase A takes, gathered or packed)
    unsigned pc = 0;
    int li = 0, nl = 1;
    if constexpr (NWV != 8) {
        pc = a.piece[__builtin_amdgcn_readfirstlane(w)];
        li = __builtin_amdgcn_readfirstlane((pc >> 8) & 255);
        nl = a.nload;
    }
    if (NWV == 8 ? w == 7 : __builtin_amdgcn_readfirstlane(pc >> 16) == CD_NONE) {
        // ---- loader: E_k -> El in 16-byte units, gathered from the core (chain_e_fill_gather) or copied from its packed image.
        // levelled workgroups: the loader is the youngest of three waves on its SIMD and the arbiter serves the oldest
        // first -- left at that it issues one load per ~300 cycles and E_k lands after phase A is over
        if constexpr (NWV != 8) __builtin_amdgcn_s_setprio(3);
#ifdef TTSK_LAB
        if (CF_DIAG(8)) {                              // one loader, the other spare waves leave
            if (li > 0) { __syncthreads(); return; }
            nl = 1;
        }
#endif
        const int NI = CF_DIAG(2) ? 0 : a.eunits >> 6;
        const uint32_t inv = e_image_inv(A2P);
        const int64_t rowstride = (int64_t)a.n * a.A2;
        const int ebuf = a.eunits * 2;                 // doubles per E image
        auto fill_gather = [&](int k) {                // (A2 is even here: no odd-rank rule)
            chain_e_fill_gather<false>(a, El + (EBUF == 2 ? (k & 1) * ebuf : 0), k, 0, A2P, inv, rowstride, NI, li, nl, lane);
        };
        // A packed core (chain_pack.hip) holds the image itself: piece m of slice k is 1 KB at Epk + (k eunits + 64 m) units,
        // a wave-uniform base that moves by a constant per instruction under the lane's fixed 16 bytes -- no division,
        // no clamp, no 64-bit product, and every instruction reads 1 KB of consecutive memory instead of 2 x 16 pieces
        // of 16 bytes from two rows 160 KB apart.  (Stamps: a loader wave still needs ~650 cycles per instruction -- the
        // arithmetic was not what bounds it -- so all spare waves stay loaders: one alone lands E_k 3.6 k cycles late.)
        const uint32_t lane16 = 16u * (uint32_t)lane;
        auto fill_packed = [&](int k) {
            const char *src = (const char *)(a.Epk + ((int64_t)k * a.eunits + 64 * li) * 2);
            double *dst = El + (EBUF == 2 ? (k & 1) * ebuf : 0);
#pragma unroll 2
            for (int m = li; m < NI; m += nl, src += 1024 * nl)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + lane16),
                                                 (__attribute__((address_space(3))) void *)(dst + m * 128), 16, 0, 0);
        };
        const bool packed = a.Epk != nullptr;          // wave-uniform (a kernel argument)
        auto fill = [&](int k) {
            if (packed) fill_packed(k);
            else fill_gather(k);
        };
        __syncthreads();                               // W staged (all waves)
        if constexpr (EBUF == 2) {
            // two images: E_{k+1} travels while the others are in phase B of slice k and phase A of k + 1
            // (short phases -- small ranks -- would otherwise wait for the load at every B1)
            if (k_beg < k_end) fill(k_beg);
            for (int k = k_beg; k < k_end; ++k) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                CF_STAMP(1);
                CF_BARRIER();                          // B1: E_k is in LDS
                CF_STAMP(2);
                if (k + 1 < k_end) fill(k + 1);        // image (k + 1) & 1 was last read in phase B of slice k - 1
                CF_STAMP(3);
                CF_BARRIER();                          // B2
                CF_STAMP(4);
            }
        } else {
            for (int k = k_beg; k < k_end; ++k) {
                CF_STAMP(0);
                fill(k);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                CF_STAMP(1);
                CF_BARRIER();                          // B1: E_k is in LDS, phase A of slice k is done
                CF_STAMP(2);
                CF_STAMP(3);
                CF_BARRIER();                          // B2: phase B of slice k is done, El may be overwritten
                CF_STAMP(4);
            }
        }
        return;
    }
    __syncthreads();                                   // W staged
    if constexpr (NWV == 8) {
        if (w >= (a.J + 15) >> 4) return;              // no rows for this wave (a finished wave leaves the barrier count)
        cf_piece<NQF, STRQ, NNF, STRN, D, WT, EBUF, UNR, CD_WHOLE>(a, Wl, El, w, 0, prob, g, k_beg, k_end, KB1, w, lane);
    } else {
        // each kind of piece is a body of its own with static tile counts
        const int kind = __builtin_amdgcn_readfirstlane(pc >> 16), tile = __builtin_amdgcn_readfirstlane(pc & 255);
        constexpr int H = cd_cut(NQF), APC = 16 * NQF + 4 * STRQ;   // a.AP
        if (kind == CD_WHOLE)
            cf_piece<NQF, STRQ, NNF, STRN, D, WT, EBUF, UNR, CD_WHOLE, APC>(a, Wl, El, tile, 0, prob, g, k_beg, k_end, KB1, w, lane);
        else if (kind == CD_FIRST)
            cf_piece<H, 0, NNF, STRN, D, WT, EBUF, UNR, CD_FIRST, APC>(a, Wl, El, tile, 0, prob, g, k_beg, k_end, KB1, w, lane);
        else if (kind == CD_REST)
            cf_piece<NQF - H, STRQ, NNF, STRN, D, WT, EBUF, UNR, CD_REST, APC>(a, Wl, El, tile, H, prob, g, k_beg, k_end, KB1, w, lane);
        else if (kind == CD_ROWS4)
            cf_rows4<NQF, STRQ, NNF, STRN, D, WT, EBUF, UNR, APC>(a, Wl, El, tile, prob, g, k_beg, k_end, KB1, w, lane);
    }
}

// What the three launchers (chain_fused.hip, chain_wide.hip, chain_sum.hip) do around their kernel with the plan's
// ChainLaunch: request the slab of partial results ...
inline double *chain_slab_request(int stream, const ChainLaunch &l) { return (double *)scratch(stream, SCRATCH_GEMM, (size_t)l.slab * 8 + 64); }

// ... and reduce it into Out[b] (J x A2 contiguous)
inline int chain_slab_reduce(hipStream_t st, const double *slab, const ChainLaunch &l, const ChainStepArgs &c)
{
    RReduceArgs r{l.red_chunks, l.red_m, l.red_n, 1, c.nb, (int64_t)c.J, (int64_t)c.A2, 1, 1.0, 0, {}};
    for (int b = 0; b < c.nb; ++b) r.out.C[b] = c.Out[b];
    return launch_r_reduce(st, slab, r);
}

// 1 = launched (the slab reduce included), 0 = shape not covered, < 0 = error
// cus: the CU budget the launch is planned for (sketch_split.h); 0 = the whole device
int chain_fused_try(const ChainStepArgs &c, int stream, hipStream_t st, bool force = false, int cus = 0);

// chain_pack.hip: the packed image registered for core E with exactly these extents and image layout, or nullptr
const double *drm_packed_lookup(const double *E, int A, int n, int A2, int A2P, int eunits);

}  // namespace ttsk
