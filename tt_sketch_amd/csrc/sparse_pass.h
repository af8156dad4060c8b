// The pass kernel of sparse_fused.hip: one wave walks its stretch of a mode's stream tile by tile -- (1) records, (2a) table
// rows by LDS-DMA, (2b) sampled factors, (3) tail samples, (2b') rows of tensor-train DRMs by a few chain steps from a table
// row (only in the instantiations with CH), (4) products on the matrix cores -- and stores the slices of Psi
// inside its stretch; its first and last (shared) slices and its Omega go to per-wave partial blocks.  The launch is planned
// by sparse_plan.h, which also owns the wave's LDS layout.
#pragma once
#include <type_traits>
#include "sampler_dev.h"
#include "sparse_plan.h"

namespace ttsk {

struct SgF {
    int kind;            // 0: ones (width 1), 1: table gathered by flat index, 2: normals sampled in the pass, 3: sign rows sampled in the pass,
                         // 4: rows of a tensor-train DRM formed in the pass (SgPass::ch; `table`, `units`, `rcp`: its start rows), and,
                         //    with SgPlanCh::diag, of a Khatri-Rao DRM (kind 5 of ttsk_sg_factor, restated by sg_plan)
    int w;               // columns of the factor (<= 16 NT)
    int rank_min;
    int src;             // flat index: 0 = prefix, 1 = suffix, 2 = prefix + j * mul, 3 = suffix + j * mul
    uint64_t mul, seed;
    const double *table;
    int full, nnz;       // kind 3: length of the whole DRM row ([rank_min, rank_min + w) of it is used), its +-1 entries
    int units, rcp;      // kind 1: SgPlanF
};

struct SgPass {
    const uint64_t *fl, *fr;   // flat prefix / suffix index of every record (w32: arrays of uint32 behind these pointers)
    int w32;
    const int32_t *jj;
    const double *val;
    size_t N, chunk;     // nonzeros, nonzeros per wave (multiple of 32)
    int64_t n;           // slices of Psi
    SgF f[3];            // Psi = (val A) (x) B by slice; Omega = (val C) (x) B  (c_left)  or  (val A) (x) C
    int c_left, has_om;
    int off[3], tcols;   // SgPlanF::off; SgPlan::tcols, tab, qcols
    int tab;
    int qcols;
    double *psi;         // [wA][n][wB]
    double *part_psi;    // [wave][2][wA * wB]
    int *part_j;         // [wave][3]: first slice, last slice (= first if none), 1 if the last partial exists
    double *part_om;     // [wave][wOl * wOr]
    int chain;           // SgPlan::chain, ch; the cores of the chain factors (read by the CH instantiations only)
    SgPlanCh ch[3];
    const double *core[3][SG_CHAIN_MAX];
#ifdef TTSK_LAB
    int lab;             // TTSK_SG_LAB: 1 = no table DMA, 2 = no products, 4 = no sampling (timing experiments; results are wrong)
#endif
};

// ndtri as a CALL in this kernel: inlined at its two sites it takes the pass kernel to ~230 VGPRs (two waves per SIMD,
// or 49 spilled registers under a tighter cap); the call costs a few scalar instructions per ~100 of arithmetic.
__device__ __attribute__((noinline)) double sg_ndtri(double u) { return ndtri_dev(u); }

__device__ __forceinline__ uint64_t sg_flat(const SgF &f, uint64_t fl, uint64_t fr, int j)
{
    const uint64_t base = (f.src & 1) ? fr : fl;
    return (f.src & 2) ? base + (uint64_t)(int64_t)j * f.mul : base;
}

// ---- The accumulators of one product, in two forms with one interface.  Ops: a factor's operands of one k-block (the lane's
// nonzero 4 b + kq, whose row is r); load (`one`: the ones factor), scaled, zero, mac, and store: the cells set to
// dst[row * stride + col] where row < wa and col < wb.  No masks in load or mac: a column beyond a factor's width only reaches
// cells that are never stored, and a nonzero beyond the stretch has val = 0 and finite (stale or zero-initialised) rows.

// NT x NT tiles of 16 x 16: lane (x16, kq) holds column 16 t + x16 of the factor.  EVERY = false skips a tile wholly beyond a
// factor's width (a factor of <= 16 columns beside a wider one).
template <int NT> struct SgTiles {
    struct Ops { double t[NT]; };
    v4d acc[NT][NT];
    static __device__ __forceinline__ Ops load(const double *r, bool one, int x16)
    {
        Ops o;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const double l = r[16 * t + x16];
            o.t[t] = one ? (16 * t + x16 == 0 ? 1.0 : 0.0) : l;
        }
        return o;
    }
    static __device__ __forceinline__ Ops scaled(Ops o, double v)
    {
#pragma unroll
        for (int t = 0; t < NT; ++t) o.t[t] *= v;
        return o;
    }
    __device__ __forceinline__ void zero()
    {
#pragma unroll
        for (int i = 0; i < NT * NT; ++i) acc[i / NT][i % NT] = v4d{0.0, 0.0, 0.0, 0.0};
    }
    template <bool EVERY> __device__ __forceinline__ void mac(const Ops &A, const Ops &B, int wa, int wb)
    {
#pragma unroll
        for (int ta = 0; ta < NT; ++ta)
#pragma unroll
            for (int tb = 0; tb < NT; ++tb)
                if (EVERY || (16 * ta < wa && 16 * tb < wb)) acc[ta][tb] = mfma16(A.t[ta], B.t[tb], acc[ta][tb]);
    }
    __device__ __forceinline__ void store(double *dst, int64_t stride, int wa, int wb, int x16, int kq) const
    {
#pragma unroll
        for (int ta = 0; ta < NT; ++ta)
#pragma unroll
            for (int tb = 0; tb < NT; ++tb)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int aa = 16 * ta + 4 * t + kq, cc = 16 * tb + x16;
                    if (aa < wa && cc < wb) dst[aa * stride + cc] = acc[ta][tb][t];
                }
    }
};

// factors that reach NS 4-wide strips beyond their first 16 columns (NS = 1: <= 20 columns, 2: <= 24): the 16 x 16 tile, NS
// column strips (rows 0..15 x columns 16 + 4 q ..: A as for the tile, B replicated over the four blocks of v_mfma_f64_4x4x4), NS
// row strips (rows 16 + 4 q .. x columns 0..15: A replicated, B as for the tile) and the corner as the same row strips against
// B's second 16 columns.  64 + 3 NS x 16 matrix cycles per four nonzeros instead of the 256 of 2 x 2 tiles (fp64 matrix
// instructions run on the vector ALU's FMA units: padding is paid for).  Per factor and k-block: the tile operand (column x16),
// NS strip operands (column 16 + 4 q + (x16 & 3)) and the second-tile operand (column 16 + x16).
template <int NS> struct SgEdge {
    struct Ops { double t, s[NS], b1; };
    v4d t;
    double sb[NS], sa[NS], c[NS];
    static __device__ __forceinline__ Ops load(const double *r, bool one, int x16)
    {
        Ops o;
        o.t = one ? (x16 == 0 ? 1.0 : 0.0) : r[x16];
        o.b1 = one ? 0.0 : r[16 + x16];
#pragma unroll
        for (int q = 0; q < NS; ++q) o.s[q] = one ? 0.0 : r[16 + 4 * q + (x16 & 3)];
        return o;
    }
    static __device__ __forceinline__ Ops scaled(Ops o, double v)
    {
        o.t *= v;
#pragma unroll
        for (int q = 0; q < NS; ++q) o.s[q] *= v;
        return o;
    }
    __device__ __forceinline__ void zero()
    {
        t = v4d{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int q = 0; q < NS; ++q) { sb[q] = 0.0; sa[q] = 0.0; c[q] = 0.0; }
    }
    template <bool EVERY> __device__ __forceinline__ void mac(const Ops &A, const Ops &B, int, int)
    {
        t = mfma16(A.t, B.t, t);
#pragma unroll
        for (int q = 0; q < NS; ++q) sb[q] = mfma4(A.t, B.s[q], sb[q]);
#pragma unroll
        for (int q = 0; q < NS; ++q) sa[q] = mfma4(A.s[q], B.t, sa[q]);
#pragma unroll
        for (int q = 0; q < NS; ++q) c[q] = mfma4(A.s[q], B.b1, c[q]);
    }
    __device__ __forceinline__ void store(double *dst, int64_t stride, int wa, int wb, int x16, int kq) const
    {
        const int beta = x16 >> 2, j4 = x16 & 3;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int aa = 4 * i + kq;
            if (aa < wa && x16 < wb) dst[aa * stride + x16] = t[i];
        }
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            { const int aa = 4 * beta + kq, cc = 16 + 4 * q + j4; if (aa < wa && cc < wb) dst[aa * stride + cc] = sb[q]; }
            { const int aa = 16 + 4 * q + kq; if (aa < wa && x16 < wb) dst[aa * stride + x16] = sa[q]; }
            { const int aa = 16 + 4 * q + kq, cc = 16 + x16; if (aa < wa && cc < wb) dst[aa * stride + cc] = c[q]; }
        }
    }
};

// where the products read a factor: nonzero e of the tile, column c at p[e * se + c] (p: the row of the lane's kq)
struct SgSrc { const double *p; int se; bool one; };

// ---- One wave's walk.  NT: 16-column matrix tiles per factor (NT = 1: every factor <= 16 columns, C4; NT = 2: up to 32, two
// waves per SIMD).  NS: edge strips, above.  T: nonzeros per staged tile; 16 where three wide factors would leave room for ONE
// workgroup per CU (sg_plan): the sampling stage then deals CP = 4 columns of a nonzero over the wave instead of 2.  CH: the
// pass has a chain factor (stage 2b'); without, none of that stage's code is in the kernel.
template <int NT, int NS, int T, bool CH> struct SgWave {
    static constexpr int CP = 64 / T;
    using Acc = std::conditional_t<(NS > 0), SgEdge<(NS > 0 ? NS : 1)>, SgTiles<NT>>;
    using Ops = typename Acc::Ops;
    const SgPass &a;
    const uint64_t (*salt)[16 * NT];
    int lane, x16, kq, t32, half;                      // t32, half: (nonzero of the tile, which of its CP column slots)
    double *tile, *tabs, *rv;
    uint64_t *ro;
    int *rj, *pj;
    unsigned short *q;
    double *cv;                                        // CH: the running vectors of the chains, the digits of the tile's nonzeros
    uint32_t *cd;
    size_t w_id, beg, end;
    int wA, wB, wOl, wOr;
    int jfirst, cur;
    bool first_done;
    Acc P, O;
    uint64_t my_fl, my_fr, nx_fl, nx_fr;               // the records of this tile and of the next, which travel meanwhile
    int my_j, nx_j;
    double nx_v;
    bool valid;

    // false: a padding wave of the last workgroup, which has written nothing but zeros for the sums
    __device__ __forceinline__ bool setup(double *lds)
    {
        lane = threadIdx.x & 63, x16 = lane & 15, kq = lane >> 4, t32 = lane & (T - 1), half = lane / T;
        const SgLds L = sg_lds_layout(a.tcols, a.tab, a.qcols, T, CH ? a.chain : 0);
        double *base = lds + (size_t)(threadIdx.x >> 6) * L.total;
        tile = base + L.tile; tabs = base + L.tabs; ro = (uint64_t *)(base + L.ro); rv = base + L.rv;
        rj = (int *)(base + L.rj); q = (unsigned short *)(base + L.q);
        if constexpr (CH) { cv = base + L.cv; cd = (uint32_t *)(base + L.cd); }
        // (finite values everywhere a product may read: the rows of nonzeros beyond the stretch are multiplied by val = 0)
        for (int i = lane; i < T * a.tcols + a.tab; i += 64) tile[i] = 0.0;
        w_id = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
        beg = w_id * a.chunk;
        wA = a.f[0].w, wB = a.f[1].w;
        wOl = a.c_left ? a.f[2].w : wA, wOr = a.c_left ? wB : a.f[2].w;
        pj = a.part_j + w_id * 3;
        if (beg >= a.N) {
            if (lane == 0) { pj[0] = 0x7fffffff; pj[1] = 0x7fffffff; pj[2] = 0; }
            if (a.has_om)
                for (int t = lane; t < wOl * wOr; t += 64) a.part_om[w_id * (size_t)(wOl * wOr) + t] = 0.0;
            return false;
        }
        end = beg + a.chunk < a.N ? beg + a.chunk : a.N;
        cur = jfirst = a.jj ? a.jj[beg] : 0;
        first_done = false;
        P.zero();
        O.zero();
        if (lane == 0) { pj[0] = jfirst; pj[1] = jfirst; pj[2] = 0; }
        rec_load(beg);
        return true;
    }

    __device__ __forceinline__ void rec_load(size_t t0)
    {
        const size_t pos = t0 + t32;
        const bool in = pos < end;
        if (a.w32) {
            nx_fl = (in && a.fl) ? ((const uint32_t *)a.fl)[pos] : 0;
            nx_fr = (in && a.fr) ? ((const uint32_t *)a.fr)[pos] : 0;
        } else {
            nx_fl = (in && a.fl) ? a.fl[pos] : 0;
            nx_fr = (in && a.fr) ? a.fr[pos] : 0;
        }
        nx_j = in ? (a.jj ? a.jj[pos] : 0) : -1;
        nx_v = in ? a.val[pos] : 0.0;
    }

    // (1) of the chain factors, by the lane of the nonzero: its digits (sg_chain_digits) and where its start row begins (a
    // missing nonzero: row 0 and digits 0, as for the tables)
    __device__ __forceinline__ void chain_records()
    {
#pragma unroll 1
        for (int f = 0; f < 3; ++f) {
            if (a.f[f].kind != 4) continue;
            const SgPlanCh &c = a.ch[f];
            const uint32_t flat = valid ? (uint32_t)((a.f[f].src & 1) ? my_fr : my_fl) : 0u;
            const uint32_t row = sg_chain_digits(c, flat, (a.f[f].src & 2) != 0, valid ? (uint32_t)my_j : 0u, cd + c.doff * T + lane, T);
            if (c.has_table) ro[f * T + lane] = (uint64_t)row * (uint64_t)(8 * c.rank[0]);
        }
    }

    // (1) the records of the tile at t0 into LDS, those of the next one on their way; true: the whole tile belongs to the
    // running slice
    __device__ __forceinline__ bool records(size_t t0)
    {
        my_fl = nx_fl, my_fr = nx_fr, my_j = nx_j;
        valid = my_j >= 0;
        if (lane < T) {
#pragma unroll
            for (int f = 0; f < 3; ++f)                // where the nonzero's row of table factor f starts (a missing nonzero: row 0)
                if (a.f[f].kind == 1) ro[f * T + lane] = valid ? sg_flat(a.f[f], my_fl, my_fr, my_j) * (uint64_t)(8 * a.f[f].w) : 0;
            rv[lane] = nx_v;
            rj[lane] = my_j;
            if constexpr (CH) chain_records();
        }
        const bool one_slice = __ballot(valid && my_j != cur) == 0ull;
        rec_load(t0 + T);
        __builtin_amdgcn_wave_barrier();
        return one_slice;
    }

    // (2a) the table factors: row flat[t] of the table into a block [t][2 units] by LDS-DMA, 16 bytes per lane (unit
    // i = 64 k + lane of the block in instruction k: nonzero i / units, unit i % units of its row), no registers held: the rows
    // of ALL table factors travel while the sampled factors are evaluated, and are waited for once, in front of the
    // products.  (A register gather paid one round trip per table factor; dword DMAs, one per column, were bound by the
    // address unit: 40 instructions per tile at C4 against 7 now.)  An odd row's last unit reads 8 bytes of the next row (the
    // table has a spare row behind its last one); rows are 8-byte aligned only.
    __device__ __forceinline__ void table_dma()
    {
#pragma unroll 1
        for (int f = 0; f < 3; ++f) {
            const SgF &F = a.f[f];
            const bool start = CH && F.kind == 4 && a.ch[f].has_table;       // the start rows of a chain factor, as a table of rank[0] columns
            if (F.kind != 1 && !start) continue;
#ifdef TTSK_LAB
            if (a.lab & 1) continue;
#endif
            double *blk = tabs + (start ? a.ch[f].toff : a.off[f]);
#pragma unroll 1
            for (int i0 = 0; i0 < T * F.units; i0 += 64) {
                const int i = i0 + lane;
                const int t = sg_div_units(i, F.rcp), cu = i - t * F.units;
                if (t < T) {
                    const char *src = (const char *)F.table + ro[f * T + t] + 16 * cu;
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                                     (__attribute__((address_space(3))) void *)(blk + 2 * i0), 16, 0, 0);
                }
            }
        }
    }

    // (2b) normals: CP columns of every nonzero side by side; the central branch of ndtri in place (inline: no call, and no
    // wait for the DMA, in this stage), a tail sample's uniform is left in its slot and the slot queued behind the qn so far
    __device__ __forceinline__ int sample_normals(int f, int qn)
    {
        const SgF &F = a.f[f];
        const uint64_t flat = sg_flat(F, my_fl, my_fr, my_j);
        for (int ci = 0; CP * ci < F.w; ++ci) {                 // the same trip count in every part: the ballots below are wave-wide
            const int c = CP * ci + half;
            const bool act = valid && c < F.w;
            const double u = mant_unit(force_exponent(mix64(flat + salt[f][c & (16 * NT - 1)])));
            const int slot = t32 * a.tcols + a.off[f] + c;
            const bool central = nd_central(u);
            const bool tail = act && !central;
            if (act && central) tile[slot] = ndtri_central_dev(u);
            const unsigned long long m = __ballot(tail);
            if (tail) {
                tile[slot] = u;
                q[qn + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)slot;
            }
            qn += __popcll(m);
        }
        return qn;
    }

    // (2b) a sparse-sign row (fast_lazy_gaussian.pyx:121-180, as sign_kernel of sampler.hip): +-1 at the first nnz positions
    // of a row of `full` zeros, then nnz swaps in order.  The whole row lives in the tile, at columns off - rank_min ..; the
    // products read [off, off + w).  Signs by all CP parts, the swaps by one lane per nonzero.
    __device__ __forceinline__ void sample_signs(int f)
    {
        const SgF &F = a.f[f];
        const uint64_t flat = sg_flat(F, my_fl, my_fr, my_j);
        double *row = tile + t32 * a.tcols + (a.off[f] - F.rank_min);
        for (int c = half; c < F.full; c += CP)
            row[c] = c < F.nnz ? (double)sign_entry(force_exponent(mix64(flat + salt[f][c]))) : 0.0;
        __builtin_amdgcn_wave_barrier();
        if (half == 0)
            for (int c = 0; c < F.nnz; ++c) {
                const int pick = swap_pick(mant_unit(force_exponent(mix64(flat + salt[f][c]))), c, F.full);
                const double x = row[c], y = row[pick];
                row[c] = y;
                row[pick] = x;
            }
    }

    // (2b) the sampled factors into the tile; returns the length of the tail queue
    __device__ __forceinline__ int sample()
    {
        int qn = 0;
#pragma unroll 1
        for (int f = 0; f < 3; ++f) {
#ifdef TTSK_LAB
            if (a.lab & 4) continue;
#endif
            if (a.f[f].kind == 2) qn = sample_normals(f, qn);
            else if (a.f[f].kind == 3) sample_signs(f);
        }
        __builtin_amdgcn_wave_barrier();
        return qn;
    }

    // (3) the tail samples, a full wave at a time
    __device__ __forceinline__ void drain_tails(int qn)
    {
        for (int i = 0; i < qn; i += 64)
            if (i + lane < qn) {
                const int slot = q[i + lane];
                tile[slot] = sg_ndtri(tile[slot]);
            }
    }

    // (2b') the rows of a chain factor, as tt_gather_kernel walks a train: the wave in groups of G = 16 lanes (32 beyond rank
    // 16), a group takes the tile's nonzeros grp, grp + 64 / G, ... one after the other.  The running vector of a nonzero
    // starts as its row of the start table (landed with the table blocks; without a table: the vector (1)) and alternates
    // between the group's two LDS vectors; in a step lane b forms out[b] = sum_a v[a] D[a, i, b], a ascending, every a one
    // contiguous row of the core through L2.  The last step keeps the columns [lo, lo + w) and writes them where the products
    // read the factor.
    __device__ __forceinline__ void chain_factor(int f)
    {
        const SgF &F = a.f[f];
        const SgPlanCh &c = a.ch[f];
        const int G = 1 << c.gsh, lg = lane & (G - 1), grp = lane >> c.gsh, groups = 64 >> c.gsh;
        double *const va = cv + grp * 2 * SG_CHAIN_RANK, *const vb = va + SG_CHAIN_RANK;
        const uint32_t *dg = cd + c.doff * T;
#pragma unroll 1
        for (int e = grp; e < T; e += groups) {                 // T / groups trips in every group
            double *row = tile + e * a.tcols + a.off[f];
            if (c.has_table) {
                const double *src = tabs + c.toff + e * 2 * F.units;
                for (int b = lg; b < c.rank[0]; b += G) va[b] = src[b];
            } else if (lg == 0) {
                va[0] = 1.0;
            }
            double *cur = va, *nxt = vb;
#pragma unroll 1
            for (int s = 0; s < c.steps; ++s) {
                wave_lds_sync();
                const int r = c.rank[s], rn = c.rank[s + 1];
                const bool last = s == c.steps - 1;
                const int64_t as = (int64_t)c.n[s] * rn;
                const double *cp = a.core[f][s] + (int64_t)dg[s * T + e] * rn + (last ? c.lo : 0);
                const int wn = last ? F.w : rn;
                double *out = last ? row : nxt;
                for (int b = lg; b < wn; b += G) {
                    const double *cb = cp + b;
                    double acc = 0.0;
#pragma unroll 4
                    for (int k = 0; k < r; ++k) acc = fma(cur[k], cb[k * as], acc);
                    out[b] = acc;
                }
                double *sw = cur; cur = nxt; nxt = sw;
            }
            wave_lds_sync();
            if (c.steps == 0)
                for (int b = lg; b < F.w; b += G) row[b] = va[c.lo + b];
            wave_lds_sync();                                    // the next nonzero of the group overwrites the vectors
        }
    }

    // (2b') the rows of a Khatri-Rao DRM (kind 5 of ttsk_sg_factor; SgPlanCh::diag): the chain above with diagonal steps.  A
    // column of a nonzero's row depends on no other column, so the T * w (nonzero, column) pairs of the tile are dealt over
    // the 64 lanes, U per lane at a time (their gathers of a step are in flight together), and each is carried in a register
    // from the start row to the tile: no running vectors in LDS, no exchange between lanes; a step gathers one entry of an
    // (n[s], rank) table through L2.  Every step is fma(v, g, +0.0): one
    // rounding, and the bits a kind-4 step gives on the diagonal core of the same table (its other terms are zeros added to
    // a sum that starts at +0.0).
    __device__ __forceinline__ void diag_factor(int f)
    {
        const SgF &F = a.f[f];
        const SgPlanCh &c = a.ch[f];
        const int rho = c.rank[0];
        const uint32_t *dg = cd + c.doff * T;
        wave_lds_sync();                                        // the digits, written by the lanes of their nonzeros
        constexpr int U = 4;                                    // pairs a lane carries at a time: their gathers of a step travel together
        const int items = T * F.w;
#pragma unroll 1
        for (int i0 = lane; i0 < items; i0 += 64 * U) {
            int e[U], col[U];
            double v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int i = i0 + 64 * u < items ? i0 + 64 * u : items - 1;      // (beyond the tile: the last pair once more, not stored)
                e[u] = i / F.w;
                col[u] = c.lo + i - e[u] * F.w;
                v[u] = c.has_table ? tabs[c.toff + e[u] * 2 * F.units + col[u]] : 1.0;
            }
#pragma unroll 1
            for (int s = 0; s < c.steps; ++s) {
                const double *cs = a.core[f][s];
                double g[U];
#pragma unroll
                for (int u = 0; u < U; ++u) g[u] = cs[(int64_t)dg[s * T + e[u]] * rho + col[u]];
#pragma unroll
                for (int u = 0; u < U; ++u) v[u] = fma(v[u], g[u], 0.0);
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (i0 + 64 * u < items) tile[e[u] * a.tcols + a.off[f] + col[u] - c.lo] = v[u];
        }
        wave_lds_sync();                                        // the rows, read by the lanes of the products
    }

    __device__ __forceinline__ void chain()
    {
#pragma unroll 1
        for (int f = 0; f < 3; ++f)
            if (a.f[f].kind == 4) {
                if (a.ch[f].diag) diag_factor(f);
                else chain_factor(f);
            }
    }

    // store the finished slice k: the wave's first slice and (final) its last one go to the partial blocks
    __device__ __forceinline__ void flush(int k, bool final)
    {
        double *dst = a.psi + (size_t)k * wB;
        int64_t stride = (int64_t)a.n * wB;
        if (!first_done && k == jfirst) {
            dst = a.part_psi + (w_id * 2) * (size_t)(wA * wB);
            stride = wB;
            first_done = true;
        } else if (final) {
            dst = a.part_psi + (w_id * 2 + 1) * (size_t)(wA * wB);
            stride = wB;
            if (lane == 0) { pj[1] = k; pj[2] = 1; }
        }
        P.store(dst, stride, wA, wB, x16, kq);
        P.zero();
    }

    __device__ __forceinline__ Ops ld(const SgSrc &s, int b) const { return Acc::load(s.p + 4 * b * s.se, s.one, x16); }

    // Omega of k-block b: (val C) (x) B, or (val A) (x) C
    template <bool CL, bool EVERY> __device__ __forceinline__ void omega(const SgSrc (&s)[3], int b, double v, const Ops &f0, const Ops &f1)
    {
        if constexpr (CL) O.template mac<EVERY>(Acc::scaled(ld(s[2], b), v), f1, wOl, wOr);
        else O.template mac<EVERY>(Acc::scaled(f0, v), ld(s[2], b), wOl, wOr);
    }

    // (4) a tile of the running slice alone (all but one tile in ~10^3 at C4): no slice test per k-block, no masks, nothing
    // but loads and matrix instructions in the loop
    template <bool OM, bool CL, bool EVERY> __device__ __forceinline__ void one_slice_tile(const SgSrc (&s)[3])
    {
        constexpr int UNR = NT == 1 ? 8 : 2;
#pragma unroll UNR
        for (int b = 0; b < T / 4; ++b) {
            const double v = rv[4 * b + kq];
            const Ops f0 = ld(s[0], b), f1 = ld(s[1], b);
            if constexpr (OM) omega<CL, EVERY>(s, b, v, f0, f1);
            P.template mac<EVERY>(Acc::scaled(f0, v), f1, wA, wB);
        }
    }

    // (4) a tile in which slices change: a k-block of one slice as above; otherwise its Omega at once and Psi nonzero by
    // nonzero, the finished slice flushed at every change.  FIXED: the Omega variant is (OM, CL) as in the one-slice loop (the
    // strip form); otherwise the pass's, read here (the tile form).  Psi of a nonzero: the other three of the k-block enter
    // as row * 0.0 (in the one-function kernel the tile form selected a literal 0.0 there, and the strip form first added a
    // Psi product with val = 0 for the whole k-block): the same bits, because the staged rows are finite.
    template <bool FIXED, bool OM, bool CL> __device__ __forceinline__ void mixed_tile(const SgSrc (&s)[3])
    {
#pragma unroll 1
        for (int b = 0; b < T / 4; ++b) {
            const int je = rj[4 * b + kq];
            const bool ok = je >= 0;
            const double v = rv[4 * b + kq];
            const Ops f0 = ld(s[0], b), f1 = ld(s[1], b);
            if constexpr (FIXED) {
                if constexpr (OM) omega<CL, true>(s, b, v, f0, f1);
            } else if (a.has_om) {
                if (a.c_left) omega<true, true>(s, b, v, f0, f1);
                else omega<false, true>(s, b, v, f0, f1);
            }
            if (__ballot(ok && je != cur) == 0ull) {
                P.template mac<true>(Acc::scaled(f0, v), f1, wA, wB);
                continue;
            }
            for (int qq = 0; qq < 4; ++qq) {
                const int okq = __shfl((int)ok, 16 * qq);
                const int jq = __shfl(je, 16 * qq);
                if (!okq) continue;
                if (jq != cur) {
                    flush(cur, false);
                    cur = jq;
                }
                P.template mac<true>(Acc::scaled(f0, kq == qq ? v : 0.0), f1, wA, wB);
            }
        }
    }

    // the compile-time variants of a tile's products: with an Omega or not, its own factor on the left or on the right
    template <bool OM, bool CL, bool EVERY> __device__ __forceinline__ void tile_products(bool one_slice, const SgSrc (&s)[3])
    {
        if (one_slice) one_slice_tile<OM, CL, EVERY>(s);
        else if constexpr (NS > 0) mixed_tile<true, OM, CL>(s);
    }

    template <bool EVERY> __device__ __forceinline__ void tile_variant(bool one_slice, const SgSrc (&s)[3])
    {
        if (!a.has_om) tile_products<false, false, EVERY>(one_slice, s);
        else if (a.c_left) tile_products<true, true, EVERY>(one_slice, s);
        else tile_products<true, false, EVERY>(one_slice, s);
    }

    // (4) the products: k-block b = nonzeros 4 b .. 4 b + 3 of the tile; a factor's rows are in its table block or in the tile
    __device__ __forceinline__ void products(bool one_slice)
    {
        SgSrc s[3];
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            s[f].se = a.f[f].kind == 1 ? 2 * a.f[f].units : a.tcols;
            s[f].p = (a.f[f].kind == 1 ? tabs : tile) + a.off[f] + kq * s[f].se;
            s[f].one = a.f[f].kind == 0;
        }
        s[2].one = false;
        if (NS == 0 && !one_slice) return mixed_tile<false, false, false>(s);
        // (NT = 2 with every factor beyond 16 columns: no tile to skip, no tests in the loop)
        const bool every = NT == 1 || NS > 0 || (wA > 16 && wB > 16 && (!a.has_om || (wOl > 16 && wOr > 16)));
        if (every) tile_variant<true>(one_slice, s);
        else tile_variant<false>(one_slice, s);
    }

    __device__ __forceinline__ void finish()
    {
        flush(cur, true);
        if (a.has_om) O.store(a.part_om + w_id * (size_t)(wOl * wOr), wOr, wOl, wOr, x16, kq);
    }
};

template <int NT, int NS, int T, bool CH = false>
__global__ __launch_bounds__(256, NT == 1 ? 3 : 2) void sg_pass_kernel(SgPass a)
{
    static_assert(NS == 0 || NT == 2, "edge strips belong to the wide instantiation");
    static_assert(T == 32 || T == 16, "tile of 32 or 16 nonzeros");
    extern __shared__ double sg_lds[];
    __shared__ uint64_t salt[3][16 * NT];
    static_assert(sizeof(salt) == sg_salt_bytes(NT), "sg_plan budgets the static LDS");
    const int tid = threadIdx.x;
    if (tid < 48 * NT) {
        const int f = tid / (16 * NT), c = tid % (16 * NT);
        salt[f][c] = mix64((uint64_t)((a.f[f].kind == 3 ? 0 : a.f[f].rank_min) + c)) + a.f[f].seed;
    }
    __syncthreads();                                   // the only workgroup barrier: waves run free from here
    SgWave<NT, NS, T, CH> w{a, salt};
    if (!w.setup(sg_lds)) return;
    for (size_t t0 = w.beg; t0 < w.end; t0 += T) {
        const bool one_slice = w.records(t0);          // (1)
        w.table_dma();                                 // (2a)
        const int qn = w.sample();                     // (2b)
        w.drain_tails(qn);                             // (3)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the table blocks have landed
        __builtin_amdgcn_wave_barrier();
        if constexpr (CH) w.chain();                   // (2b'): the start rows are among the table blocks
#ifdef TTSK_LAB
        if (a.lab & 2) continue;
#endif
        w.products(one_slice);                         // (4)
        __builtin_amdgcn_wave_barrier();
    }
    w.finish();
}

}  // namespace ttsk
