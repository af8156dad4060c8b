// Gram matrix of tensor trains: G[p, q] = <A_p, B_q> for K trains A_p and M trains B_q of one shape, each with its own
// ranks (TensorTrain.dot, reference tensor.py:542-557, for all pairs at once; Tensor.error(fast=True), tensor.py:68-72,
// needs three such numbers).  With acc_k (ra_k x rb_k), acc_0 = 1,
//   acc_{k+1}[a', b'] = sum_i A_k[:, i, a']^T acc_k B_k[:, i, b']
// one launch per mode over all pairs, plus one closing launch: d + 1 launches whatever K M is (tt_gram_plan.h).
//
// Launch k.  Workgroup (pair, chunk) of four waves takes a run of the n_k slices of its pair.
//   1. acc_k of the pair into LDS: the chunk partials of launch k - 1 summed in ascending chunk order while they are
//      loaded (the reduce costs no launch; every workgroup of the pair forms the same bits).
//   2. per stage of S slices x TA 16-column tiles of a':
//        T[b, (i, a')]  = sum_a acc[a, b] A[a, i, a']          into LDS
//        part[a', b']  += sum_{b, i} T[b, i, a'] B[b, i, b']   in registers, over all stages of the run
//   3. part to the workgroup's own place in the mode's slab: [pair][chunk][ra' x rb'].
// The closing launch sums the chunk scalars of the last mode in order into G; a last mode of one chunk writes G itself.
// No atomics, and the chunk counts depend on the shapes, K M and the CU count alone: the same bits on every call.
//
// MFMA body (v_mfma_f64_16x16x4; layouts of common.h).  Product 1 is T^T-free: the A operand is acc^T, element
// [m = b][k = a] = acc[a pitch + b] -- the 32 lanes of a half-wave read two k rows of 16 consecutive doubles, `pitch` = 16
// modulo 32 puts them on 32 different even banks -- and the B operand [k = a][n = a'] comes from the core through L2 (16
// lanes one 128-byte row segment).  The accumulator (register r of lane l: row (l >> 4) + 4 r, column l & 15) is T[b][a'],
// stored as tiles of (t_rows x 16) doubles: 64 consecutive doubles per register, and read back as the A operand of
// product 2, [m = a'][k = b] = tile[16 b + a'], 32 consecutive doubles per half-wave: conflict-free both ways.  Operands
// beyond a rank are zeros selected after a clamped load; acc is zero-padded in LDS, so padded rows of T are exact zeros.
// A wave owns the 16-column tiles wave, wave + 4 of b' and keeps TA x 2 accumulators; a B fragment serves TA matrix
// instructions.  Inside the k loops the only vector work beside the matrix instruction is the operand's address step and
// select (an fp64 matrix instruction does not hide a wave's VALU work).
//
// FMA body, for ranks below 16 where a 16-wide tile is mostly padding: the same stages, thread e of the workgroup forms
// element e of T and keeps the sums e, e + 256, ... of part.
#include "common.h"
#include "prof.h"
#include "tt_gram_plan.h"

namespace ttsk {

namespace {

// one train as mode k sees it
struct GramTrain {
    const double *core;          // (r0, n, r1) contiguous
    int r0, r1;
    int pre0, pre1;              // sums of r0 / r1 over the trains of its side before it: where its slabs sit
};

struct GramStep {
    GramTrain t[GRAM_MAX_TRAINS];    // the K trains A, then the M trains B
    const double *in;                // slab of mode k - 1 (nullptr: acc = 1)
    double *out;                     // slab of this mode
    int K, M, n, chunks, chunks_in;
    int sum_b0, sum_b1;              // sums of r0 / r1 over the trains B
    int S, TA, pitch, t_rows, acc_rows;
    unsigned acc_doubles;
};

struct GramPair {
    const double *A, *B;
    const double *in;
    double *out;                     // this workgroup's (ra1 x rb1) block
    int ra, ra1, rb, rb1;
    int64_t i0, i1;                  // its run of slices
};

__device__ __forceinline__ GramPair gram_pair(const GramStep &g)
{
    GramPair w;
    const int pair = blockIdx.x / g.chunks, c = blockIdx.x - pair * g.chunks;
    const int p = pair / g.M, q = pair - p * g.M;
    const GramTrain ta = g.t[p], tb = g.t[g.K + q];
    w.A = ta.core; w.B = tb.core;
    w.ra = ta.r0; w.ra1 = ta.r1; w.rb = tb.r0; w.rb1 = tb.r1;
    w.in = g.in ? g.in + (int64_t)g.chunks_in * ((int64_t)ta.pre0 * g.sum_b0 + (int64_t)ta.r0 * tb.pre0) : nullptr;
    w.out = g.out + (int64_t)g.chunks * ((int64_t)ta.pre1 * g.sum_b1 + (int64_t)ta.r1 * tb.pre1) + (int64_t)c * ta.r1 * tb.r1;
    w.i0 = (int64_t)c * g.n / g.chunks;
    w.i1 = (int64_t)(c + 1) * g.n / g.chunks;
    return w;
}

// acc of the pair into LDS, rows x cols as laid out (zeros beyond ra x rb): the partials of the previous launch added in
// ascending chunk order
__device__ __forceinline__ void gram_load_acc(const GramStep &g, const GramPair &w, int rows, int cols, double *accs)
{
    const int cells = w.ra * w.rb;
    for (int e = threadIdx.x; e < rows * cols; e += 256) {
        const int a = e / cols, b = e - a * cols;
        double v = 0.0;
        if (a < w.ra && b < w.rb) {
            if (!w.in) v = 1.0;
            else {
                const double *s = w.in + a * w.rb + b;
                for (int c = 0; c < g.chunks_in; ++c) v += s[(int64_t)c * cells];
            }
        }
        accs[a * g.pitch + b] = v;
    }
}

__global__ __launch_bounds__(256) void tt_gram_mfma_kernel(GramStep g)
{
    extern __shared__ double gram_sm[];
    double *const accs = gram_sm, *const Ts = gram_sm + g.acc_doubles;
    const int tid = threadIdx.x, lane = tid & 63, x16 = lane & 15, kq = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const GramPair w = gram_pair(g);
    const int ra = w.ra, ra1 = w.ra1, rb = w.rb, rb1 = w.rb1;
    const int nbt = (rb + 15) >> 4, nat = (ra1 + 15) >> 4, nb1t = (rb1 + 15) >> 4, k1 = (ra + 3) >> 2, k2 = (rb + 3) >> 2;
    gram_load_acc(g, w, k1 * 4, nbt * 16, accs);
    __syncthreads();
    const int64_t astr = (int64_t)g.n * ra1, bstr = (int64_t)g.n * rb1;
    const size_t tile = (size_t)g.t_rows * 16;

    for (int at0 = 0; at0 < nat; at0 += g.TA) {
        const int tan = nat - at0 < g.TA ? nat - at0 : g.TA;
        v4d P[GRAM_MAX_STAGE_TILES][2];
#pragma unroll
        for (int at = 0; at < GRAM_MAX_STAGE_TILES; ++at)
#pragma unroll
            for (int j = 0; j < 2; ++j) P[at][j] = v4d{0.0, 0.0, 0.0, 0.0};

        for (int64_t is = w.i0; is < w.i1; is += g.S) {
            const int sn = w.i1 - is < g.S ? (int)(w.i1 - is) : g.S, J = sn * tan;
            // ---- T = acc^T A over the stage: tile jobs (row tile of b, slice, column tile of a') dealt over the waves
            for (int job = wave; job < nbt * J; job += 4) {
                const int bt = job / J, j = job - bt * J, s = j / tan, at = j - s * tan;
                const int a1 = (at0 + at) * 16 + x16;
                const bool cok = a1 < ra1;
                const double *Ap = w.A + (is + s) * ra1 + (cok ? a1 : ra1 - 1);
                const double *af = accs + kq * g.pitch + bt * 16 + x16;
                v4d t = v4d{0.0, 0.0, 0.0, 0.0};
                // four k-blocks of the core in flight under the four matrix instructions before them
                auto core_a = [&](int ks) {
                    const int a = 4 * (ks < k1 ? ks : k1 - 1) + kq;
                    const double v = Ap[(int64_t)(a < ra ? a : ra - 1) * astr];
                    return cok && a < ra ? v : 0.0;
                };
                double cur[4], nxt[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) cur[u] = core_a(u);
                for (int ks = 0; ks < k1; ks += 4) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) nxt[u] = core_a(ks + 4 + u);
#pragma unroll
                    for (int u = 0; u < 4; ++u)
                        if (ks + u < k1) t = mfma16(LDS_UNPAIRED(af[4 * (ks + u) * g.pitch]), cur[u], t);
#pragma unroll
                    for (int u = 0; u < 4; ++u) cur[u] = nxt[u];
                }
                double *To = Ts + (size_t)j * tile + (size_t)(bt * 16 + kq) * 16 + x16;
#pragma unroll
                for (int r = 0; r < 4; ++r) To[64 * r] = t[r];
            }
            __syncthreads();
            // ---- part += T^T B: the wave's column tiles of b'
            for (int s = 0; s < sn; ++s) {
                const double *Bp[2];
                bool bok[2];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int b1 = (wave + 4 * j) * 16 + x16;
                    bok[j] = wave + 4 * j < nb1t && b1 < rb1;
                    Bp[j] = w.B + (is + s) * rb1 + (bok[j] ? b1 : 0);
                }
                const double *Tf = Ts + (size_t)(s * tan) * tile + kq * 16 + x16;
                const bool two = wave + 4 < nb1t;
                if (wave < nb1t) {
                    // the next k-block of the core in flight under this one's matrix instructions
                    auto core_b = [&](int ks, double &b0, double &b1v) {
                        const int b = 4 * (ks < k2 ? ks : k2 - 1) + kq;
                        const bool rok = b < rb;
                        const int64_t bo = (int64_t)(rok ? b : rb - 1) * bstr;
                        const double v0 = Bp[0][bo], v1 = two ? Bp[1][bo] : 0.0;
                        b0 = rok && bok[0] ? v0 : 0.0;
                        b1v = rok && bok[1] ? v1 : 0.0;
                    };
                    double b0, b1v, n0, n1;
                    core_b(0, b0, b1v);
                    for (int ks = 0; ks < k2; ++ks) {
                        core_b(ks + 1, n0, n1);
#pragma unroll
                        for (int at = 0; at < GRAM_MAX_STAGE_TILES; ++at) {
                            if (at < tan) {
                                const double tf = LDS_UNPAIRED(Tf[(size_t)at * tile + 64 * ks]);
                                P[at][0] = mfma16(tf, b0, P[at][0]);
                                if (two) P[at][1] = mfma16(tf, b1v, P[at][1]);
                            }
                        }
                        b0 = n0; b1v = n1;
                    }
                }
            }
            __syncthreads();
        }
        // ---- the (a' tile rows) x (b' tile columns) of part this wave holds
#pragma unroll
        for (int at = 0; at < GRAM_MAX_STAGE_TILES; ++at)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int b1 = (wave + 4 * j) * 16 + x16;
                if (at < tan && wave + 4 * j < nb1t && b1 < rb1)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int a1 = (at0 + at) * 16 + kq + 4 * r;
                        if (a1 < ra1) w.out[(int64_t)a1 * rb1 + b1] = P[at][j][r];
                    }
            }
    }
}

__global__ __launch_bounds__(256) void tt_gram_fma_kernel(GramStep g)
{
    extern __shared__ double gram_sm[];
    double *const accs = gram_sm, *const Ts = gram_sm + g.acc_doubles;
    const int tid = threadIdx.x;
    const GramPair w = gram_pair(g);
    const int ra = w.ra, ra1 = w.ra1, rb = w.rb, rb1 = w.rb1, cells = ra1 * rb1;
    gram_load_acc(g, w, ra, rb, accs);
    __syncthreads();
    const int64_t astr = (int64_t)g.n * ra1, bstr = (int64_t)g.n * rb1;
    constexpr int PER = GRAM_FMA_CELLS / 256;
    double P[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) P[j] = 0.0;
    for (int64_t is = w.i0; is < w.i1; is += g.S) {
        const int sn = w.i1 - is < g.S ? (int)(w.i1 - is) : g.S;
        for (int e = tid; e < sn * rb * ra1; e += 256) {             // T[(s, b)][a']
            const int sb = e / ra1, a1 = e - sb * ra1, s = sb / rb, b = sb - s * rb;
            const double *Ap = w.A + (is + s) * ra1 + a1;
            double v = 0.0;
#pragma unroll 4
            for (int a = 0; a < ra; ++a) v = fma(accs[a * g.pitch + b], Ap[a * astr], v);
            Ts[e] = v;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int e = tid + 256 * j;
            if (e < cells) {
                const int a1 = e / rb1, b1 = e - a1 * rb1;
                double v = P[j];
                for (int s = 0; s < sn; ++s) {
                    const double *Bp = w.B + (is + s) * rb1 + b1;
                    const double *Tp = Ts + (size_t)s * rb * ra1 + a1;
#pragma unroll 4
                    for (int b = 0; b < rb; ++b) v = fma(Tp[b * ra1], Bp[b * bstr], v);
                }
                P[j] = v;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < PER; ++j)
        if (tid + 256 * j < cells) w.out[tid + 256 * j] = P[j];
}

// G[pair] = sum_c slab[pair][c], ascending
__global__ __launch_bounds__(256) void tt_gram_close_kernel(const double *__restrict__ slab, int chunks, int64_t pairs, double *__restrict__ G)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= pairs) return;
    double v = 0.0;
    for (int c = 0; c < chunks; ++c) v += slab[e * chunks + c];
    G[e] = v;
}

}  // namespace

}  // namespace ttsk

using namespace ttsk;

extern "C" {

int ttsk_tt_gram(const double *const *dev_cores_a, const int64_t *ranks_a, int K, const double *const *dev_cores_b,
                 const int64_t *ranks_b, int M, const int64_t *shape, int d, double *dev_out, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(dev_cores_a && dev_cores_b && dev_out, "ttsk_tt_gram: NULL cores or output");
    const int n_cu = device_num_cu();
    if (n_cu < 1) return TTSK_ERR_HIP;
    GramPlan p;
    int rc = gram_plan(ranks_a, ranks_b, shape, d, K, M, n_cu, &p);
    if (rc) { set_error("%s", p.msg); return rc; }
    for (int i = 0; i < K * d; ++i) TTSK_ARG(dev_cores_a[i], "ttsk_tt_gram: core %d of train %d of side 0 is NULL", i % d, i / d);
    for (int i = 0; i < M * d; ++i) TTSK_ARG(dev_cores_b[i], "ttsk_tt_gram: core %d of train %d of side 1 is NULL", i % d, i / d);
    char *ws = (char *)scratch(stream, SCRATCH_MISC, p.scratch);
    if (!ws) return TTSK_ERR_HIP;
    GramStep g{};
    g.K = K; g.M = M;
    for (int k = 0; k < d; ++k) {
        const GramModePlan &m = p.m[k];
        int pre0 = 0, pre1 = 0;
        double sa01 = 0.0, sa1 = 0.0, sb01 = 0.0;
        for (int t = 0; t < K + M; ++t) {
            if (t == K) { sa1 = pre1; pre0 = pre1 = 0; }
            const int64_t *rk = t < K ? ranks_a + (size_t)t * (d + 1) : ranks_b + (size_t)(t - K) * (d + 1);
            GramTrain &T = g.t[t];
            T.core = t < K ? dev_cores_a[(size_t)t * d + k] : dev_cores_b[(size_t)(t - K) * d + k];
            T.r0 = (int)rk[k]; T.r1 = (int)rk[k + 1];
            T.pre0 = pre0; T.pre1 = pre1;
            pre0 += T.r0; pre1 += T.r1;
            (t < K ? sa01 : sb01) += (double)T.r0 * T.r1;
        }
        g.sum_b0 = pre0; g.sum_b1 = pre1;
        // sum over the pairs of 2 n (ra rb ra' + ra' rb rb')
        const double flops = 2.0 * (double)shape[k] * (sa01 * pre0 + sa1 * sb01);
        const bool last = k == d - 1;
        g.in = k ? (const double *)(ws + p.m[k - 1].slab_off) : nullptr;
        g.out = last && p.fold_last ? dev_out : (double *)(ws + m.slab_off);
        g.n = (int)shape[k]; g.chunks = m.chunks; g.chunks_in = k ? p.m[k - 1].chunks : 1;
        g.S = m.S; g.TA = m.TA; g.pitch = m.pitch; g.t_rows = m.t_rows; g.acc_rows = m.acc_rows;
        g.acc_doubles = (unsigned)m.acc_doubles;
        const bool mfma = m.body == GRAM_BODY_MFMA;
        ProfBracket prof(st, PROF_EVAL, flops, mfma ? "tt_gram_mfma_kernel" : "tt_gram_fma_kernel");
        if ((rc = launch(mfma ? tt_gram_mfma_kernel : tt_gram_fma_kernel, dim3((unsigned)(p.pairs * m.chunks)), dim3(256), m.lds, st, g)))
            return rc;
    }
    if (!p.fold_last) {
        ProfBracket prof(st, PROF_EVAL, (double)p.pairs * p.m[d - 1].chunks, "tt_gram_close_kernel");
        return launch(tt_gram_close_kernel, dim3((unsigned)cdiv(p.pairs, 256)), dim3(256), 0, st,
                      (const double *)(ws + p.m[d - 1].slab_off), p.m[d - 1].chunks, p.pairs, dev_out);
    }
    return TTSK_OK;
}

}  // extern "C"
