/*
 * ttsk.h -- C ABI of libttsk.so: the MI355X (gfx950) implementation of the
 * streaming TT-sketch hot path of RikVoorhaar/tt-sketch.
 *
 * The reference has exactly one native module (tt_sketch/drm/fast_lazy_gaussian.pyx);
 * everything else on the path is Python plug-in surface (DRM.sketch_* generators and
 * the sketch_omega_* / sketch_psi_* tables).  Each entry point below names the
 * reference interface it replaces (file:line relative to the reference root).
 *
 * Conventions
 *  - every function returns 0 on success or a negative ttsk_status; the message of
 *    the last failure on the calling thread is ttsk_last_error().  No exceptions
 *    cross the boundary.
 *  - "dev" pointers are device addresses obtained from ttsk_malloc; "host" pointers
 *    are ordinary process memory.  The library never keeps or frees host pointers.
 *  - all floating point data is fp64; index data is int64 (as the reference stores
 *    it) unless stated; hashes are uint64.
 *  - calls are asynchronous on the library's stream `stream` (0..TTSK_NUM_STREAMS-1)
 *    unless they take host pointers, in which case they block until the data is valid.
 */
#ifndef TTSK_H
#define TTSK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    TTSK_OK = 0,
    TTSK_ERR_HIP = -1,      /* a HIP runtime call failed (no device, OOM, launch failure) */
    TTSK_ERR_ARG = -2,      /* invalid argument (shape / stride / NULL) -> Python ValueError */
    TTSK_ERR_UNSUPPORTED = -3,
    TTSK_ERR_COMM = -4      /* RCCL failure */
} ttsk_status;

#define TTSK_NUM_STREAMS 8

/* ---- runtime ------------------------------------------------------------ */
int ttsk_init(int device);                    /* selects the device, creates streams; idempotent */
int ttsk_shutdown(void);
const char *ttsk_last_error(void);
int ttsk_device_info(char *name, size_t name_len, int *num_cu, size_t *hbm_bytes);
int ttsk_malloc(void **dev, size_t bytes);
int ttsk_free(void *dev);
int ttsk_memset(void *dev, int value, size_t bytes, int stream);
int ttsk_h2d(void *dev, const void *host, size_t bytes, int stream);   /* blocking */
int ttsk_d2h(void *host, const void *dev, size_t bytes, int stream);   /* blocking */
int ttsk_d2d(void *dst, const void *src, size_t bytes, int stream);
int ttsk_sync(int stream);                    /* stream < 0: all streams */
int ttsk_stream_wait(int waiter, int signaller); /* waiter waits for work queued so far on signaller */
/* hipEvent timing on a library stream (bench.py roofline leg) */
int ttsk_timer_start(int stream);
int ttsk_timer_stop(int stream, float *ms);   /* blocks until the stop event completes */
/* hipGraph capture of a launch sequence on one stream (launch-bound inner loops) */
int ttsk_graph_begin(int stream);
int ttsk_graph_end(int stream, void **graph_exec);
int ttsk_graph_launch(void *graph_exec, int stream);
int ttsk_graph_free(void *graph_exec);

/* ---- generic fp64 contraction (MFMA 16x16x4) -----------------------------
 * C[b,m,n] (+)= alpha * sum_{ko,ki} A[b,m,ko,ki] * B[b,ko,ki,n]
 * with arbitrary element strides.  batch > 1 needs c_b != 0 (TTSK_ERR_ARG otherwise).  This is the device counterpart of the
 * np.einsum / tensordot / `@` calls in tt_sketch/drm/tensor_train_drm.py:79-141,
 * tt_sketch/drm/dense_gaussian_drm.py:72-75, tt_sketch/tensor.py:390-397 and
 * tt_sketch/sketching_methods/{tensor_train,cp,dense,tucker}_sketch.py.
 * Optional row scaling of A by a vector (sparse_sketch.py:46, `left * entries`). */
typedef struct {
    int64_t batch, M, N, Ko, Ki;
    int64_t a_b, a_m, a_ko, a_ki;    /* element strides of A */
    int64_t b_b, b_ko, b_ki, b_n;    /* element strides of B */
    int64_t c_b, c_m, c_n;           /* element strides of C */
    double alpha;
    int accumulate;                  /* 0: C = ..., 1: C += ... */
    int split_k;                     /* 0: library chooses; >=1 explicit */
} ttsk_gemm_desc;
int ttsk_gemm(const ttsk_gemm_desc *desc, const double *A, const double *B, double *C,
              const double *k_scale /* NULL or length Ko*Ki, multiplies A along k */,
              int stream);
/* The three vector entry points; their checks, routes and grids are the host plans of csrc/vector_plan.h.
 *
 * strided copy / permute (<= 5 dims): dst[i0..i4] = src[i0..i4], strides in elements; Tensor.T materialisation.
 * The 8 bytes of an element are moved unchanged (NaN payloads, signalling NaNs, -0.0, subnormals).  A source stride of 0 is
 * a broadcast read.  dst must not overlap src and must address each element once: elements are written in no stated order.
 * Nothing but the addressed elements of dst is written.  TTSK_ERR_ARG: ndim outside 0 .. 5; shape or strides NULL with
 * ndim > 0; a negative extent; dst or src NULL with elements to copy.  TTSK_ERR_UNSUPPORTED: a product of the extents that
 * int64_t cannot hold (with one grid stride of 2^20 to spare).  An extent of 0 is TTSK_OK with no launch, NULL dst and src
 * allowed.  A refused call launches nothing and writes nothing. */
int ttsk_copy_strided(double *dst, const double *src, int ndim, const int64_t *shape,
                      const int64_t *dst_strides, const int64_t *src_strides, int stream);
/* y[i] = a*x[i] + b*y[i] on contiguous buffers: SketchContainer.__add__
 * (sketch_container.py:61-69) and the TensorSum accumulators (sketch_dispatch.py:93-136).
 * b == 0 (either sign) does not read y: y[i] = a*x[i] whatever y held, NaN and inf included, so y may be uninitialised.
 * x == y is allowed (an element is read and written by one thread); any other overlap is not.  a*x + b*y may or may not be
 * contracted into a fused multiply-add.  TTSK_ERR_ARG: y or x NULL with n > 0; n == 0 is TTSK_OK with no launch. */
int ttsk_axpby(double *y, const double *x, double a, double b, size_t n, int stream);
/* dst[i] (+)= sum_{b<nb} src[b*stride + i], i < n: the partial sketches of a batch summed into one
 * (the `+=` loop of sum_sketch, sketch_dispatch.py:141-147); 16-byte loads when n and stride are even and the
 * bases 16-byte aligned, 8-byte loads otherwise -- the same sums either way.
 * The order is fixed: the accumulator starts from dst[i] with accumulate = 1 and from +0.0 with accumulate = 0 (dst is then
 * not read), and the slices are added one at a time in ascending b, each sum rounded: the same bits on every call and on
 * both routes.  TTSK_ERR_ARG: dst or src NULL, nb < 1, accumulate not 0 or 1; n == 0 is TTSK_OK with no launch. */
int ttsk_sum_slices(double *dst, const double *src, int nb, size_t stride, size_t n, int accumulate, int stream);

/* ---- TT input x TT DRMs: the whole streaming sketch in one call ---------------
 * general_sketch(TensorTrain, TensorTrainDRM, TensorTrainDRM, streaming)
 * (sketch_dispatch.py:202-275) = right chain + left chain of TensorTrainDRM.sketch_tt
 * (tensor_train_drm.py:71-88, through handle_transpose drm_base.py:122-145 for the right
 * side, without materialising tensor.T), Omega_mu = L_mu^T R_mu and
 * Psi_mu = L_{mu-1}^T X_mu R_mu (tensor_train_sketch.py:8-35).  The first GEMM of a left
 * chain step, T = L_{mu-1}^T X_mu, is shared with Psi_mu.
 *
 *   n[d]              mode sizes
 *   s[d+1]            TT ranks of the input, s[0] = s[d] = 1; X[mu] is (s[mu], n[mu], s[mu+1])
 *   lt[d]             true ranks of the left DRM, lt[0] = 1; DL[mu] is (lt[mu], n[mu], lt[mu+1]), mu < d-1
 *   rt[d]             true ranks of the right DRM in ITS walking order (mode d-1 first), rt[0] = 1;
 *                     DR[j] is (rt[j], n[d-1-j], rt[j+1]), j < d-1
 *   l_lo/l_hi[d-1]    rank_min / rank_max of the left DRM (slice of the yielded contraction, :88)
 *   r_lo/r_hi[d-1]    same for the right DRM, in its walking order
 *   out               packed [Psi_0 .. Psi_{d-1}, Omega_0 .. Omega_{d-2}], Psi_mu (l_{mu-1}, n_mu, r_mu),
 *                     Omega_mu (l_mu, r_mu) with l, r the sliced ranks in user order -- the buffer that
 *                     ttsk_comm_allreduce_sum reduces.  accumulate != 0 adds (TensorSum / `stt + X`,
 *                     sketch_dispatch.py:85-139, sketch.py:292-301).
 * All pointer arrays are host arrays of device pointers. */
int ttsk_tt_sketch(int d, const int64_t *n, const int64_t *s, const int64_t *lt, const int64_t *l_lo,
                   const int64_t *l_hi, const int64_t *rt, const int64_t *r_lo, const int64_t *r_hi,
                   const double *const *X, const double *const *DL, const double *const *DR,
                   double *out, int accumulate, int stream);
/* The same for nb tensors of ONE signature (n, s) against the same DRMs: X[b*d + mu] is core mu of
 * tensor b, sketch b goes to out + b*out_stride (out_stride >= ttsk_tt_sketch_size, ignored for
 * nb == 1).  Every chain product is then a single launch over all nb tensors -- the kernels'
 * fixed costs (launch gap, staging the small operand, pipeline fill and drain) are paid once per
 * batch.  This is the term loop of a TensorSum input (sketch_dispatch.py:85-139) and the
 * throughput mode bench.py measures. */
int ttsk_tt_sketch_batch(int nb, int d, const int64_t *n, const int64_t *s, const int64_t *lt, const int64_t *l_lo,
                         const int64_t *l_hi, const int64_t *rt, const int64_t *r_lo, const int64_t *r_hi,
                         const double *const *X, const double *const *DL, const double *const *DR,
                         double *out, int64_t out_stride, int accumulate, int stream);
/* The sketch of the SUM of nb tensors of one signature (a TensorSum of TTs, sketch_dispatch.py:85-139) as ONE
 * packed sketch at `out`: the chains run per tensor as in ttsk_tt_sketch_batch, Psi_mu and Omega_mu contract over
 * (tensor, TT rank) in one product each -- a sum of TTs is a TT with block-diagonal cores -- so no per-tensor
 * sketch is written or summed.  accumulate != 0 adds to `out`. */
int ttsk_tt_sketch_sum(int nb, int d, const int64_t *n, const int64_t *s, const int64_t *lt, const int64_t *l_lo,
                       const int64_t *l_hi, const int64_t *rt, const int64_t *r_lo, const int64_t *r_hi,
                       const double *const *X, const double *const *DL, const double *const *DR,
                       double *out, int accumulate, int stream);
/* Compute-unit budgets of the batched launches of the three calls above (csrc/sketch_split.h): the right chain steps, the
 * left chain steps and the Psi products are each planned for a share of the device, so that the kernels of the call's two
 * streams run beside each other on disjoint CUs instead of taking the chip in turns.  Per class: -1 = the library's policy
 * (the default: a split only for a caller that keeps batched sketches in flight on more than one stream pair, known by
 * consecutive calls going to different streams; the whole device otherwise), 0 = the whole device, > 0 = that many CUs
 * (more than the device has: the whole device; fewer than nb: one workgroup per tensor).  Process-wide until changed;
 * takes effect with the next call; queues nothing.  A budget changes
 * how many partial sums a result is added up from: sketches under different budgets agree to rounding, not bit for bit;
 * under one setting they are the same bits on every call.  For tests and measurements.  TTSK_ERR_ARG: a value below -1.
 * The policy's one piece of history is process-wide too: the stream of the one-call sketch queued LAST by any thread (none
 * before the first); ttsk_tt_orth_sketch and ttsk_tt_orth_sketch_batch count as such a sketch on every stream they run
 * chains on (their chains go through the same driver, unbudgeted themselves).  A call counts as a pipelined caller's exactly when that stream is another one than its own, so under -1
 * the grids, and with them the bits, of a batch of 8 tensors or more depend on where the call before it went and on nothing
 * else: after a call on stream 2 the next call on stream 0 is split, the one after that on stream 0 is not.  A caller that
 * needs the bits of a call alone on its stream makes one call on that stream first, or sets the budgets.  Whatever the
 * history, the three calls may be queued on any library stream, adjacent ones included, with others in flight: a call's
 * helper (stream + 1) mod TTSK_NUM_STREAMS is forked behind what its own stream holds and joined back, its workspace is its
 * own stream's (tests/test_gpu_streams_in_flight.py). */
int ttsk_tt_sketch_split(int right_cus, int left_cus, int psi_cus);
/* One interior step of a TensorTrainDRM chain for nb tensors of one signature, both products in one launch
 * with the intermediate kept on chip (csrc/chain_fused.h):
 *   Out_b[j, a'] = sum_{c, a, k} W_b[c, a] X_b(j, k, c) E[a, k, a']        (tensor_train_drm.py:81-87)
 * W_b (K1 x A, row stride w_c), X_b addressed by element strides (x_j, x_k, x_c) -- so the transposed core of
 * a right sketch needs no copy --, E (A, n, A2) contiguous, Out_b (J x A2) contiguous.  T != NULL also stores
 * T_b[a, k, j] = sum_c W_b[c, a] X_b(j, k, c) (A x n x J contiguous), the operand Psi_mu shares with the left
 * chain (tensor_train_sketch.py:28-34).  TTSK_ERR_UNSUPPORTED when the shape is outside the kernel's cover
 * (ranks whose 16-tile / 4-strip structure has no instantiation, J > 112, odd A2); ttsk_tt_sketch_batch then
 * uses the two-launch form. */
int ttsk_chain_step(int nb, int n, int K1, int A, int A2, int J, const double *const *W, int64_t w_c,
                    const double *const *X, int64_t x_j, int64_t x_k, int64_t x_c, int64_t x_extent,
                    const double *E, double *const *T, double *const *Out, int stream);
/* The same step (same arguments, same results) on the chunked kernel (csrc/chain_wide.h): the DRM rank A is cut
 * into chunks dealt over workgroups, a wave carries up to two 16-row tiles.  Covers what ttsk_chain_step does not:
 * TT ranks K1 beyond 128 and J up to 176 (rank-150 inputs, scripts/plot_timings.py:28-36), input and output DRM
 * ranks of different tile structure, odd DRM ranks, A2 up to 160, K1 much smaller than A.  TTSK_ERR_UNSUPPORTED
 * outside that; ttsk_tt_sketch_batch tries ttsk_chain_step's kernel, then this one, then the two-launch form. */
int ttsk_chain_step_wide(int nb, int n, int K1, int A, int A2, int J, const double *const *W, int64_t w_c,
                         const double *const *X, int64_t x_j, int64_t x_k, int64_t x_c, int64_t x_extent,
                         const double *E, double *const *T, double *const *Out, int stream);
/* The same step for MANY low-rank tensor trains at once (csrc/chain_sum.h: the summands of a TensorSum,
 * sketch_dispatch.py:85-147, whose chains share the DRM; K1, J <= 20, A, A2 <= 128, A2 even): the rows of several
 * terms are stacked into full 16-row tiles, the work of the second product is dealt over the waves by (row tile,
 * column tile) rectangles.  T (optional) receives the intermediate as T[b * t_b + (a * n + k) * t_ld + j] (t_extent
 * elements addressable): t_b = J, t_ld = nb * J is the operand layout of the Psi of a sum (one product over (term,
 * rank)).  TTSK_ERR_UNSUPPORTED outside the cover; ttsk_tt_sketch_sum / _batch then use the other forms. */
int ttsk_chain_step_sum(int nb, int n, int K1, int A, int A2, int J, const double *const *W, int64_t w_c,
                        const double *const *X, int64_t x_j, int64_t x_k, int64_t x_c, int64_t x_extent,
                        const double *E, double *T, int64_t t_b, int64_t t_ld, int64_t t_extent,
                        double *const *Out, int stream);
/* The Psi products of the one-call TT sketch on their own kernels (csrc/stream_small.h; tensor_train_sketch.py:28-34:
 * Psi_mu = T_mu R_mu), reached directly:
 *   ttsk_psi_stream:      C_b[j, a] (+)= sum_c S_b[j, c] W_b[c, a]          for nb <= 32 problems of one shape
 *   ttsk_psi_stream_sum:  C[j, a]   (+)= sum_b sum_c S_b[j, c] W_b[c, a]    nb >= 2 terms, term b at S + b * s_b, W + b * w_b
 * S_b (J x K1, row stride s_j), W_b (K1 x A, row stride w_c), C (J x A, row stride c_j), columns contiguous, all 8-byte
 * aligned; accumulate != 0 adds to C.  The kernels stream J >= 1024 rows; A from 9 (17 for the sum) as far as the column
 * chunks and the LDS reach.  TTSK_ERR_UNSUPPORTED outside the cover (csrc/psi_plan.h), nothing is written then.
 * WHAT THE CALLER GUARANTEES: a row of S is read on to whole runs of k-blocks -- the elements S_b[j][K1 .. 4 KB1) behind
 * it, which are the row's padding, the rows after it and, for the sum, the gap between two terms and the head of the
 * next term -- and multiplied by exact zeros.  Every such element that lies inside the operand (before S_b[J-1][K1]; for
 * the sum before S_{nb-1}[J-1][K1]) must be FINITE; what lies behind that is never read. */
int ttsk_psi_stream(int nb, int J, int K1, int A, const double *const *S, int64_t s_j, const double *const *W,
                    int64_t w_c, double *const *C, int64_t c_j, int accumulate, int stream);
int ttsk_psi_stream_sum(int nb, int J, int K1, int A, const double *S, int64_t s_j, int64_t s_b, const double *W,
                        int64_t w_c, int64_t w_b, double *C, int64_t c_j, int accumulate, int stream);
/* A DRM core E (A, n, A2) is the same for every sketch it takes part in; ttsk_chain_step's kernel reads each slice
 * E[:, k, :] into LDS in one fixed permutation.  ttsk_drm_pack stores that permutation once (csrc/chain_pack.hip): an
 * image of n * eunits * 16 bytes -- at rank 100 as large as the core, so a packed core takes about twice the device
 * memory -- allocated by the library and registered under (core, A, n, A2).  Every later fused chain step whose E is
 * `core` with these extents loads its slices from the image, 1 KB per instruction; results are bit-identical.  Returns
 * after `stream` has drained.  TTSK_ERR_UNSUPPORTED for ranks the fused kernel does not cover (nothing is registered).
 * THE CORE MUST NOT BE WRITTEN WHILE IT IS REGISTERED, and must be unregistered before its memory is freed or reused:
 * ttsk_drm_unpack drops and frees the image (no-op for an unregistered core; waits for the device).  ttsk_shutdown
 * empties the registry. */
int ttsk_drm_pack(const double *core, int A, int n, int A2, int stream);
int ttsk_drm_unpack(const double *core);
/* Dense tensor x DRM MATRICES (dense_gaussian_drm.py:77-80, dense_sketch.py:7-52): the first four left products
 * Z_mu = A_mu X^{<mu+1>}, mu = 0..3, from ONE read of X viewed as (n0, n1, n2, C = n3 * n4) (csrc/dense_left_pass.hip).
 * A0 (l, n0) and A3 (l, n0 n1 n2 n3) as the DRM holds them, A1t (l, n1, n0) / A2t (l, n2, n1, n0) the transposed copies of
 * A_1 / A_2; Z0 (l, n1 n2 C), Z1 (l, n2 C), Z2 (l, C); E3 (l, C) still holds i3: Z_3[a, i4] = sum_{i3} E3[a, (i3, i4)].
 * TTSK_ERR_UNSUPPORTED outside the cover (n0 % 4, C % 512, n4 in {64, 128, 256, 512}, l <= 20). */
int ttsk_dense_left_pass(const double *X, int64_t n0, int64_t n1, int64_t n2, int64_t C, int64_t n4, int l,
                         const double *A0, const double *A1t, const double *A2t, const double *A3, double *Z0, double *Z1,
                         double *Z2, double *E3, int stream);
/* number of doubles ttsk_tt_sketch writes to `out` */
int64_t ttsk_tt_sketch_size(int d, const int64_t *n, const int64_t *l_lo, const int64_t *l_hi,
                            const int64_t *r_lo, const int64_t *r_hi);
/* per-kernel device timing of the launches made by ttsk_tt_sketch (bench.py roofline leg):
 * while enabled every GEMM launch is bracketed by hipEvents on its stream.  on = 1 resets every class's counters
 * and kernel name. */
int ttsk_prof_enable(int on);
/* measured ceiling of v_mfma_f64_16x16x4_f64 on this device (register-resident operands, 4 independent
 * accumulators per wave, two waves per SIMD, every CU busy): TFLOP/s.  MI355X_MICROARCH.md lists no fp64 MFMA
 * row, so bench.py states this number next to the 78.6 TF/s data-sheet value (it measures 77.7 at 2.4 GHz:
 * one instruction per 64 cycles and SIMD; sustained kernels run at a lower clock). */
int ttsk_mfma_f64_peak_probe(double *tflops);
/* measured ceiling of the hash-Gaussian sampler's arithmetic on this device (fast_lazy_gaussian.pyx:23-49,91-105: the 64-bit
 * mix, the forced-exponent bits, Cephes ndtri), operands resident, no memory traffic: gsamples[0] with the central / tail
 * split of the sampling kernels (tail samples queued and evaluated a full wave at a time), gsamples[1] every lane through
 * ndtri as it comes.  10^9 samples / s.  bench.py prices the sampling passes of the sparse sketch against [0]. */
int ttsk_ndtri_rate_probe(double *gsamples);
/* class 0/1: right-chain GEMM1 (T = R^T X^T) / GEMM2 (split-K); 2/3: left-chain GEMM1 / GEMM2;
 * 4: Psi GEMM; 5: small products (Omega, first mode); 6: samplers; 7: sparse Psi / Omega; 8: small
 * factorisations; 11 (the last class): untagged ttsk_gemm calls.  Only the main
 * contraction kernel of each call is bracketed (not the split-K reduce / zero fill) -- except for the fused
 * chain step, which replaces BOTH products of a step: it is filed under class 1 (right) / 3 (left) with the
 * flops of both and its slab reduce inside the bracket. */
int ttsk_prof_read(int cls, int64_t *launches, double *total_ms, double *flops);
/* rocprofv3 name of the largest contraction-kernel launch of class `cls` since ttsk_prof_enable(1) (empty: none) */
int ttsk_prof_kernel_name(int cls, char *buf, size_t len);

/* ---- hash sampler (the reference's native module) -------------------------
 * Host-pointer twins of the Cython API (fast_lazy_gaussian.pyx:14,53,156,183);
 * idx is (m, N) row-major int64/uint64, shape has m entries. */
int ttsk_hash_u64(uint64_t *host_vals, size_t n);                       /* pyx:13-37, in place */
int ttsk_inds_to_rand_double(const uint64_t *host_idx, const uint64_t *shape, int m, size_t N,
                             int rank_min, int rank_max, uint64_t seed, double *host_out);
int ttsk_inds_to_normal(const int64_t *host_idx, const uint64_t *shape, int m, size_t N,
                        int rank_min, int rank_max, uint64_t seed, double *host_out /* (N,rank) */);
int ttsk_inds_to_sparse_sign(const int64_t *host_idx, const uint64_t *shape, int m, size_t N,
                             int true_rank, int rank_min, int rank_max, int nnz_per_row,
                             uint64_t seed, int16_t *host_out /* (N, rank_max-rank_min) */);
/* Device-resident forms used by SparseGaussianDRM / SparseSignDRM.sketch_sparse
 * (sparse_gaussian_drm.py:29-44, sparse_sign_drm.py:34-51).  idx rows are addressed
 * as dev_idx + row_order[i]*row_stride so that tensor.T (tensor.py:201-204, reversed
 * index rows) needs no copy.  Output (N, rank) row-major fp64. */
int ttsk_sparse_normal_dev(const int64_t *dev_idx, int64_t row_stride, const int *row_order,
                           const uint64_t *shape, int m, size_t N, int rank_min, int rank_max,
                           uint64_t seed, double *dev_out, int stream);
/* the same samples for EVERY possible prefix: row f of dev_out (prod(shape), rank) belongs to the index row whose
 * Fortran-order flat index is f (only without the 32-bit wrap of the reference's running product) */
int ttsk_sparse_normal_table(const uint64_t *shape, int m, int rank_min, int rank_max, uint64_t seed, double *dev_out,
                             int stream);
int ttsk_sparse_sign_dev(const int64_t *dev_idx, int64_t row_stride, const int *row_order,
                         const uint64_t *shape, int m, size_t N, int true_rank, int rank_min,
                         int rank_max, int nnz_per_row, uint64_t seed, double *dev_out, int stream);
/* sign rows for EVERY possible prefix, as ttsk_sparse_normal_table (sparse_sign_drm.py:34-51 on all index rows at once) */
int ttsk_sparse_sign_table(const uint64_t *shape, int m, int true_rank, int rank_min, int rank_max, int nnz_per_row, uint64_t seed,
                           double *dev_out, int stream);
/* counter-based N(0,1) fill for TensorTrainDRM / DenseGaussianDRM sampling
 * (tensor.py:358-371 via utils.py:178-227; dense_gaussian_drm.py:50-55): the
 * reference's streams are not reproducible across hosts, parity is by
 * injection; this generator is the same hash -> ndtri construction keyed by (seed, i). */
int ttsk_fill_normal(double *dev_out, size_t n, uint64_t seed, double scale, int stream);
/* `count` such fills in one launch -- array i gets exactly the samples ttsk_fill_normal(seeds[i], scales[i]) would
 * give it (the d - 1 cores of a TensorTrainDRM, tensor.py:358-371: one launch instead of d - 1).  Host arrays. */
int ttsk_fill_normal_many(int count, double *const *dev_outs, const size_t *ns, const uint64_t *seeds,
                          const double *scales, int stream);
/* ---- products with a Gaussian matrix that is never stored (csrc/gauss_lazy.hip, plan in csrc/gauss_lazy_plan.h) ----
 * G is the (row_hi x cols) array ttsk_fill_normal(seed, scale 1) writes, rows [row_lo, row_hi) of it: its entries are
 * sampled where an fp64 MFMA GEMM consumes them, bit for bit the stored ones.  w = row_hi - row_lo.
 *   left:  Z (w x Q, leading dimension ldz) = G[row_lo:row_hi, 0:cols] Xu,  Xu (cols x Q) row-major, leading dimension ldx
 *   right: Out (rows x w, ldo) = S G[row_lo:row_hi, 0:cols]^T,             S (rows x cols) row-major, leading dimension lds
 * Fixed order of summation, no atomics: the same bits on every call.  w = 0 or no columns / rows: nothing is done.
 * TTSK_ERR_UNSUPPORTED (the caller fills the matrix and multiplies): w > 64, an extent of 2^31 or more, row_hi * cols
 * beyond 2^63. */
int ttsk_gauss_lazy_left(uint64_t seed, int64_t row_lo, int64_t row_hi, int64_t cols, const double *dev_xu, int64_t Q, int64_t ldx,
                         double *dev_z, int64_t ldz, int stream);
int ttsk_gauss_lazy_right(uint64_t seed, int64_t row_lo, int64_t row_hi, int64_t cols, const double *dev_s, int64_t rows, int64_t lds,
                          double *dev_out, int64_t ldo, int stream);

/* ---- sparse-input kernels --------------------------------------------------
 * TensorTrainDRM.sketch_sparse (tensor_train_drm.py:60-69): per nonzero e,
 *   v_e <- v_e * D[:, idx[e], :], out (N, rho') row-major; vin NULL for the first mode */
int ttsk_sparse_ttdrm_step(const double *dev_vin, int64_t rho, const double *dev_core,
                           int64_t n, int64_t rhop, const int64_t *dev_idx_row, size_t N,
                           double *dev_vout, int stream);
/* ---- Khatri-Rao DRM (csrc/khatri_rao.hip): every step is an elementwise product of rows of width w ----
 * the rows of all prefixes of one level from the level before:
 *   out[i * P + p, c] = prev[p, c] * g[i, c],  prev (P, w) or NULL (P = 1, ones), g (n, w), out (n * P, w) row-major
 * (the row order of the sparse pass's tables: the first mode the fastest digit; the caller allocates one spare row) */
int ttsk_kr_rows(const double *dev_prev, int64_t P, const double *dev_g, int64_t n, int64_t w, double *dev_out, int stream);
/* one step of the panels: out[e, c] = (v ? v[e, c] : 1) * g[idx ? idx[e] : e, c], v and out (N, w), g (n, w) row-major;
 * out may be v; without idx N <= n; an index outside [0, n) is clamped */
int ttsk_kr_step(const double *dev_v, const double *dev_g, int64_t n, int64_t w, const int64_t *dev_idx, size_t N,
                 double *dev_out, int stream);
/* DenseGaussianDRM.sketch_sparse (dense_gaussian_drm.py:59-66): C-order ravel of the
 * first m index rows, then column gather of mat (rank, cols): out (N, rank) row-major */
int ttsk_sparse_densedrm_gather(const double *dev_mat, int64_t rank, int64_t cols,
                                const int64_t *dev_idx, int64_t row_stride, const int *row_order,
                                const int64_t *shape, int m, size_t N, double *dev_out, int stream);
/* sketch_psi_sparse (sparse_sketch.py:8-36,49-69):
 *   Psi[a, idx[e], c] += val[e] * Lv[e,a] * Rv[e,c]   (Lv/Rv NULL -> rank 1, value 1)
 * Lv (N,l) and Rv (N,r) row-major as produced above; Psi (l,n,r) contiguous, zeroed by caller.
 * The kernel reduces runs of equal mode index in registers and issues one atomic per run and
 * output pair; with `dev_perm` = ttsk_sparse_sort_mode's permutation (nonzeros visited in order of
 * their mode index) that is a segmented reduction.  dev_idx_row == NULL with n == 1 sums over all
 * nonzeros: sketch_omega_sparse (sparse_sketch.py:39-46), Omega = (L * entries) R^T. */
int ttsk_sparse_psi(const double *dev_val, const int64_t *dev_idx_row, const int64_t *dev_perm, size_t N,
                    const double *dev_Lv, int64_t l, const double *dev_Rv, int64_t r,
                    int64_t n, double *dev_psi, int stream);

/* ---- evaluation at index lists (csrc/tt_gather.hip) --------------------------
 * TensorTrain.gather (tensor.py:414-440): per index tuple e the chain
 *   t_e = G_0[0, i_0(e), :] G_1[:, i_1(e), :] ... G_{d-1}[:, i_{d-1}(e), 0]
 * with all d modes in one launch and the running vector kept on chip (no (N x rank) panel in HBM).
 *   dev_cores[k]  (ranks[k], shape[k], ranks[k + 1]) contiguous, ranks[0] = ranks[d] = 1
 *   dev_idx       int64 index matrix: mode k of tuple e at dev_idx[row_order[k] * row_stride + e] (row_order NULL:
 *                 identity), the addressing of ttsk_sparse_densedrm_gather -- a SparseTensor and its .T are read in place
 *   dev_val       (N,) entries, or NULL
 *   dev_out       (N,) receives t in input order, or NULL
 *   dev_stats     3 doubles, or NULL: sum_e x_e t_e (SparseTensor.dot, tensor.py:250-255), sum_e t_e^2 and
 *                 sum_e (t_e - x_e)^2 (the sampled error of scripts/frostt.py:112-116 over all of the list); needs dev_val.
 *                 Summed in a fixed order (per-workgroup partial sums, then one workgroup): the same bits on every
 *                 call, with or without dev_out.
 * TTSK_ERR_ARG: NULL cores / indices, d < 1, ranks[0] or ranks[d] != 1, dev_out and dev_stats both NULL, dev_stats
 * without dev_val.  TTSK_ERR_UNSUPPORTED before anything is launched: d > 32, a rank beyond 256, a mode of 2^31 or more. */
int ttsk_tt_gather(const double *const *dev_cores, const int64_t *ranks /* d + 1 */, const int64_t *shape, int d,
                   const int64_t *dev_idx, int64_t row_stride, const int *row_order, size_t N,
                   const double *dev_val, double *dev_out, double *dev_stats /* 3 doubles */, int stream);
/* CPTensor.gather (tensor.py:726-732): t_e = sum_rho prod_k A_k[i_k(e), rho], dev_factors[k] (shape[k], rank) contiguous;
 * indices, outputs, statistics and errors as above (any rank >= 1 is covered). */
int ttsk_cp_gather(const double *const *dev_factors, int64_t rank, const int64_t *shape, int d,
                   const int64_t *dev_idx, int64_t row_stride, const int *row_order, size_t N,
                   const double *dev_val, double *dev_out, double *dev_stats, int stream);
/* TuckerTensor entries (tensor.py:771-780 at single indices; csrc/tucker_gather.hip, plan in csrc/tucker_gather_plan.h):
 *   t_e = sum_{a_1..a_d} C[a_1..a_d] prod_k U_k[a_k, i_k(e)]
 *   dev_core       (ranks[0], .., ranks[d-1]) contiguous, C order
 *   dev_factors[k] (ranks[k], shape[k]) contiguous
 * indices, dev_val, dev_out, dev_stats, their summation order and the argument errors exactly as ttsk_tt_gather (and a
 * rank below 1 is TTSK_ERR_ARG).  2 |C| flops per tuple on the fp64 matrix instructions, no atomics, the same bits on
 * every call.  TTSK_ERR_UNSUPPORTED before anything is launched or allocated: d > 8, a core of more than 2^20 entries, a
 * mode of 2^31 or more. */
int ttsk_tucker_gather(const double *dev_core, const double *const *dev_factors, const int64_t *ranks /* d */,
                       const int64_t *shape, int d, const int64_t *dev_idx, int64_t row_stride, const int *row_order,
                       size_t N, const double *dev_val, double *dev_out, double *dev_stats /* 3 doubles */, int stream);

/* ---- a sparse tensor against another explicit tensor: join on sorted keys (csrc/sparse_join.hip, plan in
 * csrc/sparse_join_plan.h) ----
 * SparseTensor.gather (tensor.py:275-286, a dict of every nonzero) and SparseTensor.dot (tensor.py:250-255) against a
 * sparse or a dense tensor.  The key of an index tuple is its C-order flat index in `shape` (np.ravel_multi_index); index
 * matrices are addressed as in ttsk_tt_gather (row_stride, row_order), so a SparseTensor and its .T are read in place.
 * TTSK_ERR_UNSUPPORTED before anything is launched or allocated: d > 32, a shape of more than 2^63 - 1 entries, a table
 * of 2^31 nonzeros or more.  max_split: splitters kept per table, 0 for the library's choice (the same value in the calls
 * that build and that read an index).
 *
 * Index of a table: the nonzeros sorted stably by key.
 *   dev_keys_sorted (N) int64, dev_vals_sorted (N): dev_vals_sorted[i] = dev_val[perm[i]]
 *   dev_splitters   every stride-th sorted key; stride and count from ttsk_sparse_join_layout */
int ttsk_sparse_key_index(const int64_t *shape, int d, const int64_t *dev_idx, int64_t row_stride, const int *row_order, size_t N,
                          const double *dev_val, int max_split, int64_t *dev_keys_sorted, double *dev_vals_sorted,
                          int64_t *dev_splitters, int stream);
/* Lookup of Nq index tuples in an index: dev_out[q] (or NULL) = the entry of the LAST nonzero of the table with the key of
 * query q, 0.0 if there is none (a repeated index of the table counts once, the last one wins: the dict of the reference;
 * every query counts); dev_dot (1 double, or NULL; needs dev_qval) = sum_q dev_qval[q] * that, summed in a fixed order
 * without atomics: the same bits on every call, with or without dev_out.  N_table = 0 and Nq = 0 are legal. */
int ttsk_sparse_join(const int64_t *dev_keys_sorted, const double *dev_vals_sorted, const int64_t *dev_splitters, size_t N_table,
                     int max_split, const int64_t *shape, int d, const int64_t *dev_qidx, int64_t q_row_stride,
                     const int *q_row_order, size_t Nq, const double *dev_qval, double *dev_out, double *dev_dot, int stream);
/* The same against a contiguous C-order dense tensor dev_x of `shape`: the key is the element offset */
int ttsk_dense_join(const double *dev_x, const int64_t *shape, int d, const int64_t *dev_qidx, int64_t q_row_stride,
                    const int *q_row_order, size_t Nq, const double *dev_qval, double *dev_out, double *dev_dot, int stream);
/* The plan's numbers for a table of N_table nonzeros and Nq queries on this device (host only, after ttsk_init):
 * out[0..7] = SJ_MAX_SPLIT, stride, splitter count, steps of the LDS search, steps of the segment search, workgroups,
 * queries per workgroup, longest chain of additions of the dot */
int ttsk_sparse_join_layout(size_t N_table, size_t Nq, int max_split, int64_t *out);

/* ---- Gram matrix of tensor trains (csrc/tt_gram.hip, plan in csrc/tt_gram_plan.h) ----
 * TensorTrain.dot (tensor.py:542-557) for every pair of two lists of trains at once: dev_out[p * M + q] = <A_p, B_q>.  With
 * it Tensor.error(fast=True) (tensor.py:68-72) of two trains is one 2 x 2 call, a Hessenberg column of tt_gmres.py:385-386
 * one 1 x (j + 1) call.  One launch per mode over all pairs (the chunk partials of the mode before are summed, in order, as
 * they are loaded) and one closing launch: at most d + 1 launches whatever K M is.
 *   dev_cores_a[p * d + k]  core k of A_p, (ranks_a[p * (d + 1) + k], shape[k], ranks_a[p * (d + 1) + k + 1]) contiguous;
 *   dev_cores_b, ranks_b    the same for the M trains B_q; all trains of the one shape, each with its own ranks
 *   dev_out                 (K, M) row-major
 * No atomics; the split of a mode depends on the shapes, K M and the CU count alone: the same bits on every call.
 * TTSK_ERR_ARG: a NULL pointer, d < 1, K or M < 1, a boundary rank != 1, a rank or a mode size < 1.  TTSK_ERR_UNSUPPORTED
 * before anything is launched: d > 32, a rank beyond 128, a mode of 2^31 or more, K + M > 128 (the caller then composes
 * the products from ttsk_gemm, or cuts the lists). */
int ttsk_tt_gram(const double *const *dev_cores_a, const int64_t *ranks_a, int K, const double *const *dev_cores_b,
                 const int64_t *ranks_b, int M, const int64_t *shape, int d, double *dev_out, int stream);

/* ---- the bond solve of Gram-SVD rounding (csrc/gram_round.hip, plan in csrc/gram_round_plan.h) ----
 * Every bond of a tensor train truncated at once from the Gram matrices of its left and right parts (Al Daas, Ballard,
 * Manning 2022).  For bond b of rank r = ranks[b], with GL = V_L L_L V_L^T and GR = V_R L_R V_R^T (the
 * eigenpairs above r eps_machine of the largest) and M = L_L^{1/2} V_L^T V_R L_R^{1/2} = U S W^T:
 *   dev_sigma[b]   (r) the singular values S of the b-th unfolding, descending, zero beyond those found
 *   dev_rank_out   [b] = rho = max(1, min(#{S > S_1 eps}, caps[b]))
 *   dev_pt[b]      (r, r) row-major, row c < rho the column c of P = V_L L_L^{-1/2} U_rho, rows >= rho zero
 *   dev_q[b]       (r, r) row-major, row c < rho of Q = U_rho^T L_L^{1/2} V_L^T, rows >= rho zero
 * so that the rounded cores are Q_k C_k P_{k+1}.  dev_gl[b], dev_gr[b]: (r, r) row-major.  The pointer tables and ranks
 * are host arrays.  Two launches whatever count is (one workgroup per Gram, then one per bond), one-sided Jacobi; no
 * atomics: the same bits on every call.  Singular values below about sqrt(eps_machine) of the largest are not resolved.
 * TTSK_ERR_ARG: a NULL pointer, count < 1, a rank or cap < 1, eps negative or not finite.  TTSK_ERR_UNSUPPORTED before
 * anything is launched: count > 64, a rank beyond 1024. */
int ttsk_gram_round_bonds(const double *const *dev_gl, const double *const *dev_gr, const int64_t *ranks, const int64_t *caps,
                          int count, double eps, double *const *dev_pt, double *const *dev_q, double *const *dev_sigma,
                          int *dev_rank_out, int stream);

/* ---- operator-times-train products, never formed (csrc/op_apply.hip, plan in csrc/op_apply_plan.h) ----
 * One step of sketching the product of a matrix product operator and a tensor train (tt_gmres.py:91-101) without its
 * cores: for every term p of a sum, with operator core M (R, n_in, n_out, R'), train core C (r, n_in, r') and the chain
 * so far L (R, r, l),
 *   W[l, i, w_off + beta' r' + a'] = sum_{beta, j} M[beta, j, i, beta'] sum_a L[beta, a, l] C[a, j, a'];
 * the inner sum stays on the chip.  The chain step, Psi and Omega of the sum are one ttsk_gemm each on W.
 *   L[p]      contiguous (R, r, l)
 *   M[p]      strided, or NULL: a plain train in the sum, W[l, i, w_off + a'] = sum_a L[a, l] C[a, i, a'] (R = R' = 1,
 *             n_in = n_out)
 *   C[p]      strided
 *   dims      K rows of 7: R, R', r, r', n_in, n_out, w_off
 *   strides   K rows of 7, in elements: M over (beta, j, i, beta'), then C over (a, j, a')
 *   W         contiguous (l, n_out, w_cols); term p writes the columns w_off .. w_off + R' r' and nothing else
 * n_out and l are those of every term.  One workgroup forms each element in a fixed order, no atomics: the same bits on
 * every call.  TTSK_ERR_ARG: a NULL pointer, K < 1, an extent below 1, a term without operator that has R or R' != 1 or
 * n_in != n_out, w_off + R' r' > w_cols, differing n_out.  TTSK_ERR_UNSUPPORTED before anything is launched: an extent,
 * R n_in or n_out R' of 2^31 or more, K > 24 (the terms travel as the kernel's argument; the caller cuts longer lists into
 * several calls, which the column offsets allow).  Inside those bounds every shape runs. */
int ttsk_op_apply(int K, const double *const *L, const double *const *M, const double *const *C, const int64_t *dims,
                  const int64_t *strides, int64_t l, double *W, int64_t w_cols, int stream);

/* ---- entrywise (Hadamard) products of two tensor trains, never formed (csrc/hadamard_apply.hip, plan in
 * csrc/hadamard_plan.h) ----
 * One step of sketching x o y, whose core is P[(beta a), i, (beta' a')] = X[beta, i, beta'] Y[a, i, a'], without that core:
 * with the chain so far L (R, r, l),
 *   W[l, i, w_off + beta' r' + a'] = sum_beta X[beta, i, beta'] sum_a L[beta, a, l] Y[a, i, a'];
 * the inner sum stays on the chip.  The chain step, Psi and Omega are one ttsk_gemm each on W.  One term per call.
 *   L         contiguous (R, r, l)
 *   X, Y      strided: (R, n, R') and (r, n, r')
 *   dims      R, R', r, r', n, l
 *   strides   in elements: X over (beta, i, beta'), then Y over (a, i, a')
 *   W         contiguous (l, n, w_cols); the call writes the columns w_off .. w_off + R' r' and nothing else
 * One workgroup forms each element in a fixed order, no atomics: the same bits on every call.  TTSK_ERR_ARG: a NULL
 * pointer, an extent below 1, w_off < 0, w_off + R' r' > w_cols.  TTSK_ERR_UNSUPPORTED before anything is launched: an
 * extent or the number of workgroups (n x ceil(l / 16) x ceil(r' / 16) x ceil(R' / 64)) of 2^31 or more.  Inside those
 * bounds every shape runs. */
int ttsk_hadamard_apply(const double *L, const double *X, const double *Y, const int64_t *dims, const int64_t *strides,
                        double *W, int64_t w_cols, int64_t w_off, int stream);

/* ---- inner product of two such products: the closing half of a mode (csrc/hadamard_close.hip, plan in
 * csrc/hadamard_close_plan.h) ----
 * <x o y, u o v> carries a chain G (R, r, S, s) over the ranks of x, y, u and v.  Per mode, ttsk_hadamard_apply with
 * l = S s takes G through the cores of x and y: Wl ((gamma c), i, p) with p = (beta' a').  This entry takes Wl through the cores
 * U (S, n, S') of u and V (s, n, s') of v and sums over the mode:
 *   out[p, gamma' s' + c'] (+)= sum_{i < n} sum_gamma U[gamma, i, gamma'] sum_c Wl[(gamma s + c), i, p] V[c, i, c'];
 * the inner sum stays on the chip and no array indexed by i is written.
 *   Wl            contiguous (S s, n, P)
 *   U, V          strided: (S, n, S') and (s, n, s')
 *   dims          S, S', s, s', n, P
 *   strides       in elements: U over (gamma, i, gamma'), then V over (c, i, c')
 *   out           contiguous (P, S' s'); accumulate = 1 adds to what it holds
 *   work          a slab of the caller's, work_doubles doubles, at least what ttsk_hadamard_close_layout names; every double
 *                 of that size is overwritten
 * The mode is cut into ichunks ranges of i so that few (p, c', gamma') tiles still fill the device; a workgroup writes its
 * partial tile to work (ichunks, P, S' s') and ttsk_sum_slices adds the slices in ascending order into out.  The cut depends
 * on dims alone.  No atomics: the same bits on every call.  TTSK_ERR_ARG: a NULL pointer, an extent below 1, accumulate
 * not 0 or 1, a slab smaller than the plan's.  TTSK_ERR_UNSUPPORTED: an extent or the number of workgroups (ichunks x
 * ceil(P / 16) x ceil(s' / 16) x ceil(S' / 64)) of 2^31 or more.  A refused call launches nothing and writes nothing.  Inside those bounds every shape runs. */
int ttsk_hadamard_close(const double *Wl, const double *U, const double *V, const int64_t *dims, const int64_t *strides, double *out,
                        int accumulate, double *work, int64_t work_doubles, int stream);
/* The plan's numbers for those dims (host only): out[0] = ichunks, out[1] = doubles of the slab */
int ttsk_hadamard_close_layout(const int64_t *dims, int64_t *out);

/* ---- inner product of two operator-times-train products: the closing half of a mode (csrc/op_close.hip, plan in
 * csrc/op_close_plan.h) ----
 * <M x, N y> carries a chain G (R, r, s, S) over the ranks of M, x, y and N, flattened with the train rank of y major,
 * l = c S + gamma.  Per mode, ttsk_op_apply with that l takes G through the cores of M and x: Wl ((c gamma), i, p) with
 * p = (beta' a').  This entry takes Wl through the cores N (S, n_in, n_out, S') of the operator and Y (s, n_in, s') of the
 * train and sums over both mode indices:
 *   out[p, c' S' + gamma'] (+)= sum_{j < n_in} sum_c Y[c, j, c'] sum_gamma sum_{i < n_out} Wl[(c S + gamma), i, p] N[gamma, j, i, gamma'];
 * the inner sums stay on the chip and no array indexed by j is written.
 *   Wl            contiguous (s S, n_out, P)
 *   N, Y          strided: (S, n_in, n_out, S') and (s, n_in, s').  (gamma, i) of N must be one run,
 *                 stride[gamma] == n_out stride[i] (where S or n_out is 1 the other's stride is the run's): a contiguous
 *                 (S, n_out, n_in, S') array viewed as (S, n_in, n_out, S'), padded or not, is; an operator core as stored is not
 *   dims          S, S', s, s', n_in, n_out, P
 *   strides       in elements: N over (gamma, j, i, gamma'), then Y over (c, j, c')
 *   out           contiguous (P, s' S'), columns in (c', gamma') order; accumulate = 1 adds to what it holds
 *   work          a slab of the caller's, work_doubles doubles, at least what ttsk_op_close_layout names; every double
 *                 of that size is overwritten
 * The in-index is cut into jchunks ranges of j so that few (p, gamma', c') tiles still fill the device; a workgroup writes
 * its partial tile to work (jchunks, P, s' S') and ttsk_sum_slices adds the slices in ascending order into out.  The cut
 * depends on dims alone.  No atomics: the same bits on every call.  TTSK_ERR_ARG: a NULL pointer, an extent below 1,
 * accumulate not 0 or 1, a slab smaller than the plan's.  TTSK_ERR_UNSUPPORTED: an N whose (gamma, i) is not one run; an
 * extent, S n_out or the number of workgroups (jchunks x ceil(P / 16) x ceil(S' / 16) x ceil(s' / 64)) of 2^31 or more.  A
 * refused call launches nothing and writes nothing.  Inside those bounds every shape runs. */
int ttsk_op_close(const double *Wl, const double *N, const double *Y, const int64_t *dims, const int64_t *strides, double *out,
                  int accumulate, double *work, int64_t work_doubles, int stream);
/* The plan's numbers for those dims (host only): out[0] = jchunks, out[1] = doubles of the slab */
int ttsk_op_close_layout(const int64_t *dims, int64_t *out);

/* ---- the same for many pairs in one launch (csrc/op_close.hip, plan in csrc/op_close_batch_plan.h) ----
 * The work of ttsk_op_close for npairs independent pairs: one launch in which every pair's workgroups run side by side,
 * and one launch that adds every pair's slices into its out.  Two launches whatever npairs is.
 *   Wl, N, Y, out npairs pointers each, as ttsk_op_close takes them, but for
 *   ldw           npairs numbers: the elements between consecutive (l, i) rows of a pair's Wl, at least its P.  A column
 *                 slice of the W (l, n_out, sum of columns) that one ttsk_op_apply call wrote for many terms is read in
 *                 place with ldw = the width of that W
 *   dims          npairs x 7: S, S', s, s', n_in, n_out, P of each pair
 *   strides       npairs x 7 in elements: N over (gamma, j, i, gamma'), then Y over (c, j, c')
 *   accumulate    one flag for the whole call: 1 adds to what every out holds
 *   work          one slab of the caller's for all pairs, work_doubles doubles, at least what ttsk_op_close_batch_layout
 *                 names; every double of that size is overwritten
 * The out arrays must not overlap each other, work or any input: the entry cannot check this.
 * Each pair is planned as ttsk_op_close plans it (the same cut of j, tiles and slab for the same dims) and its slices are
 * added in the same order, so out holds the bits of a ttsk_op_close call on the same operands, wherever in the list the
 * pair stands.  No atomics: the same bits on every call.  TTSK_ERR_ARG: a NULL array or element, npairs below 1, an
 * extent below 1, ldw below P, accumulate not 0 or 1, a slab smaller than the plan's.  TTSK_ERR_UNSUPPORTED: more than 23
 * pairs (the table of pairs is the kernel's argument); for any pair what ttsk_op_close refuses; 2^31 workgroups or more
 * in all.  The message names the pair.  A refused call launches nothing and writes nothing. */
int ttsk_op_close_batch(int npairs, const double *const *Wl, const double *const *N, const double *const *Y, const int64_t *dims,
                        const int64_t *strides, const int64_t *ldw, double *const *out, int accumulate, double *work,
                        int64_t work_doubles, int stream);
/* The slab of those pairs (host only): out[p] = first double of pair p, p < npairs; out[npairs] = doubles of the slab */
int ttsk_op_close_batch_layout(int npairs, const int64_t *dims, int64_t *out);

/* ---- CP tensors against tensor-train DRMs, no panels (csrc/cp_pass.hip, plan in csrc/cp_pass_plan.h) ----
 * A CP tensor of rank N has factor matrices V_mu (n x N).  The step of TensorTrainDRM.sketch_cp (tensor_train_drm.py:90-107)
 * and the Psi / Omega of cp_sketch.py:6-36 are one GEMM each whose Khatri-Rao operand is formed in registers; the N x n x
 * rank panels of the reference never exist.  All sizes and strides count doubles (elements, not bytes).
 *
 * ttsk_cp_chain_step:  out[j, m] = sum_{a, k} L[j, a] V[k, j] D[a, k, m]
 *   L      (N x rho), row j at L + j ldl, columns contiguous; NULL: rho = 1 and L == 1 (the first mode; ldl is not read)
 *   V      (n x N), element (k, j) at V + k v_k + j v_j: any view of a factor matrix, transposed or a column slice
 *   D      (rho, n, rho') contiguous, the DRM core
 *   out    (N x rho'), row j at out + j ldo; columns from rho' on are not touched
 * ttsk_cp_psi_omega:   psi[i, k, m] = sum_j L[j, i] V[k, j] R[j, m]   and   omega[i, m] = sum_j L[j, i] R_om[j, m]
 *   L      (N x l), row j at L + j ldl; NULL: l = 1 and L == 1 (the first mode)
 *   R      (N x r), row j at R + j ldr; NULL: r = 1 and R == 1 (the last mode)
 *   V      as above; may be NULL when psi is
 *   psi    (l, n, r) contiguous, or NULL (n is not read then)
 *   R_om   (N x r_om), row j at R_om + j ld_om: in a sketch Psi_mu and Omega_{mu-1} share the left contraction L_{mu-1}, but
 *          Omega pairs it with the right contraction of its own bond.  NULL: R itself, omega[i, m] = sum_j L[j, i] R[j, m]
 *          (ld_om and r_om are not read)
 *   omega  (l, r_om) contiguous, or NULL: the columns of Omega ride in the same launch as further columns with V == 1
 * The sum over j is cut into chunks of 512 whose partials (workspace of the library, chunks x the outputs) a closing
 * launch adds in ascending chunk order; with N <= 512 the one launch writes the outputs itself.  No atomics: the same bits
 * on every call.  TTSK_ERR_ARG: a NULL V, D or out, neither psi nor omega, a size below 1, a NULL L or R with its rank
 * != 1, a leading dimension below its width.  TTSK_ERR_UNSUPPORTED before anything is launched: rho, rho', l, r or r_om beyond
 * 128, N or n of 2^31 or more, rho n beyond 2^31 - 65, more than 2^31 - 1 workgroups, partials that 64 bits do not
 * address (the caller then composes the products from ttsk_gemm).  Inside those bounds every shape runs. */
int ttsk_cp_chain_step(const double *L, int64_t ldl, const double *V, int64_t v_k, int64_t v_j, const double *D, double *out,
                       int64_t ldo, int64_t N, int64_t rho, int64_t n, int64_t rho1, int stream);
int ttsk_cp_psi_omega(const double *L, int64_t ldl, const double *R, int64_t ldr, const double *V, int64_t v_k, int64_t v_j,
                      double *psi, const double *R_om, int64_t ld_om, int64_t r_om, double *omega, int64_t N, int64_t l, int64_t n,
                      int64_t r, int stream);

/* ---- inner product of two CP tensors (csrc/cp_gram.hip, plan in csrc/cp_gram_plan.h) ----
 * Tensor.dot / norm / error(fast=True) with a CPTensor on either side (tensor.py:53-88 densifies both operands):
 *   dev_out[0] = sum_{j < N, j' < M} prod_k sum_i A_k[i, j] B_k[i, j']
 * for factor matrices A_k (shape[k] x N) and B_k (shape[k] x M): 2 N M sum_k shape[k] flops, and no array of size N x M --
 * a workgroup keeps the product over the modes of its 64 x 64 tile of (j, j') in registers.
 *   dev_a[k]   A_k, element (i, j) at dev_a[k] + i lda[k] + j: columns contiguous, lda[k] >= N (a column slice of a wider
 *              matrix is taken as it is); dev_a itself is a host array of d device pointers
 *   dev_b, ldb the same for B_k, ldb[k] >= M
 *   sym        != 0: b IS a (dev_b[k] == dev_a[k] and ldb[k] == lda[k] for every k, M == N); only the tiles with
 *              tile(j) <= tile(j') are formed and those strictly above the diagonal count twice
 *   dev_out    1 double
 * Workgroup g of G = min(tiles, 3 x compute units) owns the tiles g, g + G, ... in ascending order and writes one partial;
 * one workgroup adds the partials.  No atomics; the split depends on the shapes, sym and the CU count alone: the same
 * bits on every call.  TTSK_ERR_ARG: a NULL pointer, d < 1, an extent below 1, a leading dimension below its width, sym
 * with differing factors or M != N.  TTSK_ERR_UNSUPPORTED before anything is launched: d > 32, N, M or a mode of 2^31 or
 * more.  Inside those bounds every shape runs. */
int ttsk_cp_gram(const double *const *dev_a, const int64_t *lda, int64_t N, const double *const *dev_b, const int64_t *ldb,
                 int64_t M, const int64_t *shape, int d, int sym, double *dev_out /* 1 double */, int stream);
/* dev_out[0] = sum_i x_i by one workgroup in the library's fixed order (thread t adds x_t, x_{t + 256}, ... in ascending
 * order, then the workgroup total): the same bits on every call; closes <tt, cp> after its chain of ttsk_cp_chain_step.
 * n = 0 gives 0.  TTSK_ERR_UNSUPPORTED: n of 2^32 or more. */
int ttsk_sum(const double *dev_x, size_t n, double *dev_out, int stream);

/* ---- a tensor train against a dense tensor (csrc/tt_dense_stats.hip) ----------
 * Tensor.error / dot / norm for a DenseTensor argument (tensor.py:53-88) and TensorTrain.dense in one pass over the
 * tensor.  The train is cut at a bond: T^{<k>} = L R, dev_L (M x rho) and dev_R (rho x N) row-major and contiguous.
 *   dev_x      (M x N) row-major, or NULL (read as zeros)
 *   dev_out    (M x N) row-major, receives T, or NULL: the reconstruction is then never stored
 *   dev_stats  4 doubles, or NULL: sum x t, sum t^2, sum (t - x)^2, sum x^2.  Per-workgroup partial sums, then one
 *              workgroup, in an order that depends on M and N alone: the same bits on every call, with or without dev_out.
 * Any M, N, rho >= 1.  TTSK_ERR_ARG: a non-positive extent, a NULL factor, a row stride below N.  TTSK_ERR_UNSUPPORTED:
 * dev_out and dev_stats both NULL. */
int ttsk_tt_dense_stats(const double *dev_L, int64_t M, const double *dev_R, int64_t N, int64_t rho,
                        const double *dev_x, double *dev_out, double *dev_stats /* 4 doubles */, int stream);
/* the same on a block of columns of a wider array: rows of dev_x / dev_out are ld_x / ld_out numbers apart (the slab of
 * one range of a mode's values), and with accumulate != 0 the four sums are added to what dev_stats holds */
int ttsk_tt_dense_stats_ld(const double *dev_L, int64_t M, const double *dev_R, int64_t N, int64_t rho,
                           const double *dev_x, int64_t ld_x, double *dev_out, int64_t ld_out, double *dev_stats,
                           int accumulate, int stream);
/* dev_out[0] = sum_i x_i^2 (DenseTensor.norm of a device tensor), the same two-stage, atomic-free form; n = 0 gives 0 */
int ttsk_sumsq(const double *dev_x, size_t n, double *dev_out, int stream);

/* ---- SparseTensor x SparseGaussianDRM without (nnz x rank) panels (csrc/sparse_fused.hip) ----
 * sparse_gaussian_drm.py:29-44 + sparse_sketch.py:8-69 as one pass per mode over a resident, mode-ordered stream. */
/* multipliers of the Fortran-order flat index of fast_lazy_gaussian.pyx:60-71 incl. its 32-bit running product (host) */
int ttsk_sparse_flat_mult(const uint64_t *shape, int m, uint64_t *mult_out);
/* order of one mode's stream: ascending (index of physical row mode_row, flat index of the suffix rows r_rows as in
 * ttsk_sparse_mode_stream); the suffix as the secondary key makes the rows of a right-hand DRM table ascend inside a slice */
int ttsk_sparse_mode_order(const int64_t *dev_idx, int64_t row_stride, size_t N, const int *r_rows, const uint64_t *r_shape, int r_m,
                           int mode_row, int64_t n, int64_t *dev_perm, int stream);
/* stream of one mode: record pos = nonzero perm[pos] (perm: ttsk_sparse_sort_mode; NULL = identity): flat index of the
 * l_m index rows l_rows (prefix, shape l_shape) and of the r_m rows r_rows (suffix as the transposed tensor walks it),
 * the index of physical row mode_row as int32, the entry.  Rows are physical rows of the (d, N) index matrix. */
int ttsk_sparse_mode_stream(const int64_t *dev_idx, int64_t row_stride, const int64_t *dev_perm, size_t N, const int *l_rows,
                            const uint64_t *l_shape, int l_m, const int *r_rows, const uint64_t *r_shape, int r_m, int mode_row,
                            const double *dev_val, uint64_t *dev_fl, uint64_t *dev_fr, int32_t *dev_j, double *dev_v, int stream);
/* the same with 32-bit flat indices (20 instead of 28 bytes per record): TTSK_ERR_UNSUPPORTED when a prefix or suffix extent
 * reaches 2^31 */
int ttsk_sparse_mode_stream_u32(const int64_t *dev_idx, int64_t row_stride, const int64_t *dev_perm, size_t N, const int *l_rows,
                            const uint64_t *l_shape, int l_m, const int *r_rows, const uint64_t *r_shape, int r_m, int mode_row,
                            const double *dev_val, uint32_t *dev_fl, uint32_t *dev_fr, int32_t *dev_j, double *dev_v, int stream);
/* one DRM factor of a pass: kind 0 = ones (width 1), 1 = table[flat][w] (every possible prefix sampled once:
 * ttsk_sparse_normal_table / ttsk_sparse_sign_table; allocated with one spare row: rows are fetched in 16-byte units), 2 = normals sampled in the pass: ndtri(u(hash(flat + hash(rank_min + c)
 * + seed))), 3 = sparse-sign rows sampled in the pass (fast_lazy_gaussian.pyx:121-180; whole row <= 32 entries);
 * flat = src 0: prefix, 1: suffix, 2: prefix + j * mul, 3: suffix + j * mul (the prefix / suffix one mode longer)
 *
 * kind 4 = a row of a tensor-train DRM, formed in the pass: a running vector times `steps` slices of the DRM's cores,
 *     row(e) = t(e) core[0][:, i_0(e), :] ... core[steps - 1][:, i_{steps-1}(e), rank_min : rank_min + w]
 * with core[s] a contiguous (rank[s], n[s], rank[s + 1]) device array.  The digits: the record's flat prefix (src 0, 2) or
 * suffix (src 1, 3) index, the first mode the fastest digit, is split into (row, i_0, i_1, ...) -- `rows` first where there
 * is a table, then n[0], n[1], ...; with src 2 or 3 the last digit is the record's mode index j and is not part of the flat
 * index (mul is not read).  The start: t(e) = table[row(e)][0 : rank[0]], the DRM's partial products up to the level in
 * front of core[0] (`rows` rows of rank[0] doubles and one spare row), or, with table == NULL, the vector (1): rank[0] = 1,
 * core[0] is the DRM's first core.  steps = 0 with a table copies columns [rank_min, rank_min + w) of the start row.  Ranks
 * <= 32, steps <= TTSK_SG_CHAIN_MAX, rows and every n[s] below 2^31; the 32-bit entry point only (the digits of a flat index
 * that wrapped are not those of the record).  seed, full and nnz are not read.
 *
 * kind 5 = a row of a Khatri-Rao DRM, formed in the pass: a kind-4 chain whose steps are diagonal, with the same descriptor,
 *     row(e)[b] = t(e)[rank_min + b] core[0][i_0(e), rank_min + b] ... core[steps - 1][i_{steps-1}(e), rank_min + b],  b < w,
 * the products taken in this order, one rounding each.  core[s] is a contiguous (n[s], rho) device array and every rank[s]
 * is rho <= 32.  The start: t(e) = table[row(e)][0 : rho] (`rows` rows of rho doubles and one spare row), or, with
 * table == NULL, the vector of rho ones.  The digits, steps = 0, the limits and the 32-bit entry point are those of kind 4. */
#define TTSK_SG_CHAIN_MAX 8
typedef struct {
    int steps;
    uint64_t rows;                               /* rows of the start table; 0 without one */
    const double *core[TTSK_SG_CHAIN_MAX];
    int64_t n[TTSK_SG_CHAIN_MAX];
    int rank[TTSK_SG_CHAIN_MAX + 1];
} ttsk_sg_chain;
typedef struct {
    int kind, w, rank_min, src;
    uint64_t mul, seed;
    const double *table;
    int full, nnz;          /* kind 3 only: length of the whole sign row, its +-1 entries (sparse_sign_drm.py:34-51) */
    const ttsk_sg_chain *chain;      /* kinds 4 and 5 only (host memory, read during the call); not read for any other kind */
} ttsk_sg_factor;
/* Psi[a, j, c] (+)= sum_{e: j_e = j} val_e A[e, a] B[e, c]   (dev_psi (wA, n, wB), zero-initialised by the caller)
 * and, with C != NULL, Omega += sum_e val_e C[e, a] B[e, c] (c_left) or sum_e val_e A[e, a] C[e, c]  (dev_omega,
 * zero-initialised).  Stream in ascending j (ttsk_sparse_mode_stream); dev_j == NULL: one slice.  Widths <= 32 (one
 * 16-column matrix tile per factor up to 16, 2 x 2 tiles per product beyond).  No atomics: the result is bit-reproducible. */
int ttsk_sparse_gauss_pass(const uint64_t *dev_fl, const uint64_t *dev_fr, const int32_t *dev_j, const double *dev_val, size_t N,
                           int64_t n, const ttsk_sg_factor *A, const ttsk_sg_factor *B, const ttsk_sg_factor *C, int c_left,
                           double *dev_psi, double *dev_omega, int stream);
int ttsk_sparse_gauss_pass_u32(const uint32_t *dev_fl, const uint32_t *dev_fr, const int32_t *dev_j, const double *dev_val, size_t N,
                           int64_t n, const ttsk_sg_factor *A, const ttsk_sg_factor *B, const ttsk_sg_factor *C, int c_left,
                           double *dev_psi, double *dev_omega, int stream);
/* stable sort permutation of the nonzeros by one index row (values < n): perm[i] = id of the i-th
 * nonzero in mode-index order.  Independent of the DRM: computed once per tensor and mode. */
int ttsk_sparse_sort_mode(const int64_t *dev_idx_row, size_t N, int64_t n, int64_t *dev_perm, int stream);

/* ---- solves ----------------------------------------------------------------
 * right_mul_pinv / left_mul_pinv (utils.py:98-109; SciPy lstsq -> LAPACK gelsd with
 * cond = eps): P = pinv(Omega) by one-sided Jacobi SVD on the device, singular values
 * below rcond*sigma_max dropped (rcond < 0 -> DBL_EPSILON).  Omega is (l, r)
 * contiguous; P is (r, l) contiguous.  The products A*P / P*B are ttsk_gemm calls. */
int ttsk_pinv(const double *dev_omega, int64_t l, int64_t r, double rcond, double *dev_pinv,
              int *host_rank /* may be NULL */, int stream);
/* The same in two phases for callers with several independent pseudo-inverses (assemble_sketched_tt,
 * sketch.py:400-443: one per mode): `begin` queues the fast path on `stream` and returns at once, `end`
 * waits for that stream, and runs the Jacobi SVD if the fast path was rejected.  One begin per library
 * stream may be outstanding; arguments of `end` repeat those of `begin`. */
int ttsk_pinv_begin(const double *dev_omega, int64_t l, int64_t r, double rcond, double *dev_pinv, int stream);
int ttsk_pinv_end(const double *dev_omega, int64_t l, int64_t r, double rcond, double *dev_pinv,
                  int *host_rank /* may be NULL */, int stream);
/* thin SVD of a small matrix (TensorTrain.round, tensor.py:446-484, and tt_svd.py:21-42, after a QR has
 * reduced the unfolding to its triangular factor): A (m, n) row-major, m >= n, by one-sided Jacobi --
 * n <= 1024 in one workgroup (asynchronous), 1024 < n <= 8192 over all compute units with a grid barrier
 * per round (blocks the host once).  US (m, n) = U diag(S), S (n) descending, Vt (n, n); A = US Vt. */
int ttsk_svd_small(const double *dev_A, int64_t m, int64_t n, double *dev_US, double *dev_S, double *dev_Vt,
                   int stream);
/* zero the strictly lower triangle of A (m, n) row-major: the triangular factor R = Q^T M of a thin
 * QR recovered by a product is upper triangular only up to rounding; np.linalg.qr (tensor.py:568)
 * returns exact zeros there, which is what keeps structurally zero singular values exactly zero. */
int ttsk_triu(double *dev_A, int64_t m, int64_t n, int stream);
/* thin QR of orth_step (sketch_dispatch.py:172, scipy.linalg.qr(mode="economic")):
 * A (m, n) row-major with m >= n is overwritten by Q (m, n); Householder with LAPACK's
 * sign convention.  R is not returned (the reference discards it). */
int ttsk_qr_thin(double *dev_A, int64_t m, int64_t n, int stream);
/* orth_step (sketch_dispatch.py:160-174) as ONE call with no read-back: Q (m, k) = qr_thin(Psi_mat pinv(Omega)), k = l,
 * Psi_mat (m, r2) row-major, Omega (l, r2) -- or Omega == NULL: Q = qr_thin(Psi_mat), k = r2 (hmt_sketch).  Same Q as
 * ttsk_pinv + product + ttsk_qr_thin on their fast paths (normal equations, CholeskyQR2, LAPACK's column signs) for
 * ranks up to 256.  The acceptance tests of those factorisations are NOT waited for: a rejection (Omega rank deficient
 * or the diagonal of its Cholesky factor spread by more than 3e4, that of Psi_mat Omega^+ by more than 1e6 -- the spread
 * bounds kappa from below, a matrix with kappa ten times the gate usually still passes) sets the stream's deferred flag and
 * leaves Q meaningless; the caller reads the flag once when the whole sketch is queued (ttsk_deferred_status) and then
 * repeats it through ttsk_pinv / ttsk_qr_thin.  TTSK_ERR_UNSUPPORTED outside the fast path (ranks > 256). */
int ttsk_orth_step(const double *dev_psi, int64_t m, int64_t r2, const double *dev_omega, int64_t l, double *dev_q,
                   int stream);
/* The same in two pieces for orthogonal_sketch, whose d - 1 Omega are all known before its sequential loop over the modes
 * starts: the pseudo-inverses of `count` matrices of ONE shape (l, r) with every stage as one batched launch (fast path
 * as in ttsk_orth_step, min(l, r) <= 128, verdicts in `stream`'s deferred flag), then per mode Q = qr_thin(Psi_mat P)
 * with P (r2, l) given. */
int ttsk_pinv_batch_deferred(int count, const double *const *dev_omegas, int64_t l, int64_t r, double *const *dev_pinvs,
                             int stream);
int ttsk_orth_step_pinv(const double *dev_psi, int64_t m, int64_t r2, const double *dev_pinv, int64_t l, double *dev_q,
                        int stream);
/* *host_flag = 1 if a factorisation queued by ttsk_orth_step on `stream` was rejected since the last call; waits for
 * the stream and clears the flag. */
int ttsk_deferred_status(int stream, int *host_flag);
/* orthogonal_sketch / hmt_sketch of a tensor train with tensor-train DRMs as ONE call (sketch.py:44-151,
 * sketch_dispatch.py:160-193, 202-275 with method = orthogonal / hmt; tensor_train_drm.py:71-88 for the chains):
 * right chain (and, orthogonal, left chain + Omega_mu) on the kernels of ttsk_tt_sketch, the pseudo-inverses batched,
 * then per mode T = (Q_0 .. Q_{mu-1})^T-chain (x) X_mu, Q_mu = qr_thin(T R_mu Omega_mu^+) (hmt: qr_thin(T R_mu)).
 *   n, s, X       as ttsk_tt_sketch
 *   rt, DR        right DRM, true ranks and cores in its walking order (mode d-1 first), rt[0] = 1
 *   lt, DL        left DRM (lt[0] = 1), or DL == NULL: hmt_sketch
 *   cores_out[d]  core mu (k_{mu-1}, n[mu], k_mu) with k_mu = lt[mu+1] (orthogonal) or rt[d-1-mu] (hmt), k_{-1} = k_{d-1} = 1
 *   omega_out     orthogonal: d - 1 matrices (lt[mu+1], rt[d-1-mu])
 * Verdicts deferred as in ttsk_orth_step (ttsk_deferred_status on `stream` afterwards).  TTSK_ERR_UNSUPPORTED: ranks
 * beyond 256, k_{mu-1} n[mu] < k_mu.  (Omega of one shape with min(l, r) <= 128: the pseudo-inverses
 * are batched launches; the sign reconstruction runs on stream + 1 and is joined back.) */
int ttsk_tt_orth_sketch(int d, const int64_t *n, const int64_t *s, const int64_t *lt, const int64_t *rt,
                        const double *const *X, const double *const *DL, const double *const *DR,
                        double *const *cores_out, double *const *omega_out, int stream);
/* the same for `count` tensor trains of ONE signature (n, s) against ONE pair of DRMs -- the streaming setting of
 * sketch.py:292-301, and the many same-shaped re-orthogonalisations of tt_gmres.py:293-299.  Up to 16 tensors whose
 * unfoldings are all at least twice as tall as wide, ranks <= 128: ONE chain of launches, every step (chain products,
 * pseudo-inverses, Gram / Cholesky / triangular products, sign reconstruction) over all tensors at once, one verdict for the
 * whole batch.  Otherwise as concurrent chains: tensor b on the library streams (stream + 2 (b mod 4), + 1), forked from and
 * joined back into `stream`, a verdict per tensor.
 *   X, cores_out     count * d pointers, tensor-major;   omega_out   count * (d - 1) pointers (orthogonal)
 *   dev_status       count ints in device memory: 1 = a fast factorisation of that tensor was rejected (repeat it on the
 *                    robust path: ttsk_pinv / ttsk_qr_thin); read after ttsk_sync(stream)
 * The verdicts come back in dev_status ALONE: whichever form ran, the deferred flag of every stream it used, `stream`
 * included, is clear afterwards (ttsk_deferred_status reads 0 on all of them).  A flag that an earlier, unrelated call left on
 * one of the OTHER streams is dropped; one left on `stream` itself counts against the batch's first tensor (the fused form:
 * against all).  (ttsk_tt_orth_sketch, the single call, sets the flag of its own stream only: its helper carries none.) */
int ttsk_tt_orth_sketch_batch(int count, int d, const int64_t *n, const int64_t *s, const int64_t *lt, const int64_t *rt,
                              const double *const *X, const double *const *DL, const double *const *DR,
                              double *const *cores_out, double *const *omega_out, int *dev_status, int stream);

/* The two products of a dense-tensor sketch with tensor-train DRMs that read the tensor, from ONE read of it (reference
 * dense_sketch.py:7-52, sketch_omega_dense / sketch_psi_dense, with the DRM matrices of tensor_train_drm.py:109-122):
 *   X (n0, Q, T) C order; C (n0, ll) the left DRM's first core; P (Q, r) the right DRM's matrix of one core less
 *   Z (ll, Q, T) = sum_b C[b, .] X[b, ., .]     the first left product (dense_sketch.py:13-14 at mu = 0)
 *   U (n0, r, T) = sum_q P[q, .] X[., q, .]     Psi_0 before its last core (dense_sketch.py:36-52 at mu = 0)
 * The same call one level down gives Z_1 and Psi_1 from Z_0 (rows (p', i_1), C = the left DRM's second core as a matrix): a
 * first extent beyond 64 runs as blocks of 64 rows (of 32 for ll > 20 or r > 40), Z summed over the blocks.
 * TTSK_ERR_UNSUPPORTED outside the kernel's cover: n0 a multiple of 32, T % 16 == 0, Q % 8 == 0, ll <= 32, r <= 64
 * (an odd r through a padded copy of P), Q T < 2^27, X, P and Z 16-byte aligned (the caller then forms the two
 * products separately). */
int ttsk_dense_first_pass(const double *dev_x, int64_t n0, int64_t Q, int64_t T, const double *dev_c, int64_t ll,
                          const double *dev_p, int64_t r, double *dev_z, double *dev_u, int stream);

/* ttsk_pinv for `count` (<= 32) matrices of ONE shape (l, r), min(l, r) <= 128: every stage of the fast attempt one batched
 * launch, the robust kernel queued behind it per matrix with that matrix's verdict as predicate; no read-back (utils.py:98-109
 * for the d - 1 Omega of an assembly).  TTSK_ERR_UNSUPPORTED outside that cover. */
int ttsk_pinv_batch(int count, const double *const *dev_omegas, int64_t l, int64_t r, double *const *dev_pinvs, int stream);
/* assemble_sketched_tt (sketch.py:400-443) as one call: direction 0 ("right") C_mu = Psi_mu pinv(Omega_mu), mu < d - 1,
 * C_{d-1} = Psi_{d-1}; direction 1 ("left") C_0 = Psi_0, C_{mu+1} = pinv(Omega_mu) Psi_{mu+1}.  lr / rr: the d - 1 sketch
 * ranks; psi[mu] (lr[mu-1], n[mu], rr[mu]) contiguous; omega[mu] (lr[mu], rr[mu]); work[mu]: rr[mu] * lr[mu] doubles that
 * receive pinv(Omega_mu).  Omega of one shape: the pseudo-inverses are batched launches on `stream`, and in direction 0 so
 * are the products of the interior pairs whose mode size is n[1].  Every other pair mu runs on the helper stream
 * (stream + 1 + mu) mod TTSK_NUM_STREAMS (pairs 8 apart share one; pair 7 is on `stream` itself) with ttsk_pinv's robust
 * fallback queued behind the fast attempt (no read-back); every helper is forked behind `stream` when its first pair reaches
 * it and joined into `stream` before the call returns. */
int ttsk_tt_assemble(int d, const int64_t *n, const int64_t *lr, const int64_t *rr, const double *const *dev_psi,
                     const double *const *dev_omega, double *const *dev_cores_out, double *const *dev_work, int direction,
                     int stream);
/* assemble_sketched_tt (sketch.py:400-443) for `count` sketches of one signature at once -- the to_tt() half of the
 * reference's recompression stream_sketch(tt, l, r).to_tt() (sketch.py:154-229, :279-280).  Per tensor b the contract of
 * ttsk_tt_assemble on psi + b d, omega + b (d - 1), cores_out + b d, work + b (d - 1); the core that is copied unchanged
 * (right: d - 1, left: 0) may alias its Psi.  All pairs of one Omega shape share a fixed number of launches on `stream`
 * (batched normal-equations pseudo-inverses, the Jacobi kernel predicated per matrix, one fused refined product
 * C = Psi P, R = Psi - C Omega, C += R P) when operands of one mode are equally spaced across the tensors; no host
 * synchronisation, no stream forked.  TTSK_ERR_ARG before anything is queued for count < 1, a NULL pointer or a
 * direction other than 0 / 1. */
int ttsk_tt_assemble_batch(int count, int d, const int64_t *n, const int64_t *lr, const int64_t *rr,
                           const double *const *dev_psi /* count * d */, const double *const *dev_omega /* count * (d - 1) */,
                           double *const *dev_cores_out /* count * d */, double *const *dev_work /* count * (d - 1) */,
                           int direction, int stream);
/* ---- multi-GPU: one RCCL sum of the packed partial sketch ------------------
 * SketchContainer.__add__ across ranks (sketch_container.py:61-69). */
int ttsk_comm_unique_id(void *host_id128);                 /* rank 0: 128-byte id */
int ttsk_comm_init(const void *host_id128, int rank, int nranks);
int ttsk_comm_allreduce_sum(double *dev_buf, size_t n, int stream);
int ttsk_comm_reduce_sum(double *dev_buf, size_t n, int root, int stream);
/* every rank's n doubles in rank order into dev_recv (n * nranks doubles): placement of the blocks of a
 * rank-sharded sketch (blocked_stream_sketch, sketch.py:364-397,446-473 -- disjoint blocks, no sum) */
int ttsk_comm_allgather(const double *dev_send, double *dev_recv, size_t n, int stream);
int ttsk_comm_allreduce_max(double *dev_buf, size_t n, int stream);   /* elementwise max, in place */
/* A failed ttsk_comm_init leaves no communicator behind (the call can be repeated, and the process
 * exits cleanly); destroy is a no-op without one. */
int ttsk_comm_destroy(void);

#ifdef __cplusplus
}
#endif
#endif /* TTSK_H */
