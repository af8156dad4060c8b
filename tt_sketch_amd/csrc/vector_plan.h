// What the three vector entry points (vector_ops.hip) are launched with, decided on the host: the argument checks of
// ttsk_copy_strided, ttsk_sum_slices and ttsk_axpby, the copy kernel's argument with its padding to five dimensions, the
// route of the slice sum (16-byte or 8-byte loads) and the grid of each launch against its cap.  The entry points call the
// plan, set the error and launch; blocks == 0 is a call with nothing to do (TTSK_OK, no launch).
//
// Plain C++: no HIP types, so that the plans are compiled and checked by the host compiler alone
// (tests/test_vector_plan.py) before any kernel reads them.  Pointers are tested for NULL and alignment, never dereferenced.
// (No kernel of this family indexes an extent with an int -- the copy counts in int64_t, the other two in size_t -- so
// PLAN_MAX_EXTENT bounds nothing here; what is refused as unsupported is a number of elements that int64_t cannot hold.)
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "ttsk.h"
#include "plan_common.h"

namespace ttsk {

constexpr int VEC_THREADS = 256;                 // threads of a workgroup, all three kernels
constexpr int COPY_MAX_DIMS = 5;                 // digits of the copy kernel's index decomposition
constexpr int64_t COPY_BLOCKS_MAX = 4096;        // workgroups of a copy at most: beyond, the grid-stride loop
constexpr int64_t AXPBY_BLOCKS_MAX = 4096;       // of an axpby
constexpr int64_t SUM_SLICES_BLOCKS_MAX = 8192;  // of a slice sum, either route

// the copy kernel's argument: dimension a of the call is digit a + 5 - ndim; the digits in front are (1, 0, 0)
struct CopyDesc {
    int64_t shape[5], ds[5], ss[5];
    int64_t total;
};

struct CopyPlan {
    CopyDesc c;
    int64_t blocks;              // workgroups; 0: nothing to copy
    char msg[200];               // why not, when the status is not TTSK_OK
};

struct SumSlicesPlan {
    int vector;                  // 1: sum_slices_kernel on double2; 0: sum_slices_scalar_kernel
    size_t stride, n;            // in the route's unit: halved on the vector route
    int64_t blocks;              // workgroups; 0: n == 0
    char msg[200];
};

struct AxpbyPlan {
    int64_t blocks;              // workgroups; 0: n == 0
    char msg[200];
};

// ceil(n / VEC_THREADS) against a cap, for any size_t (n + 255 may wrap)
inline int64_t vec_blocks(size_t n, int64_t cap)
{
    const size_t b = n / VEC_THREADS + (n % VEC_THREADS ? 1 : 0);
    return b > (size_t)cap ? cap : (int64_t)b;
}

inline int copy_strided_plan(const double *dst, const double *src, int ndim, const int64_t *shape, const int64_t *dst_strides,
                             const int64_t *src_strides, CopyPlan *p)
{
    *p = CopyPlan{};
    if (ndim < 0 || ndim > COPY_MAX_DIMS) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_copy_strided: ndim = %d is outside 0 .. %d", ndim, COPY_MAX_DIMS);
    if (ndim > 0 && (!shape || !dst_strides || !src_strides)) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_copy_strided: NULL shape or strides with ndim = %d", ndim);
    CopyDesc &c = p->c;
    bool empty = false;
    for (int a = 0; a < COPY_MAX_DIMS; ++a) {
        const int src_a = a - (COPY_MAX_DIMS - ndim);
        if (src_a >= 0) {
            c.shape[a] = shape[src_a];
            c.ds[a] = dst_strides[src_a];
            c.ss[a] = src_strides[src_a];
        } else {
            c.shape[a] = 1;
            c.ds[a] = 0;
            c.ss[a] = 0;
        }
        if (c.shape[a] < 0) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_copy_strided: negative extent shape[%d] = %lld", src_a, (long long)c.shape[a]);
        if (c.shape[a] == 0) empty = true;
    }
    if (empty) return TTSK_OK;               // c.total = 0, blocks = 0: NULL pointers allowed
    if (!dst || !src) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_copy_strided: NULL dst or src with elements to copy");
    int64_t total = 1;
    for (int a = 0; a < COPY_MAX_DIMS; ++a)
        if (__builtin_mul_overflow(total, c.shape[a], &total))
            PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_copy_strided: the product of the extents does not fit in int64_t");
    // the kernel's index runs up to one grid stride past total before its loop ends
    if (total > INT64_MAX - COPY_BLOCKS_MAX * VEC_THREADS)
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_copy_strided: the product of the extents and one grid stride do not fit in int64_t");
    c.total = total;
    p->blocks = total / VEC_THREADS + (total % VEC_THREADS ? 1 : 0);
    if (p->blocks > COPY_BLOCKS_MAX) p->blocks = COPY_BLOCKS_MAX;
    return TTSK_OK;
}

inline int sum_slices_plan(const double *dst, const double *src, int nb, size_t stride, size_t n, int accumulate, SumSlicesPlan *p)
{
    *p = SumSlicesPlan{};
    if (!dst || !src) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_sum_slices: NULL dst or src");
    if (nb < 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_sum_slices: nb = %d must be positive", nb);
    if (accumulate != 0 && accumulate != 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_sum_slices: accumulate = %d is neither 0 nor 1", accumulate);
    if (n == 0) return TTSK_OK;
    // 16-byte loads need whole pairs: an even length, an even distance of the slices, both bases on 16 bytes
    p->vector = !(n & 1) && !(stride & 1) && !((uintptr_t)dst & 15) && !((uintptr_t)src & 15);
    p->stride = p->vector ? stride / 2 : stride;
    p->n = p->vector ? n / 2 : n;
    p->blocks = vec_blocks(p->n, SUM_SLICES_BLOCKS_MAX);
    return TTSK_OK;
}

inline int axpby_plan(const double *y, const double *x, double a, double b, size_t n, AxpbyPlan *p)
{
    (void)a; (void)b;
    *p = AxpbyPlan{};
    if (n == 0) return TTSK_OK;
    if (!y || !x) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_axpby: NULL y or x with n = %zu", n);
    p->blocks = vec_blocks(n, AXPBY_BLOCKS_MAX);
    return TTSK_OK;
}

}  // namespace ttsk
