// Wave and workgroup primitives of libttsk's kernels (gfx950, wave64): each device idiom is defined here once.
#pragma once
#include <hip/hip_runtime.h>

namespace ttsk {

// Fragment reads of tiles p, p + 1 (256 bytes apart) must NOT be paired into ds_read2_b64: its 16-lane groups bank modulo
// 32 dwords, and this layout's interleaved k-pairs (lane stride 16 bytes) then collide two by two -- 16 LDS cycles per pair of
// fragments; two ds_read_b64 (32-lane halves, modulo 64 dwords) are conflict-free on it: 4 cycles (MI355X_MICROARCH.md, LDS
// table).  A volatile access is what the compiler does not combine; the reads keep their place in the instruction stream, which
// is where the look-ahead of the k-block loops wants them anyway.
#define LDS_UNPAIRED(x) (*(const volatile __attribute__((address_space(3))) double *)(&(x)))

typedef double v4d __attribute__((ext_vector_type(4)));

// v_mfma_f64_16x16x4_f64: A lane l holds A[m=l&15][k=l>>4], B lane l holds
// B[k=l>>4][n=l&15]; D reg j of lane l is D[row=(l>>4)+4j][col=l&15].
__device__ __forceinline__ v4d mfma16(double a, double b, v4d c)
{
    return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}

// v_mfma_f64_4x4x4_f64 (4 blocks).  Measured on MI355X (profiles/scripts/mfma_probe2.hip, mfma_mix.hip; DESIGN.md
// section 4): both forms reach the pipe rate -- 16x16x4 one instruction per 64 cycles and SIMD (77.7 TF/s at 2.4 GHz),
// 4x4x4 one per 16-17 cycles (75 TF/s), freely mixed.  (Round 1 read 49 vs 65 TF/s off a probe compiled with
// __launch_bounds__(256): there hipcc keeps the accumulators in AGPRs and copies them around every instruction.  The same
// happened to the gemm kernel until it declared two waves per SIMD.)  The 4x4x4 form multiplies, for each of the four lane
// sub-groups beta (lanes 16k + 4 beta + {0..3}), the 4x4 blocks A[4beta+i][k] (lane 4beta+i+16k) and B[k][4beta+j]
// (lane 4beta+j+16k) into D[4beta+i][4beta+j] at lane 16i+4beta+j, i.e. the diagonal 4x4 blocks of the 16x16 product of
// the SAME operand registers the 16x16x4 form takes.
__device__ __forceinline__ double mfma4(double a, double b, double c)
{
    return __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c, 0, 0, 0);
}

// Sum over the 64 lanes of a wave, in every lane: the xor butterfly from 32 down to 1 (at step o a lane adds the value of
// lane ^ o to its own).
__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// Lanes of one wave hand data to each other through LDS: the hardware runs a wave's LDS accesses in order, this keeps the
// compiler from reordering them.
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Workgroup barrier for data handed over through LDS.
__device__ __forceinline__ void lds_barrier()
{
    // LDS traffic of this wave is complete, nothing moves across; vector-memory loads stay in flight
    // (__syncthreads() would wait for them too)
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// Sums of W values over a workgroup of 256 threads (four waves): thread j < W returns the total of s[j] (every other
// thread that of s[0]); the caller stores, adds or accumulates it.  THE ORDER, which is what "fixed order: the same bits
// on every call" means throughout the library: wave_sum() inside each wave, then the four waves as (w0 + w1) + (w2 + w3).
// What a thread sums into s[] before the call (ascending, strided by the grid or by 256) is the caller's and is stated
// there.  Ends in no barrier: one call per kernel, or a __syncthreads() before the next.
template <int W>
__device__ __forceinline__ double block_total(double (&s)[W])
{
    __shared__ double ws[4][W];
#pragma unroll
    for (int j = 0; j < W; ++j) s[j] = wave_sum(s[j]);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int j = 0; j < W; ++j) ws[threadIdx.x >> 6][j] = s[j];
    __syncthreads();
    const int j = threadIdx.x < W ? threadIdx.x : 0;
    return (ws[0][j] + ws[1][j]) + (ws[2][j] + ws[3][j]);
}

}  // namespace ttsk
