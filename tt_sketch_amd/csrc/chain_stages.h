// The workgroup-level stages of a fused chain step, each defined once for chain_step_kernel (chain_fused.h) and
// chain_wide_kernel (chain_wide.h).  Device function templates only, no kernels.
//
//   chain_block_unit     workgroup -> (problem, unit), units of one kind on one XCD
//   chain_e_fill_gather  one loader wave's pieces of the E image of slice k, gathered from the core (chain_plan.h: e_image_unit)
//
// KA is the kernel-argument struct (ChainStep, ChainWide: the same names for the same things).  It is taken by reference,
// and so is a scalar a caller may hold in it: a field is then loaded where it is used, as in the kernels before these
// functions existed -- taken by value it is loaded at the call, and the register allocation of the wave bodies behind
// it moves ("Chain-step stages").
//
// The W image and the stages of a compute wave (X ring, phase A, T store, phase B, slab store) are still written out in
// both kernels: DESIGN.md says what sharing them did to the kernels' registers.
#pragma once
#include "chain_plan.h"
#include "skinny.h"

namespace ttsk {

// blocks b and b + 8 share an XCD: with xcd_map the units are dealt over the XCDs, all problems of a unit to the same one
// (they read the same E_k)
__device__ __forceinline__ void chain_block_unit(const int xcd_map, const int &units, int &prob, int &unit)
{
    if (xcd_map) {
        const int upx = units >> 3, xcd = blockIdx.x & 7, j = blockIdx.x >> 3;
        unit = xcd * upx + j % upx;
        prob = j / upx;
    } else {
        prob = blockIdx.x / units;
        unit = blockIdx.x - prob * units;
    }
}

// Loader li of nl: pieces li, li + nl, ... (64 units = 1 KB per instruction) of the image of slice k, rows a0 .. of E_k;
// rowstride = n A2, the elements between two rows of a slice.  Unit u of section sec (rows 2 sec, 2 sec + 1) is columns
// (2 (u >> 1), + 1) of row 2 sec + (u & 1); lanes (kq in {0, 1}, x) of a fragment read 16 consecutive units.  Rows beyond A
// repeat row A - 1: they meet exact zeros of T.
// (A rolled loop: unrolled, the LDS destinations are hoisted into scalar registers and the whole kernel starts spilling.)
// ODD (odd A2 possible: rows are only 8-byte aligned): see e_image_unit_from; the one unit per row of the last slice that
// would reach past the core is patched with an 8-byte load -- rows 0 .. rows - 1 of the image, by one wave (nl = 1).
template <bool ODD, class KA>
__device__ __forceinline__ void chain_e_fill_gather(const KA &a, double *dst, const int k, const int a0, const int A2P, const uint32_t inv,
                                                    const int64_t rowstride, const int NI, const int li, const int nl, const int lane,
                                                    const int rows = 0)
{
    const double *Ek = a.E + (int64_t)k * a.A2;
    const bool tail = ODD && (a.A2 & 1) && k == a.n - 1;
#pragma unroll 2
    for (int m = li; m < NI; m += nl) {
        const uint32_t U = 64u * (uint32_t)m + (uint32_t)lane;
        const EUnit un = ODD ? e_image_unit_from(U, inv, a0, a.A, a.A2, A2P, tail) : e_image_unit(U, inv, a.A, a.A2, A2P);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(Ek + un.row * rowstride + un.col),
                                         (__attribute__((address_space(3))) void *)(dst + m * 128), 16, 0, 0);
    }
    if constexpr (ODD) {
        if (tail) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // after the units have landed
            if (lane < rows) {
                const int row = a0 + lane < a.A ? a0 + lane : a.A - 1;
                dst[e_image_at(lane, a.A2 - 1, A2P)] = Ek[row * rowstride + a.A2 - 1];
            }
        }
    }
}

}  // namespace ttsk
