// What the closing step of the inner product of two Hadamard products (hadamard_close.hip) is launched with, decided on the
// host: the argument checks and the cover of ttsk_hadamard_close, the kernel's argument, the split of the mode over the
// grid, the slab of partial tiles and the flops of the call.
//
// Plain C++: no HIP types, so that the plan is compiled and checked by the host compiler alone
// (tests/test_hadamard_close_host.py) before any kernel reads it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include "ttsk.h"
#include "plan_common.h"
#include "hadamard_plan.h"

namespace ttsk {

// The stages are those of hadamard_apply (hadamard_stages.h): gamma in chunks of HD_KC through LDS at HD_PITCH, HD_COLS
// values of gamma' per workgroup, HD_LDS bytes.  What is new is the split of the mode: the kernel sums over i, so i is not a grid index that
// comes for free.  A (p, c', gamma') tile count below HC_FILL is multiplied by cutting i into chunks until the grid holds
// HC_FILL workgroups: two per compute unit of a 256-CU device, which is what the kernel's registers and LDS allow to be
// resident.  Where the grid then ends in a round of HC_FILL that is less than nine tenths full, i is cut once more, up to
// HC_TRIES times: at S = s = 50, P = 2500 (628 tiles, a second round 23% full) three chunks of i take 5.9 ms where one took
// 8.6 ms, while cutting every shape four times finer (HC_FILL = 2048) cost the shapes that were full already 6 to 22%
// (DESIGN section 21).  The split depends on the extents alone, never on the device: the same bits everywhere.
constexpr int64_t HC_FILL = 512;
constexpr int64_t HC_TAIL_NUM = 9, HC_TAIL_DEN = 10;
constexpr int HC_TRIES = 16;

// the kernel's argument
struct HadamardCloseArgs {
    const double *Wl, *U, *V;
    double *work;
    int64_t sU[3];               // element strides of U over (gamma, i, gamma')
    int64_t sV[3];               // of V over (c, i, c')
    int S, S1, s, s1, n, P;
    int ptiles, ctiles, gblocks; // workgroups are (i chunk, p tile, c' tile, gamma' block), the last fastest
    int ichunks, iper;           // chunk q sums i = q iper .. min(n, (q + 1) iper)
};

struct HadamardClosePlan {
    HadamardCloseArgs a;
    int64_t blocks;              // workgroups of the launch
    int64_t slab;                // doubles of `work`: ichunks x P x S' s'
    double flops;                // 2 n P (S s s' + S S' s')
    char msg[200];               // why not, when the status is not TTSK_OK
};

// The filling rule above for `groups` tiles and a summed index of extent n (op_close_plan.h cuts its j by it too): chunk q
// sums q per .. min(n, (q + 1) per); returns the workgroups of the launch, groups x chunks.
inline int64_t hc_cut(int64_t groups, int64_t n, int *per, int *chunks)
{
    int64_t want = cdiv(HC_FILL, groups), blocks;
    for (int tries = 0;; ++tries, ++want) {
        if (want > n) want = n;
        *per = (int)cdiv(n, want);
        *chunks = (int)cdiv(n, *per);                               // no chunk is empty
        blocks = groups * *chunks;
        const int64_t rounds = cdiv(blocks, HC_FILL);
        // the last round of HC_FILL workgroups nearly full, or nothing left to cut
        if (HC_TAIL_DEN * blocks >= HC_TAIL_NUM * rounds * HC_FILL || want >= n || tries == HC_TRIES) break;
    }
    return blocks;
}

// The part of the plan that needs no pointers: dims are S, S', s, s', n, P.  ttsk_hadamard_close_layout is this.
inline int hadamard_close_layout(const int64_t *dims, HadamardClosePlan *p)
{
    static const char *const names[6] = {"S", "S'", "s", "s'", "n", "P"};
    *p = HadamardClosePlan{};
    if (!dims) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_hadamard_close: NULL argument");
    bool wide = false;
    if (const int rc = hadamard_extents("ttsk_hadamard_close", names, dims, &wide, p)) return rc;
    // ---- the cover
    if (wide) return hadamard_wide("ttsk_hadamard_close", p);
    HadamardCloseArgs &a = p->a;
    a.S = (int)dims[0]; a.S1 = (int)dims[1]; a.s = (int)dims[2]; a.s1 = (int)dims[3]; a.n = (int)dims[4]; a.P = (int)dims[5];
    a.ptiles = (int)cdiv(dims[5], 16);
    a.ctiles = (int)cdiv(dims[3], 16);
    a.gblocks = (int)cdiv(dims[1], HD_COLS);
    const int64_t tiles = (int64_t)a.ptiles * a.ctiles;             // below 2^56
    if (tiles > PLAN_MAX_EXTENT || tiles * a.gblocks > PLAN_MAX_EXTENT)
        PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_hadamard_close: 2^31 workgroups or more");
    p->blocks = hc_cut(tiles * a.gblocks, dims[4], &a.iper, &a.ichunks);
    if (p->blocks > PLAN_MAX_EXTENT) PLAN_FAIL(TTSK_ERR_UNSUPPORTED, "ttsk_hadamard_close: 2^31 workgroups or more");
    // a workgroup covers at most 16 x 16 x HD_COLS elements of its slice: the slab is below 2^14 x 2^31 doubles
    p->slab = dims[1] * dims[3] * dims[5] * a.ichunks;
    p->flops = 2.0 * (double)dims[4] * (double)dims[5] * ((double)dims[0] * dims[2] * dims[3] + (double)dims[0] * dims[1] * dims[3]);
    return TTSK_OK;
}

// strides in elements: U (gamma, i, gamma') then V (c, i, c'); work_doubles: what the caller's slab holds
inline int hadamard_close_plan(const double *Wl, const double *U, const double *V, const int64_t *dims, const int64_t *strides,
                               double *out, int accumulate, double *work, int64_t work_doubles, HadamardClosePlan *p)
{
    *p = HadamardClosePlan{};
    if (!Wl || !U || !V || !dims || !strides || !out || !work) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_hadamard_close: NULL argument");
    if (accumulate != 0 && accumulate != 1) PLAN_FAIL(TTSK_ERR_ARG, "ttsk_hadamard_close: accumulate = %d, 0 or 1", accumulate);
    const int rc = hadamard_close_layout(dims, p);
    if (rc) return rc;
    if (work_doubles < p->slab)
        PLAN_FAIL(TTSK_ERR_ARG, "ttsk_hadamard_close: a slab of %lld doubles, the plan needs %lld", (long long)work_doubles, (long long)p->slab);
    HadamardCloseArgs &a = p->a;
    a.Wl = Wl; a.U = U; a.V = V; a.work = work;
    for (int i = 0; i < 3; ++i) { a.sU[i] = strides[i]; a.sV[i] = strides[3 + i]; }
    return TTSK_OK;
}

}  // namespace ttsk
