// DRM cores packed for chain_step_kernel's loader.  A DRM core E[a][k][a'] never changes after it is sampled, and every
// launch of the fused chain step brings each slice E_k into LDS in one fixed permutation (chain_plan.h: e_image_unit).
// ttsk_drm_pack applies that permutation once: Epk[k][eunits] 16-byte units, slice k the LDS image of E_k byte for byte,
// so that the loader copies 1 KB pieces instead of gathering 16-byte units.  The images are kept in a registry keyed by
// the core's address; chain_fused_try asks it for every launch.  A packed core costs e_pack_bytes of device memory on top
// of the core: at rank 100 as much again.
#include <map>
#include <mutex>
#include "chain_fused.h"

namespace ttsk {

struct PackedCore {
    int A, n, A2, A2P, eunits;
    double *img;
};

static std::mutex g_pack_mu;
static std::map<const double *, PackedCore> g_packed;

// one 16-byte unit per thread: consecutive threads write consecutive units
__global__ __launch_bounds__(256) void chain_pack_kernel(const double *__restrict__ E, double *__restrict__ Epk, int A, int n, int A2, int A2P,
                                                         int eunits, uint32_t inv)
{
    const int k = blockIdx.y;
    const int U = blockIdx.x * 256 + threadIdx.x;
    if (U >= eunits) return;
    const EUnit un = e_image_unit((uint32_t)U, inv, A, A2, A2P);
    const double2 v = *(const double2 *)(E + ((int64_t)un.row * n + k) * A2 + un.col);
    *(double2 *)(Epk + ((int64_t)k * eunits + U) * 2) = v;
}

const double *drm_packed_lookup(const double *E, int A, int n, int A2, int A2P, int eunits)
{
    std::lock_guard<std::mutex> lk(g_pack_mu);
    const auto it = g_packed.find(E);
    if (it == g_packed.end()) return nullptr;
    const PackedCore &p = it->second;
    return p.A == A && p.n == n && p.A2 == A2 && p.A2P == A2P && p.eunits == eunits ? p.img : nullptr;
}

void drm_packed_clear()
{
    std::lock_guard<std::mutex> lk(g_pack_mu);
    for (auto &kv : g_packed) (void)hipFree(kv.second.img);
    g_packed.clear();
}

}  // namespace ttsk

using namespace ttsk;

extern "C" int ttsk_drm_pack(const double *core, int A, int n, int A2, int stream)
{
    TTSK_STREAM(st, stream);
    TTSK_ARG(core && A >= 1 && n >= 1 && A2 >= 1, "ttsk_drm_pack: bad argument");
    int A2P, eunits;
    if (((uintptr_t)core & 15) || !chain_e_image(A, A2, A2P, eunits) || eunits >= (1 << 16) || n > 65535) {
        set_error("ttsk_drm_pack: the fused chain step has no image for a core of ranks (%d, %d), n = %d", A, A2, n);
        return TTSK_ERR_UNSUPPORTED;
    }
    if (drm_packed_lookup(core, A, n, A2, A2P, eunits)) return TTSK_OK;
    int rc = ttsk_drm_unpack(core);                    // registered with other extents
    if (rc != TTSK_OK) return rc;
    double *img = nullptr;
    TTSK_HIP(hipMalloc(&img, (size_t)e_pack_bytes(n, eunits)));
    rc = launch(chain_pack_kernel, dim3((eunits + 255) / 256, n), 256, 0, st, core, img, A, n, A2, A2P, eunits, e_image_inv(A2P));
    // the image is read by launches on any stream from here on: it is complete before it is registered
    const hipError_t e = rc == TTSK_OK ? hipStreamSynchronize(st) : hipSuccess;
    if (rc != TTSK_OK || e != hipSuccess) {
        (void)hipFree(img);
        if (rc == TTSK_OK) set_error("ttsk_drm_pack: %s", hipGetErrorString(e));
        return TTSK_ERR_HIP;
    }
    std::lock_guard<std::mutex> lk(g_pack_mu);
    g_packed[core] = PackedCore{A, n, A2, A2P, eunits, img};
    return TTSK_OK;
}

extern "C" int ttsk_drm_unpack(const double *core)
{
    double *img = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_pack_mu);
        const auto it = g_packed.find(core);
        if (it == g_packed.end()) return TTSK_OK;
        img = it->second.img;
        g_packed.erase(it);
    }
    TTSK_HIP(hipFree(img));                            // waits for the launches that still read it
    return TTSK_OK;
}
