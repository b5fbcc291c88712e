// The AuthorityRule mark pass (sf_authority.h): one kernel per batch, ahead of
// the sort, and only while rules are loaded.
//
// k_auth_mark reads res, origin and flags of every event (9 B) and writes the
// engine's effective flag byte (1 B): the caller's flags without the reserved
// bits, plus SF_EV_BLOCKED | EVF_AUTH where the resource's rule blocks the
// entry's origin (auth_flag).  Bandwidth-bound: a workgroup takes tiles of
// AUTH_TILE events; per tile a thread handles AUTH_TILE / (256 * AUTH_VEC)
// groups of AUTH_VEC consecutive events, group g of thread t at event
// (g * 256 + t) * AUTH_VEC, so one load instruction of a wavefront reads 1 KiB
// of res / origin (dwordx4 per lane) or 256 B of flags (dword per lane),
// contiguous.  All loads of a tile are issued before the first rule lookup,
// and a group's lookup goes step by step over its events (auth_slot of all,
// then the rule records, then the lists), so their gathers overlap.
// The lookup gathers auth_of[row] (4 B per event, served by L2 / the Infinity
// Cache for the hot rows of a skewed batch) and touches a rule's list only for
// rows that have one.  The group that crosses n, and every group of arrays
// that are not 16-byte aligned, goes event by event.  No LDS, no atomics.
#include <hip/hip_runtime.h>

#include "sf_internal.h"

namespace sf {

constexpr int AUTH_BLOCK = 256;
constexpr uint32_t AUTH_VEC = 4;
constexpr uint32_t AUTH_TILE = 4096;
constexpr uint32_t AUTH_GROUPS = AUTH_TILE / (AUTH_BLOCK * AUTH_VEC);
constexpr uint32_t AUTH_MAX_GRID = 2048;
static_assert(AUTH_GROUPS * AUTH_BLOCK * AUTH_VEC == AUTH_TILE, "tile = groups x threads x vector");
static_assert(AUTH_VEC == 4, "one dwordx4 of ids and one dword of flags per group");

template <bool VEC>
__global__ void __launch_bounds__(AUTH_BLOCK)
k_auth_mark(AuthTables t, const uint32_t* __restrict__ res, const uint32_t* __restrict__ origin,
            const uint8_t* __restrict__ flags, uint32_t n, uint8_t mark, uint8_t* __restrict__ out) {
    const size_t N = n;
    const size_t ntiles = (N + AUTH_TILE - 1) / AUTH_TILE;
    for (size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const size_t base = tile * AUTH_TILE + (size_t)threadIdx.x * AUTH_VEC;
        uint4 r[AUTH_GROUPS], o[AUTH_GROUPS];
        uint32_t f[AUTH_GROUPS];
        bool full[AUTH_GROUPS];
#pragma unroll
        for (uint32_t g = 0; g < AUTH_GROUPS; g++) {
            const size_t i0 = base + (size_t)g * AUTH_BLOCK * AUTH_VEC;
            full[g] = VEC && i0 + AUTH_VEC <= N;
            if (full[g]) {
                r[g] = *reinterpret_cast<const uint4*>(res + i0);
                o[g] = *reinterpret_cast<const uint4*>(origin + i0);
                f[g] = *reinterpret_cast<const uint32_t*>(flags + i0);
            }
        }
        // a full group in three steps, each over its 4 events before the next:
        // the auth_of gathers, the rule records of the events that have a rule,
        // the lists -- so the dependent gathers of 4 events are in flight together
#pragma unroll
        for (uint32_t g = 0; g < AUTH_GROUPS; g++) {
            const size_t i0 = base + (size_t)g * AUTH_BLOCK * AUTH_VEC;
            if (full[g]) {
                const uint32_t rr[AUTH_VEC] = {r[g].x, r[g].y, r[g].z, r[g].w};
                const uint32_t oo[AUTH_VEC] = {o[g].x, o[g].y, o[g].z, o[g].w};
                uint8_t ff[AUTH_VEC];
                uint32_t k[AUTH_VEC];
                AuthRule ru[AUTH_VEC];
#pragma unroll
                for (uint32_t e = 0; e < AUTH_VEC; e++) {
                    ff[e] = (uint8_t)(f[g] >> (8 * e)) & (uint8_t)~EVF_CALLER_STRIP;
                    k[e] = auth_markable(ff[e]) ? auth_slot(t, rr[e], oo[e]) : AUTH_NONE;
                }
#pragma unroll
                for (uint32_t e = 0; e < AUTH_VEC; e++) {
                    ru[e] = AuthRule{-1, 0, 0};
                    if (k[e] != AUTH_NONE) ru[e] = t.rule[k[e]];
                }
                uint32_t w = 0;
#pragma unroll
                for (uint32_t e = 0; e < AUTH_VEC; e++) {
                    if (k[e] != AUTH_NONE && auth_rule_blocks(t, ru[e], oo[e])) ff[e] |= mark;
                    w |= (uint32_t)ff[e] << (8 * e);
                }
                *reinterpret_cast<uint32_t*>(out + i0) = w;
            } else {
                for (size_t i = i0; i < i0 + AUTH_VEC && i < N; i++)
                    out[i] = auth_flag(t, res[i], origin[i], flags[i], mark);
            }
        }
    }
}

hipError_t launch_auth_mark(const AuthTables& t, const uint32_t* res, const uint32_t* origin, const uint8_t* flags,
                            uint32_t n, uint8_t mark, uint8_t* out, hipStream_t s) {
    if (!n) return hipSuccess;
    const size_t ntiles = ((size_t)n + AUTH_TILE - 1) / AUTH_TILE;
    const unsigned grid = (unsigned)(ntiles < AUTH_MAX_GRID ? ntiles : AUTH_MAX_GRID);
    const uintptr_t a = (uintptr_t)res | (uintptr_t)origin | (uintptr_t)flags | (uintptr_t)out;
    if ((a & 15) == 0) hipLaunchKernelGGL(k_auth_mark<true>, dim3(grid), dim3(AUTH_BLOCK), 0, s, t, res, origin, flags, n, mark, out);
    else hipLaunchKernelGGL(k_auth_mark<false>, dim3(grid), dim3(AUTH_BLOCK), 0, s, t, res, origin, flags, n, mark, out);
    return hipGetLastError();
}

}  // namespace sf
