// sf_scatter.hip — the verdict scatter that ends the decide phase
// (launch_scatter): statuses from sorted to submission order.  Product code.
#include "sf_launch.h"

namespace sf {

// ============================================================ verdict scatter
// Every deciding kernel leaves its statuses in sorted order (v_status); the
// caller's array is in submission order, a permutation away (perm).  One byte
// stored per event at a random address costs a partial-line write each (the
// lean QPS walk of config 2 spent half its time on them), so the statuses
// travel instead in bucketed passes whose every global store is part of a
// run: A buckets by submission index >> s1 (<= 256 buckets of 2^s1), B by
// index >> VS_REG inside an A bucket, C assembles each 2^VS_REG region in LDS
// and stores it with coalesced writes.  A record is (status << 24) | (the
// index bits below its bucket).  A permutation fills every bucket exactly, so
// bucket sizes are known and no histogram pass is needed: each workgroup
// counting-sorts its tile in LDS, claims a run per bucket with one global
// atomic, and writes the run.
#ifndef SF_VS_T
#define SF_VS_T 1024                 // 16 waves per workgroup: 256 x 32 ran the scatter 4.4 -> 2.3 ms slower
#define SF_VS_PER 8
#endif
constexpr uint32_t VS_T = SF_VS_T, VS_PER = SF_VS_PER, VS_TILE = VS_T * VS_PER;
// k_vs_bucket's LDS: hist / lbase / gbase (3 x 4 KiB), part, buf (4 B per record)
// and kb (2 B per record); a record's rank in its bucket is packed in 16 bits
static_assert(VS_TILE < 65536u, "k_vs_bucket packs a record's rank into 16 bits");
static_assert(3u * 1024u * 4u + VS_T * 4u + VS_TILE * 4u + VS_TILE * 2u <= 65536u,
              "k_vs_bucket LDS footprint over 64 KiB: retune SF_VS_T / SF_VS_PER");
constexpr uint32_t VS_DIRECT_MAX = 1u << 20;        // smaller batches: one direct scatter

// A (FIRST: sorted positions [blockIdx * VS_TILE, +VS_TILE) -> bucket idx >> s1)
// or B (records of A bucket blockIdx / tpb, tile blockIdx % tpb -> region idx >> VS_REG)
template <bool FIRST>
__global__ void __launch_bounds__(VS_T) k_vs_bucket(const uint32_t* perm, const uint8_t* v_status, const uint32_t* in,
                                                     uint32_t* out, uint32_t* cursor, uint32_t n, uint32_t s1,
                                                     uint32_t tpb, int32_t* err) {
    __shared__ uint32_t hist[1024], lbase[1024], gbase[1024], part[VS_T];
    __shared__ uint32_t buf[VS_TILE];
    __shared__ uint16_t kb[VS_TILE];
    const uint32_t tid = threadIdx.x;
    const uint32_t m1 = s1 >= 32 ? 0xffffffffu : (1u << s1) - 1u;
    uint32_t lo, hi, nk, bb = 0;
    if (FIRST) {
        lo = blockIdx.x * VS_TILE;
        hi = min(n, lo + VS_TILE);
        nk = (uint32_t)(((uint64_t)n + m1) >> s1);
    } else {
        bb = blockIdx.x / tpb;
        const uint64_t b0 = (uint64_t)bb << s1;
        const uint64_t bend = min((uint64_t)n, b0 + (1ull << s1));
        const uint64_t l = b0 + (uint64_t)(blockIdx.x % tpb) * VS_TILE;
        if (l >= bend) return;                           // (whole workgroup)
        lo = (uint32_t)l; hi = (uint32_t)min(bend, l + VS_TILE);
        nk = 1u << (s1 - VS_REG);
    }
    for (uint32_t k = tid; k < nk; k += VS_T) hist[k] = 0;
    __syncthreads();
    uint32_t rec[VS_PER], kr[VS_PER];                    // record, key << 16 | rank in the tile's bucket
#pragma unroll
    for (uint32_t r = 0; r < VS_PER; r++) {
        const uint32_t e = lo + r * VS_T + tid;
        kr[r] = 0xffffffffu;
        if (e < hi) {
            uint32_t key;
            if (FIRST) {
                const uint32_t i = perm[e];
                key = i >> s1; rec[r] = ((uint32_t)v_status[e] << 24) | (i & m1);
            } else {
                const uint32_t v = in[e];
                key = (v & m1) >> VS_REG; rec[r] = (v & 0xff000000u) | (v & ((1u << VS_REG) - 1u));
            }
            kr[r] = (key << 16) | atomicAdd(&hist[key], 1u);
        }
    }
    __syncthreads();
    // exclusive scan of the bucket counts (ceil(nk / VS_T) per thread), then one claim per bucket
    const uint32_t per = (nk + VS_T - 1) / VS_T;
    uint32_t sum = 0;
    for (uint32_t q = 0; q < per; q++) { const uint32_t k = tid * per + q; if (k < nk) sum += hist[k]; }
    // (wavefront scans, then the wavefronts' totals: one barrier)
    const uint32_t lane = tid & 63u, wv = tid >> 6;
    uint32_t incl = sum;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(incl, d, 64);
        if (lane >= d) incl += y;
    }
    if (lane == 63u) part[wv] = incl;
    __syncthreads();
    uint32_t run = incl - sum;
    for (uint32_t q = 0; q < wv; q++) run += part[q];
    for (uint32_t q = 0; q < per; q++) {
        const uint32_t k = tid * per + q;
        if (k >= nk) break;
        const uint32_t h = hist[k];
        lbase[k] = run; run += h;
        if (h) {
            const uint32_t c = FIRST ? k : 256u + bb * nk + k;
            const uint32_t g = atomicAdd(&cursor[c], h);
            // bucket capacity: what the permutation puts there (anything more is a broken permutation)
            const uint64_t first = FIRST ? ((uint64_t)k << s1) : (((uint64_t)bb * nk + k) << VS_REG);
            const uint64_t cap = min((uint64_t)(FIRST ? (1ull << s1) : (1ull << VS_REG)), (uint64_t)n - min((uint64_t)n, first));
            if ((uint64_t)g + h > cap) *err = SF_ERR_INVALID;
            gbase[k] = (uint32_t)first + g - lbase[k];       // destination of the tile's k-th record, minus k
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < VS_PER; r++)
        if (kr[r] != 0xffffffffu) {
            const uint32_t key = kr[r] >> 16, p = lbase[key] + (kr[r] & 0xffffu);
            buf[p] = rec[r]; kb[p] = (uint16_t)key;
        }
    __syncthreads();
    for (uint32_t k = tid; k < hi - lo; k += VS_T) {
        const uint32_t dst = gbase[kb[k]] + k;              // (a broken permutation: flagged above, kept in bounds)
        if (dst < n) out[dst] = buf[k];
    }
}

// C: region blockIdx (2^VS_REG submission indices) assembled in LDS, stored coalesced
__global__ void __launch_bounds__(VS_T) k_vs_region(const uint32_t* in, uint8_t* o_status, uint32_t n) {
    __shared__ __align__(16) uint8_t reg[1u << VS_REG];
    const uint32_t base = blockIdx.x << VS_REG;
    const uint32_t cnt = min(1u << VS_REG, n - base);
    for (uint32_t k = threadIdx.x; k < cnt; k += VS_T) {
        const uint32_t v = in[base + k];
        reg[v & ((1u << VS_REG) - 1u)] = (uint8_t)(v >> 24);
    }
    __syncthreads();
    uint8_t* o = o_status + base;
    if (((uintptr_t)o & 15) == 0) {
        for (uint32_t k = threadIdx.x; k < cnt / 16; k += VS_T) ((uint4*)o)[k] = ((const uint4*)reg)[k];
        for (uint32_t k = (cnt & ~15u) + threadIdx.x; k < cnt; k += VS_T) o[k] = reg[k];
    } else {
        for (uint32_t k = threadIdx.x; k < cnt; k += VS_T) o[k] = reg[k];
    }
}

__global__ void k_vs_direct(const uint32_t* perm, const uint8_t* v_status, uint8_t* o_status, uint32_t n) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) o_status[perm[j]] = v_status[j];
}

// statuses of a decided batch: sorted order -> the caller's array (submission order)
void launch_scatter(Work& w, uint32_t n, uint8_t* o_status, hipStream_t s) {
    if (n <= VS_DIRECT_MAX) {
        hipLaunchKernelGGL(k_vs_direct, dim3(blocks(n, 256)), dim3(256), 0, s, w.perm, w.v_status, o_status, n);
        return;
    }
    const uint32_t lg = 32u - (uint32_t)__builtin_clz(n - 1u);          // ceil(log2 n)
    const uint32_t s1 = std::max(VS_REG, lg - 8u);                      // <= 256 A buckets
    const uint32_t nb1 = (uint32_t)(((uint64_t)n + (1ull << s1) - 1) >> s1);
    const uint32_t nk = 1u << (s1 - VS_REG);
    hipMemsetAsync(w.vs_cursor, 0, (256 + (size_t)nb1 * nk) * 4, s);
    // staging: the sort's key buffers (dead once the batch is unpacked)
    hipLaunchKernelGGL(k_vs_bucket<true>, dim3((n + VS_TILE - 1) / VS_TILE), dim3(VS_T), 0, s, w.perm, w.v_status,
                       nullptr, w.keys_in, w.vs_cursor, n, s1, 0u, w.err);
    const uint32_t* regions = w.keys_in;
    if (s1 > VS_REG) {
        const uint32_t tpb = (1u << s1) / VS_TILE;
        hipLaunchKernelGGL(k_vs_bucket<false>, dim3(nb1 * tpb), dim3(VS_T), 0, s, nullptr, nullptr, w.keys_in,
                           w.keys_out, w.vs_cursor, n, s1, tpb, w.err);
        regions = w.keys_out;
    }
    hipLaunchKernelGGL(k_vs_region, dim3((n + (1u << VS_REG) - 1) >> VS_REG), dim3(VS_T), 0, s, regions, o_status, n);
}

}  // namespace sf
