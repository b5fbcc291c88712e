// sf_packed.hip — compact batches: sf_packed_batch and its arguments expanded
// into the arrays the sort phase reads, and the sparse copy back of a decided
// batch's waits and rule indices.  Product code.
#include "sf_launch.h"
#include "sf_pkargs.h"

namespace sf {

// ============================================================ compact batches
// sf_packed_batch -> the SoA DevBatch arrays (res, ts, count, flags, entry_ref,
// create_ts).  EXIT events and count-0 events take the next value of the
// sparse exit_ref / exit_cts / count_ext arrays: a per-tile count, one scan of
// the tile counts, then each tile's own scan (PK_T threads x PK_PER events).
constexpr uint32_t PK_T = 256, PK_PER = 16, PK_TILE = PK_T * PK_PER;
struct PkIn { const uint64_t* ev; const int64_t* xref; const int64_t* xcts; const int32_t* cext; int64_t base;
              uint32_t n, n_exit, n_cext;
              const uint32_t* ev4; const uint32_t* ms_end; uint32_t n_ms; };   // the narrow form: ev null
struct PkOut { uint32_t* res; int64_t* ts; int32_t* cnt; uint8_t* flags; int64_t* eref; int64_t* cts; };

__device__ __forceinline__ uint32_t pk_flags(uint64_t w) { return (uint32_t)(w >> SF_PK_FLAGS_SHIFT) & 0x1fu; }
__device__ __forceinline__ uint32_t pk_count(uint64_t w) { return (uint32_t)(w >> SF_PK_COUNT_SHIFT) & 0x7fu; }
// the narrow form's word as the 8-byte one without the time (res, acquireCount, flags)
__device__ __forceinline__ uint64_t pk_widen(uint32_t w) {
    return (uint64_t)(w & 0xffffffu) | ((uint64_t)((w >> SF_PK4_COUNT_SHIFT) & 7u) << SF_PK_COUNT_SHIFT) |
           ((uint64_t)(w >> SF_PK4_FLAGS_SHIFT) << SF_PK_FLAGS_SHIFT);
}
__device__ __forceinline__ uint64_t pk_word(const PkIn& in, uint32_t i) {
    return in.ev4 ? pk_widen(in.ev4[i]) : in.ev[i];
}
// first m in [lo, hi) with ms_end[m] > i (hi when none)
__device__ __forceinline__ uint32_t pk_ms_search(const uint32_t* ms_end, uint32_t lo, uint32_t hi, uint32_t i) {
    while (lo < hi) { const uint32_t m = lo + (hi - lo) / 2; if (ms_end[m] > i) hi = m; else lo = m + 1; }
    return lo;
}
constexpr uint32_t PK_ME = 1024;   // ms_end entries of a tile staged in LDS (longer spans search HBM)

__global__ void __launch_bounds__(PK_T) k_pk_count(PkIn in, uint2* tile_cnt) {
    __shared__ uint32_t sx, sc;
    if (threadIdx.x == 0) { sx = 0; sc = 0; }
    __syncthreads();
    uint32_t x = 0, c = 0;
    const uint32_t t0 = blockIdx.x * PK_TILE;
    for (uint32_t k = 0; k < PK_PER; k++) {
        const uint32_t i = t0 + k * PK_T + threadIdx.x;
        if (i >= in.n) break;
        const uint64_t w = pk_word(in, i);
        x += (pk_flags(w) & SF_EV_EXIT) ? 1u : 0u;
        c += pk_count(w) == 0 ? 1u : 0u;
    }
    x = (uint32_t)wave_sum(x); c = (uint32_t)wave_sum(c);
    if ((threadIdx.x & 63) == 0) { atomicAdd(&sx, x); atomicAdd(&sc, c); }
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = make_uint2(sx, sc);
}

// exclusive scan of the tile counts (one workgroup); err when a sparse array is short
__global__ void __launch_bounds__(1024) k_pk_scan(uint2* tile_cnt, uint32_t nt, PkIn in, int32_t* err) {
    __shared__ uint32_t wx[16], wc[16];
    __shared__ uint32_t cx, cc;
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    if (threadIdx.x == 0) { cx = 0; cc = 0; }
    __syncthreads();
    for (uint32_t b0 = 0; b0 < nt; b0 += 1024) {
        const uint32_t i = b0 + threadIdx.x;
        const uint2 v = i < nt ? tile_cnt[i] : make_uint2(0u, 0u);
        const uint32_t ix = (uint32_t)wave_scan_add((int)v.x), ic = (uint32_t)wave_scan_add((int)v.y);
        if (lane == 63) { wx[wv] = ix; wc[wv] = ic; }
        __syncthreads();
        uint32_t bx = cx, bc = cc;
        for (int k = 0; k < wv; k++) { bx += wx[k]; bc += wc[k]; }
        if (i < nt) tile_cnt[i] = make_uint2(bx + ix - v.x, bc + ic - v.y);
        __syncthreads();
        if (threadIdx.x == 1023) { cx = bx + ix; cc = bc + ic; }
        __syncthreads();
    }
    if (threadIdx.x == 0 && (cx > in.n_exit || cc > in.n_cext)) *err = SF_ERR_INVALID;
    // the narrow form's time table must cover every event
    if (threadIdx.x == 0 && in.ev4 && (in.n_ms == 0 || in.ms_end[in.n_ms - 1] != in.n)) *err = SF_ERR_INVALID;
}

// coalesced: round k of a tile holds events t0 + 256 k + thread, scanned in
// that (batch) order with a carry from round to round
// The narrow form's time: event i is at ts_base + the first m with
// ms_end[m] > i; the tile's first millisecond is searched once, the next
// PK_ME entries staged in LDS.
__global__ void __launch_bounds__(PK_T) k_pk_expand(PkIn in, const uint2* tile_base, PkOut out) {
    __shared__ uint32_t wx[PK_T / 64], wc[PK_T / 64];
    __shared__ uint32_t sme[PK_ME];
    __shared__ uint32_t s_m0;
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    const uint2 tb = tile_base[blockIdx.x];
    uint32_t cx = tb.x, cc = tb.y;
    uint32_t m0 = 0;
    if (in.ev4) {
        if (threadIdx.x == 0) s_m0 = pk_ms_search(in.ms_end, 0, in.n_ms, blockIdx.x * PK_TILE);
        __syncthreads();
        m0 = s_m0;
        for (uint32_t j = threadIdx.x; j < PK_ME; j += PK_T) sme[j] = m0 + j < in.n_ms ? in.ms_end[m0 + j] : 0xffffffffu;
        __syncthreads();
    }
    for (uint32_t k = 0; k < PK_PER; k++) {
        const uint32_t i = blockIdx.x * PK_TILE + k * PK_T + threadIdx.x;
        const bool in_b = i < in.n;
        const uint64_t w = in_b ? pk_word(in, i) : 0ull;
        const uint32_t f = pk_flags(w), c8 = pk_count(w);
        const uint32_t x = (in_b && (f & SF_EV_EXIT)) ? 1u : 0u, c = (in_b && c8 == 0) ? 1u : 0u;
        const uint32_t ix = (uint32_t)wave_scan_add((int)x), ic = (uint32_t)wave_scan_add((int)c);
        if (lane == 63) { wx[wv] = ix; wc[wv] = ic; }
        __syncthreads();
        uint32_t bx = cx + ix - x, bc = cc + ic - c, tx = 0, tc = 0;
        for (int q = 0; q < PK_T / 64; q++) {
            if (q < wv) { bx += wx[q]; bc += wc[q]; }
            tx += wx[q]; tc += wc[q];
        }
        __syncthreads();
        cx += tx; cc += tc;
        if (!in_b) continue;
        out.res[i] = (uint32_t)w;
        if (in.ev4) {
            uint32_t m;
            if (sme[PK_ME - 1] > i) {
                uint32_t lo = 0, hi = PK_ME;
                while (lo < hi) { const uint32_t md = (lo + hi) / 2; if (sme[md] > i) hi = md; else lo = md + 1; }
                m = m0 + lo;
            } else {
                m = pk_ms_search(in.ms_end, m0 + PK_ME, in.n_ms, i);
            }
            out.ts[i] = in.base + (int64_t)m;
        } else {
            out.ts[i] = in.base + (int64_t)((w >> 32) & 0xfffffu);
        }
        out.flags[i] = (uint8_t)f;
        out.cnt[i] = c8 ? (int32_t)c8 : (bc < in.n_cext ? in.cext[bc] : 0);
        if (f & SF_EV_EXIT) {
            out.eref[i] = bx < in.n_exit ? in.xref[bx] : -1;
            if (out.cts) out.cts[i] = (in.xcts && bx < in.n_exit) ? in.xcts[bx] : 0;
        } else {
            out.eref[i] = -1;
            if (out.cts) out.cts[i] = 0;
        }
    }
}

// Sparse copy back of a packed batch's verdicts (sf_sparse_verdicts): the
// nonzero waits and rule indices as (index << 32 | value), any order.
// counts[0], counts[1]: lengths.  One workgroup per SV_TILE events and one
// atomic per workgroup and list: a counter bumped once per wavefront (2M
// atomics on one address per 2^27 events) serialised the kernel to 13-17 ms
// beside the next batch (profiles/r06_e2e_trace.txt).  Each thread keeps its
// SV_PT values in registers between the count and the write.
constexpr int SV_T = 256, SV_PT = 16;
constexpr uint32_t SV_TILE = SV_T * SV_PT;
__global__ void __launch_bounds__(SV_T) k_sparse_verdicts(const int32_t* wait, const uint16_t* rule, uint32_t n,
                                                          unsigned long long* wl, unsigned long long* rl,
                                                          uint32_t* counts) {
    __shared__ uint32_t wsum[2][SV_T / 64];
    __shared__ uint32_t base[2];
    const uint32_t t0 = blockIdx.x * SV_TILE;
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    int32_t w[SV_PT];
    uint16_t r[SV_PT];
    uint32_t cw = 0, cr = 0;
#pragma unroll
    for (int k = 0; k < SV_PT; k++) {
        const uint32_t i = t0 + (uint32_t)k * SV_T + threadIdx.x;
        w[k] = i < n ? wait[i] : 0;
        r[k] = i < n ? rule[i] : (uint16_t)0;
        cw += w[k] != 0;
        cr += r[k] != 0;
    }
    const uint32_t sw = (uint32_t)wave_scan_add((int)cw), sr = (uint32_t)wave_scan_add((int)cr);
    if (lane == 63) { wsum[0][wave] = sw; wsum[1][wave] = sr; }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t tot = 0;
        for (int k = 0; k < SV_T / 64; k++) tot += wsum[threadIdx.x][k];
        base[threadIdx.x] = tot ? atomicAdd(&counts[threadIdx.x], tot) : 0u;
    }
    __syncthreads();
    uint32_t ow = base[0] + sw - cw, orr = base[1] + sr - cr;
    for (int k = 0; k < wave; k++) { ow += wsum[0][k]; orr += wsum[1][k]; }
#pragma unroll
    for (int k = 0; k < SV_PT; k++) {
        const unsigned long long i = t0 + (uint32_t)k * SV_T + threadIdx.x;
        if (w[k] != 0) wl[ow++] = (i << 32) | (uint32_t)w[k];
        if (r[k] != 0) rl[orr++] = (i << 32) | r[k];
    }
}
hipError_t launch_sparse_verdicts(const int32_t* wait, const uint16_t* rule, uint32_t n, unsigned long long* wl,
                                  unsigned long long* rl, uint32_t* counts, hipStream_t s) {
    hipMemsetAsync(counts, 0, 8, s);
    if (n) hipLaunchKernelGGL(k_sparse_verdicts, dim3((n + SV_TILE - 1) / SV_TILE), dim3(SV_T), 0, s, wait, rule, n,
                              wl, rl, counts);
    return hipGetLastError();
}

// The arguments, elements and contexts of a packed batch (sf_pkargs.h), after
// nargs / atag are zero-filled on the same stream, in two grid-stride passes.
// k_pk_args_check validates every listed entry and every entry of the element
// CSR (copying the CSR, clamped to n_elems) and raises the batch's error flag
// on any defect.  k_pk_args then expands the listed events into the dense
// slot-major arrays -- only when the flag is clear, so the verdict is global:
// a refused table leaves every event without arguments, and in an accepted
// one exactly one thread writes an event (arg_event is strictly increasing
// as a whole).  The same pass copies elements, contexts and origins into the
// expanded region, which outlives the staged inputs.
constexpr uint32_t PKA_T = 256, PKA_MAX_BLOCKS = 2048;
__global__ void __launch_bounds__(PKA_T) k_pk_args_check(PkArgIn in, PkArgOut out, uint32_t span, int32_t* err) {
    bool bad = false;
    for (uint32_t t = blockIdx.x * PKA_T + threadIdx.x; t < span; t += gridDim.x * PKA_T) {
        if (t < in.n_arg_events) bad |= !pk_args_event_ok(in, t);
        if (in.elem_off && t <= in.n_values) bad |= !pk_args_elem_off(in, out, t);
    }
    if (bad) *err = SF_ERR_INVALID;
}
__global__ void __launch_bounds__(PKA_T) k_pk_args(PkArgIn in, PkArgOut out, PkCopy cp, uint32_t span, const int32_t* err) {
    // (the flag of the whole batch, k_pk_scan's included: an errored batch carries no arguments)
    const bool expand = *err == 0;
    for (uint32_t t = blockIdx.x * PKA_T + threadIdx.x; t < span; t += gridDim.x * PKA_T) {
        if (expand && t < in.n_arg_events) pk_args_event_put(in, out, t);
        if (cp.etag && t < in.n_elems) { cp.etag_out[t] = cp.etag[t]; cp.ebits_out[t] = cp.ebits[t]; }
        if (t < in.n) {
            if (cp.ctx) cp.ctx_out[t] = cp.ctx[t];
            if (cp.origin) cp.origin_out[t] = cp.origin[t];
        }
    }
}
hipError_t launch_pk_args(const PkArgIn& in, const PkArgOut& out, const PkCopy& cp, int32_t* err, hipStream_t s) {
    auto blocks = [](uint32_t span) { const uint32_t nb = (span + PKA_T - 1) / PKA_T; return nb < PKA_MAX_BLOCKS ? nb : PKA_MAX_BLOCKS; };
    uint32_t span = 0;
    if (in.n_arg_events) {
        // (the final sort pass gathers every slot of every event: the bytes no listed event writes are zero)
        hipError_t me = hipMemsetAsync(out.nargs, 0, in.n, s);
        if (me == hipSuccess) me = hipMemsetAsync(out.atag, 0, (size_t)in.n * in.arg_slots, s);
        if (me != hipSuccess) return me;
        span = in.n_arg_events;
        if (in.elem_off && in.n_values + 1 > span) span = in.n_values + 1;
        hipLaunchKernelGGL(k_pk_args_check, dim3(blocks(span)), dim3(PKA_T), 0, s, in, out, span, err);
        span = in.n_arg_events;
    }
    if (cp.etag && in.n_elems > span) span = in.n_elems;
    if ((cp.ctx || cp.origin) && in.n > span) span = in.n;
    if (!span) return hipGetLastError();
    hipLaunchKernelGGL(k_pk_args, dim3(blocks(span)), dim3(PKA_T), 0, s, in, out, cp, span, (const int32_t*)err);
    return hipGetLastError();
}

hipError_t launch_pk_expand(const uint64_t* ev, const uint32_t* ev4, const uint32_t* ms_end, uint32_t n_ms,
                            const int64_t* xref, const int64_t* xcts, const int32_t* cext,
                            int64_t base, uint32_t n, uint32_t n_exit, uint32_t n_cext, uint2* tile_cnt,
                            uint32_t* res, int64_t* ts, int32_t* cnt, uint8_t* flags, int64_t* eref, int64_t* cts,
                            int32_t* err, hipStream_t s) {
    if (!n) return hipSuccess;
    const PkIn in{ev, xref, xcts, cext, base, n, n_exit, n_cext, ev ? nullptr : ev4, ms_end, n_ms};
    const PkOut out{res, ts, cnt, flags, eref, cts};
    const uint32_t nt = (n + PK_TILE - 1) / PK_TILE;
    hipLaunchKernelGGL(k_pk_count, dim3(nt), dim3(PK_T), 0, s, in, tile_cnt);
    hipLaunchKernelGGL(k_pk_scan, dim3(1), dim3(1024), 0, s, tile_cnt, nt, in, err);
    hipLaunchKernelGGL(k_pk_expand, dim3(nt), dim3(PK_T), 0, s, in, (const uint2*)tile_cnt, out);
    return hipGetLastError();
}

}  // namespace sf
