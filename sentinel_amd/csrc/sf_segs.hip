// sf_segs.hip — the sort phase of a batch (launch_sort): gfx950 kernels of
// its tail and the host function that lays the phase out (product code).
//
// The phase is state-independent except for the engine clock and the error
// word, and runs on ONE stream, the sort stream, into the batch's own Work
// set: the engine sorts batch k + 1 there while batch k is decided on the
// decide phase's streams (sf_decide.hip), and joins the two with its own
// Slot events.  No fork or join happens inside the phase; the pipeline events
// it records (PipeEvent, sf_internal.h) are timing events only.
//
//   EV_SORT_START
//   radix sort     (sf_rsort.h) validate + map resource ids to shard-local keys;
//                  stable (key, payload) sort by resource: per-resource time
//                  order is the input order (LeapArray semantics need it); the
//                  last pass leaves keys, submission index (perm), the event's
//                  32-bit word (s_meta: time offset, flags, acquireCount), the
//                  origin and the arguments in sorted order
//   segflag clear
//   EV_SORTED
//   k_segs_red / k_segs_tscan / k_segs_out   (launch_segs3) segment table,
//                  head scan, per-segment flags, the engine clock and, with
//                  window rules loaded, the acquireCount prefix (pcg)
//   launch_classify (when it ends the sort phase, which is how the engine
//                  runs it: the origin index passes that follow read the
//                  routes; launch_decide can run it on stream A instead)
//     k_fill       Work::counters, lcounts, pass bits, far live exits cleared
//     EV_CLASSIFY_START
//     k_classify   light segments (by length class) -> lane lists; heavy ->
//                  window / stream lists and accumulator slots; long xflow
//                  segments -> the wave walk's list (WorkCounter slots)
//     k_fill_tiles fill tiles of the heavy segments of each class
//     EV_CLASSIFIED
//
// The exit pairing (k_gather_exit) and the THREAD run tables (launch_thr_prep)
// are state-independent too, but run at the head of the decide phase: the
// sort phase is the longer of the two pipelined phases.
#include "sf_launch.h"
#include "sf_rsort.h"
#include "sf_xflow.h"

namespace sf {

// ============================================================ segment table + prefixes (reduce, scan, rescan)
// The segment heads of the sorted keys and their inclusive count per
// position (head_scan = segment id + 1), the segment table (start, resource,
// flags) and, when the decide phase's window budgets need it, the inclusive
// prefix of the entries' acquireCounts (pcg: 0 for exits and EVF_SYSBLK
// entries; k_heavy_decide's greedy prefix), in one pipeline of three
// launches without any cross-workgroup waiting: per-tile totals, one
// workgroup scanning the tile totals, then every tile again from its prefix.
// (A decoupled look-back single pass measured 5 ms per batch on gfx950: its
// agent-scope release / acquire publishes write back and bypass the per-XCD
// L2 on every tile.)

constexpr int SL_T = 256, SL_K = 16, SL_TILE = SL_T * SL_K;       // 4096 positions per tile
size_t segs_lb_bytes(uint32_t max_n) { return ((size_t)max_n / SL_TILE + 2) * 16 + 64; }   // (sf_internal.h)

struct SegTile {                 // one thread's 16 positions
    uint32_t k[SL_K];
    uint32_t m[SL_K];            // the events' words (exit flag alone beyond n)
    uint32_t hmask, heads;
    long long acq;
};
template <bool PCG>
__device__ __forceinline__ void seg_load(SegTile& t, const uint32_t* keys, const SortedEv& ev, uint32_t p0, uint32_t n) {
    if (p0 + SL_K <= n) {
        const uint4* kp = (const uint4*)(keys + p0);
#pragma unroll
        for (int q = 0; q < SL_K / 4; q++) { const uint4 v = kp[q]; t.k[4 * q] = v.x; t.k[4 * q + 1] = v.y; t.k[4 * q + 2] = v.z; t.k[4 * q + 3] = v.w; }
        const uint4* mp = (const uint4*)(ev.meta + p0);
#pragma unroll
        for (int q = 0; q < SL_K / 4; q++) { const uint4 v = mp[q]; t.m[4 * q] = v.x; t.m[4 * q + 1] = v.y; t.m[4 * q + 2] = v.z; t.m[4 * q + 3] = v.w; }
    } else {
#pragma unroll
        for (int q = 0; q < SL_K; q++) {
            const bool in = p0 + q < n;
            t.k[q] = in ? keys[p0 + q] : 0u;
            t.m[q] = in ? ev.meta[p0 + q] : ((uint32_t)SF_EV_EXIT << 16) | (1u << 24);
        }
    }
    const uint32_t kprev = (p0 > 0 && p0 < n) ? keys[p0 - 1] : ~0u;
    t.hmask = 0; t.heads = 0; t.acq = 0;
#pragma unroll
    for (int q = 0; q < SL_K; q++) {
        const bool in = p0 + q < n;
        const bool h = in && (p0 + q == 0 || t.k[q] != (q ? t.k[q - 1] : kprev));
        t.hmask |= (h ? 1u : 0u) << q;
        t.heads += h;
        if (PCG) t.acq += (in && !(ev_flags(t.m[q]) & (SF_EV_EXIT | EVF_SYSBLK))) ? (long long)ev_count(ev, t.m[q], p0 + q) : 0;
    }
}
// block-wide exclusive scan of (heads, acq) over the threads; totals out
__device__ __forceinline__ void seg_block_scan(uint32_t& hx, long long& ax, uint32_t* htot, long long* atot) {
    __shared__ uint32_t w_heads[SL_T / 64];
    __shared__ long long w_acq[SL_T / 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t h0 = hx;
    const long long a0 = ax;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t h2 = __shfl_up(hx, d);
        const long long a2 = __shfl_up(ax, d);
        if (lane >= d) { hx += h2; ax += a2; }
    }
    if (lane == 63) { w_heads[wv] = hx; w_acq[wv] = ax; }
    __syncthreads();
    uint32_t hb = 0, ht = 0;
    long long ab = 0, at = 0;
#pragma unroll
    for (int w = 0; w < SL_T / 64; w++) {
        if (w < wv) { hb += w_heads[w]; ab += w_acq[w]; }
        ht += w_heads[w]; at += w_acq[w];
    }
    hx = hx - h0 + hb;
    ax = ax - a0 + ab;
    *htot = ht; *atot = at;
}

template <bool PCG>
__global__ void __launch_bounds__(SL_T) k_segs_red(const uint32_t* keys, SortedEv ev, uint32_t n, uint32_t* t_heads,
                                                   long long* t_acq) {
    SegTile t;
    seg_load<PCG>(t, keys, ev, blockIdx.x * SL_TILE + threadIdx.x * SL_K, n);
    uint32_t hx = t.heads, ht;
    long long ax = t.acq, at;
    seg_block_scan(hx, ax, &ht, &at);
    if (threadIdx.x == 0) { t_heads[blockIdx.x] = ht; t_acq[blockIdx.x] = at; }
}
// one workgroup: exclusive prefix of the tile totals, in place
__global__ void __launch_bounds__(1024) k_segs_tscan(uint32_t* t_heads, long long* t_acq, uint32_t tiles) {
    __shared__ uint32_t sh[1024];
    __shared__ long long sa[1024];
    const uint32_t per = (tiles + 1023) / 1024, i0 = threadIdx.x * per, i1 = min(i0 + per, tiles);
    uint32_t h = 0;
    long long a = 0;
    for (uint32_t i = i0; i < i1; i++) { h += t_heads[i]; a += t_acq[i]; }
    sh[threadIdx.x] = h; sa[threadIdx.x] = a;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const uint32_t h2 = threadIdx.x >= (unsigned)d ? sh[threadIdx.x - d] : 0u;
        const long long a2 = threadIdx.x >= (unsigned)d ? sa[threadIdx.x - d] : 0;
        __syncthreads();
        sh[threadIdx.x] += h2; sa[threadIdx.x] += a2;
        __syncthreads();
    }
    h = sh[threadIdx.x] - h; a = sa[threadIdx.x] - a;        // exclusive prefix of this thread's run
    for (uint32_t i = i0; i < i1; i++) {
        const uint32_t th = t_heads[i];
        const long long ta = t_acq[i];
        t_heads[i] = h; t_acq[i] = a;
        h += th; a += ta;
    }
}

template <bool PCG>
__global__ void __launch_bounds__(SL_T) k_segs_out(DevBatch b, SortedEv ev,
                                                   const uint8_t* s_atag, const uint32_t* keys, uint32_t* head_scan,
                                                   int64_t* pcg, uint32_t* seg_start, uint32_t* seg_res,
                                                   uint32_t* n_seg, uint32_t* segflag, int64_t* last_ts,
                                                   const int32_t* err, bool exit_marks, int32_t* prio_seen,
                                                   const uint32_t* t_heads, const long long* t_acq) {
    const uint32_t n = b.n, p0 = blockIdx.x * SL_TILE + threadIdx.x * SL_K;
    SegTile t;
    seg_load<PCG>(t, keys, ev, p0, n);
    uint32_t hx = t.heads, ht;
    long long ax = t.acq, at;
    seg_block_scan(hx, ax, &ht, &at);
    if (p0 >= n) return;
    uint32_t hs = t_heads[blockIdx.x] + hx;   // heads before this thread's first position
    long long run = PCG ? t_acq[blockIdx.x] + ax : 0;
    uint32_t hsv[SL_K];
    long long pv[SL_K];
    uint32_t acc = 0, prio = 0;
    int64_t cur = hs ? (int64_t)hs - 1 : -1;   // the segment of the position before this thread's first
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < SL_K; q++) {
        const uint32_t p = p0 + q;
        const bool in = p < n;
        if ((t.hmask >> q) & 1u) {
            if (acc && cur >= 0) atomicOr(&segflag[cur], acc);
            acc = 0;
            hs++;
            cur = (int64_t)hs - 1;
            seg_start[hs - 1] = p;
            seg_res[hs - 1] = t.k[q];
        }
        hsv[q] = hs;
        const uint8_t fq = ev_flags(t.m[q]);
        // (the count escape is a gather: only events that need the count take it)
        const int32_t cq = (in && !(fq & SF_EV_EXIT)) ? ev_count(ev, t.m[q], p) : 0;
        if (PCG) { run += (fq & EVF_SYSBLK) ? 0 : (long long)cq; pv[q] = run; }
        if (!in) continue;
        uint32_t mine = 0;
        if (exit_marks && (fq & SF_EV_EXIT)) mine |= SEGF_EXIT;
        if (!(fq & SF_EV_EXIT))
            mine |= ((fq & SF_EV_PRIO) ? SEGF_PRIO : 0u) | (cq <= 0 ? SEGF_NONPOS : 0u) |
                    ((fq & EVF_SYSBLK) ? SEGF_SYS : 0u);
        for (uint32_t a = 0; a < b.arg_slots; a++)
            if (s_atag[(size_t)a * n + p] == SF_TAG_COLLECTION) mine |= SEGF_COLL;
        acc |= mine;
        prio |= mine & SEGF_PRIO;
        if (p == n - 1) { *n_seg = hs; seg_start[hs] = n; }
        if (p == 0 && *err == 0) *last_ts = b.ts[n - 1];      // the sort's first pass has read the old value
    }
    if (acc && cur >= 0) atomicOr(&segflag[cur], acc);
    if (__ballot(prio != 0) && lane == 0) atomicOr(prio_seen, 1);
    if (p0 + SL_K <= n) {
        uint4* hp = (uint4*)(head_scan + p0);
#pragma unroll
        for (int q = 0; q < SL_K / 4; q++) hp[q] = make_uint4(hsv[4 * q], hsv[4 * q + 1], hsv[4 * q + 2], hsv[4 * q + 3]);
        if (PCG) {
            longlong2* pp = (longlong2*)(pcg + p0);
#pragma unroll
            for (int q = 0; q < SL_K / 2; q++) pp[q] = make_longlong2(pv[2 * q], pv[2 * q + 1]);
        }
    } else {
        for (int q = 0; q < SL_K; q++) {
            if (p0 + q >= n) break;
            head_scan[p0 + q] = hsv[q];
            if (PCG) pcg[p0 + q] = pv[q];
        }
    }
}

template <bool PCG>
static void launch_segs3(const DevState& st, Work& w, const DevBatch& b, hipStream_t s) {
    const uint32_t n = b.n, tiles = (n + SL_TILE - 1) / SL_TILE;
    uint32_t* th = (uint32_t*)w.segs_lb;
    long long* ta = (long long*)((char*)w.segs_lb + (((size_t)tiles * 4 + 15) & ~(size_t)15));
    const SortedEv ev = sorted_ev(w, b);
    hipLaunchKernelGGL(k_segs_red<PCG>, dim3(tiles), dim3(SL_T), 0, s, w.keys_out, ev, n, th, ta);
    hipLaunchKernelGGL(k_segs_tscan, dim3(1), dim3(1024), 0, s, th, ta, tiles);
    hipLaunchKernelGGL(k_segs_out<PCG>, dim3(tiles), dim3(SL_T), 0, s, b, ev, w.s_atag, w.keys_out,
                       w.head_scan, w.pcg, w.seg_start, w.seg_res, w.n_seg, w.segflag, st.last_ts, st.err,
                       st.n_prule != 0, st.prio_seen, th, ta);
}

// Append to a list with one atomic per wavefront (a single hot counter would
// otherwise serialise millions of atomics at one L2 channel).
__device__ uint32_t wave_append(uint32_t* counter, bool take) {
    const unsigned long long m = __ballot(take);
    if (!m) return 0;
    const int lane = (int)(threadIdx.x & 63);
    const int leader = __ffsll((long long)m) - 1;
    uint32_t base = 0;
    if (lane == leader) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = __shfl(base, leader);
    return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// Route each segment: light lane interpreter, heavy window algorithms, or the
// heavy generic interpreter (one lane of a wavefront).
__global__ void k_classify(DevState st, Work w, SortedEv ev) {
    ev_open(ev);
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = s < *w.n_seg;
    uint32_t lo = 0, hi = 0, res = 0;
    if (valid) { lo = w.seg_start[s]; hi = w.seg_start[s + 1]; res = w.seg_res[s]; }
    // an xflow group (sf_xflow.h) is decided by k_decide_x only; origins alone
    // do not route a segment there (their nodes: sf_origin.hip)
    const bool xs = valid && st.xmap && st.xmap[res] != XNONE;
    if (xs) w.seg_mode[s] = SM_XFLOW;
    {   // long xflow segments the wave walk can take (k_decide_xw)
        const bool xw = xs && xw_take(st, res, hi - lo);
        const uint32_t p = wave_append(&w.counters[WC_XW_LIST], xw);
        if (xw) w.xw_list[p] = s;
    }
    if (st.emb) {   // long segments of a resource whose only rule is a bound cluster rule (k_decide_xcl)
        const bool xc = xs && xcl_take(st, res, hi - lo);
        const uint32_t p = wave_append(&w.counters[WC_XCL_LIST], xc);
        if (xc) w.xcl_list[p] = s;
    }
    bool light = valid && !xs && hi - lo <= w.heavy_min;
    // a ParamFlow-only segment of more than 32 events is faster on the
    // wavefront-by-value path (SM_PARAM) than as one lane's serial table walk
    if (light && hi - lo > 32 && (st.rdesc[res].flags & RD_PRULE) &&
        heavy_mode(st, res, w.segflag[s], ev_time(ev, lo)) == SM_PARAM)
        light = false;
    // light list slot: workgroup histogram of the length classes in LDS, one
    // global atomic per class and workgroup
    // (hcnt / hbase [0, LCLS): generic lane walk, [LCLS, 2 LCLS): lean QPS walk)
    __shared__ uint32_t hcnt[2 * LCLS], hbase[2 * LCLS];
    if (threadIdx.x < 2 * LCLS) hcnt[threadIdx.x] = 0;
    __syncthreads();
    // a segment of a resource whose only check is one QPS DefaultController rule
    // runs the lean lane walk (decide_qps_segment: k_decide_short_qps / k_decide_light_qps)
    const bool lean = light && qps_lean(st, res, w.segflag[s]);
    const int lc = (light && hi - lo > SHORT_MAX) ? light_class(hi - lo) : -1;
    const int hk = lc + (lean ? LCLS : 0);
    const uint32_t lrank = lc >= 0 ? atomicAdd(&hcnt[hk], 1u) : 0u;
    __syncthreads();
    if (threadIdx.x < 2 * LCLS)
        hbase[threadIdx.x] = hcnt[threadIdx.x] ? atomicAdd(&w.lcounts[threadIdx.x], hcnt[threadIdx.x]) : 0u;
    __syncthreads();
    if (light) {
        w.seg_mode[s] = lean ? SM_LIGHTQ : SM_LIGHT;
        if (lc >= 0) {
            if (lean) w.light_list[w.loff[lc] + w.lcap[lc] - 1 - (hbase[hk] + lrank)] = s;
            else w.light_list[w.loff[lc] + hbase[hk] + lrank] = s;
        }
    }
    // short segments (<= SHORT_MAX events) listed densely for k_decide_short /
    // k_decide_short_qps, in segment (resource) order within each workgroup,
    // one global atomic per workgroup and list: a deciding wavefront's lanes
    // hold neighbouring resource rows and no idle lanes for the segments of
    // the other kernel.  Class 0's light_list region (every segment fits)
    // holds both lists: generic from the front, lean QPS from the back.
    static_assert(SHORT_MAX >= 1, "class 0 (one-event segments) must be a short class");
    __shared__ uint32_t wsh[2][32], bsh[2];
    const bool shrt = light && hi - lo <= SHORT_MAX;
    const unsigned long long mg = __ballot(shrt && !lean), mq = __ballot(shrt && lean);
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6), nwv = (int)(blockDim.x >> 6);
    if (lane == 0) { wsh[0][wv] = (uint32_t)__popcll(mg); wsh[1][wv] = (uint32_t)__popcll(mq); }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t acc = 0;
        for (int k = 0; k < nwv; k++) { const uint32_t c = wsh[threadIdx.x][k]; wsh[threadIdx.x][k] = acc; acc += c; }
        bsh[threadIdx.x] = acc ? atomicAdd(&w.counters[WC_SHORT + threadIdx.x], acc) : 0u;
    }
    __syncthreads();
    if (shrt) {
        const unsigned long long below = (1ull << lane) - 1ull;
        if (lean) w.light_list[w.loff[0] + w.lcap[0] - 1 - (bsh[1] + wsh[1][wv] + (uint32_t)__popcll(mq & below))] = s;
        else w.light_list[w.loff[0] + bsh[0] + wsh[0][wv] + (uint32_t)__popcll(mg & below)] = s;
    }
    const bool heavy = valid && !light && !xs;
    if (!__ballot(heavy)) return;
    uint8_t mode = SM_GENERIC;
    if (heavy) {
        const int64_t tlo = ev_time(ev, lo);
        mode = heavy_mode(st, res, w.segflag[s], tlo);
        if (mode != SM_GENERIC) {
            const int64_t thi = ev_time(ev, hi - 1);
            const int64_t h0 = tlo / st.wl, h1 = thi / st.wl;
            const int64_t s0 = tlo / 1000, s1 = thi / 1000;
            const int64_t nh = h1 - h0 + 1, ns = s1 - s0 + 1;
            if (nh > 65536 || ns > 65536) mode = SM_GENERIC;
            else {
                uint32_t bh = atomicAdd(&w.counters[WC_ACC_HW], (uint32_t)nh);
                uint32_t bs = atomicAdd(&w.counters[WC_ACC_SEC], (uint32_t)ns);
                if ((uint64_t)bh + nh > w.acc_cap || (uint64_t)bs + ns > w.acc_cap) mode = SM_GENERIC;
                else {
                    w.acc_hw_base[s] = bh; w.acc_sec_base[s] = bs;
                    w.seg_hw0[s] = h0; w.seg_sec0[s] = s0; w.seg_nhw[s] = (uint32_t)nh; w.seg_nsec[s] = (uint32_t)ns;
                    Acc z{}; z.min_rt = INT64_MAX;
                    Acc* ah = (Acc*)w.acc_hw; Acc* as = (Acc*)w.acc_sec;
                    for (int64_t k = 0; k < nh; k++) ah[bh + k] = z;
                    for (int64_t k = 0; k < ns; k++) as[bs + k] = z;
                }
            }
        }
        w.seg_mode[s] = mode;
    }
    // THREAD-grade and RateLimiter segments go to k_heavy_stream, the rest to
    // k_heavy_decide.  Long-running segments first in each list, so that they
    // start first: [0, front) and [seg_cap - back, seg_cap)
    const bool strm = heavy && (mode == SM_THREAD || mode == SM_RL);
    const bool big = hi - lo > 65536u;
    const bool slow = heavy && !strm && (mode == SM_GENERIC || big);
    const uint32_t fpos = wave_append(&w.counters[WC_HEAVY_FRONT], slow);
    const uint32_t bpos = wave_append(&w.counters[WC_HEAVY_BACK], heavy && !strm && !slow);
    if (slow) w.heavy_list[fpos] = s;
    else if (heavy && !strm) w.heavy_list[w.seg_cap - 1 - bpos] = s;
    const uint32_t sfp = wave_append(&w.counters[WC_STREAM_FRONT], strm && big);
    const uint32_t sbp = wave_append(&w.counters[WC_STREAM_BACK], strm && !big);
    if (strm && big) w.stream_list[sfp] = s;
    else if (strm) w.stream_list[w.seg_cap - 1 - sbp] = s;
}

// Tiles of FILL_TILE events over the heavy segments of each class (block c:
// class c): cls 0 = k_heavy_decide's list (QPS / WarmUp / no rule; generic
// segments wrote their verdicts themselves), cls 1 = k_heavy_stream's list
// (THREAD / RL).  k_heavy_fill then reads only the events of its class.
__global__ void __launch_bounds__(1024) k_fill_tiles(HeavyCtx hc, StreamCtx sc, uint2* tiles, uint32_t cap,
                                                     uint32_t* ntiles) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry;
    const int c = (int)blockIdx.x;
    uint2* out = tiles + (size_t)c * cap;
    const uint32_t nl = c == 0 ? hc.n_heavy[0] + hc.n_heavy[WC_HEAVY_BACK - WC_HEAVY_FRONT]
                               : sc.n_list[0] + sc.n_list[WC_STREAM_BACK - WC_STREAM_FRONT];
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < nl; b0 += 1024) {
        const uint32_t i = b0 + threadIdx.x;
        uint32_t s = 0, nt = 0;
        if (i < nl) {
            const bool ok = c == 0 ? heavy_at(hc, i, &s) : stream_at(sc, i, &s);
            if (ok && hc.seg_mode[s] >= SM_QPS)                 // aligned FILL_TILE blocks the segment overlaps
                nt = (hc.seg_start[s + 1] - 1) / FILL_TILE - hc.seg_start[s] / FILL_TILE + 1;
        }
        const uint32_t incl = (uint32_t)wave_scan_add((int)nt);
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        uint32_t before = carry;
        for (int k = 0; k < wv; k++) before += wsum[k];
        const uint32_t base = before + incl - nt;
        const uint32_t g0 = nt ? hc.seg_start[s] / FILL_TILE : 0;
        for (uint32_t k = 0; k < nt && base + k < cap; k++) out[base + k] = make_uint2(s, g0 + k);
        __syncthreads();
        if (threadIdx.x == 1023) carry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) ntiles[c] = min(carry, cap);
}

// Segment routing (k_classify) and the heavy fill tiles: the end of the sort
// phase when the origin index passes follow (they read the routes), else the
// head of the decide phase on stream A (the sort phase is the longer of the two)
void launch_classify(const DevState& st, Work& w, const DevBatch& b, hipStream_t s, hipEvent_t* ev, bool timing) {
    const uint32_t n = b.n;
    FillSet f;
    f.add(w.counters, WC_COUNT * sizeof(uint32_t), 0);
    f.add(w.lcounts, 2 * LCLS * sizeof(uint32_t), 0);
    f.add(w.passbits, ((size_t)n / 64 + 2) * 8, 0);
    if (st.n_stream_rules) f.add(w.lxfar, ((size_t)n / 64 + 2) * 8, 0);
    launch_fill(f, s);
    const uint32_t max_seg = n < st.R ? n : st.R;
    if (timing) hipEventRecord(ev[EV_CLASSIFY_START], s);
    hipLaunchKernelGGL(k_classify, dim3(blocks(max_seg, 1024)), dim3(1024), 0, s, st, w, sorted_ev(w, b));
    HeavyCtx hc = heavy_ctx(w);
    StreamCtx sc{w.stream_list, w.counters + WC_STREAM_FRONT, w.seg_cap, nullptr, w.counters + WC_STREAM_NEXT};
    hipLaunchKernelGGL(k_fill_tiles, dim3(2), dim3(1024), 0, s, hc, sc, w.fill_tiles, w.fill_tile_cap, w.fill_ntiles);
    if (timing) hipEventRecord(ev[EV_CLASSIFIED], s);
}

// scratch of the radix sort (the segment table's is Work::segs_lb, segs_lb_bytes)
hipError_t query_temp_bytes(uint32_t max_n, size_t* sort_bytes) {
    (void)max_n;
    *sort_bytes = rs_scratch_bytes();
    return hipSuccess;
}

// The sort phase of a batch, all on stream s (see the file header).
hipError_t launch_sort(const DevState& st, Work& w, const DevBatch& b, uint32_t shard_count, uint32_t shard_index,
                       uint32_t key_bits, hipStream_t s, hipEvent_t* ev, bool timing, bool classify) {
    const uint32_t n = b.n;
    if (n == 0) return hipSuccess;
    if (timing) hipEventRecord(ev[EV_SORT_START], s);
    hipError_t e;
    const bool org = b.origin != nullptr;                       // the origin rides in a 12-B payload
    // the chunked LSD sort (sf_rsort.h): middle passes in (keys_in, pv_in) and
    // (head_scan, pv_out); the last pass writes keys_out, perm, s_meta and the arguments
    const RsBatchSrc src{b, shard_count, shard_index, st.R, st.err, st.last_ts, st.xmap};
    if (org) {
        const RsSinkFinal<PackedEvO> fin{b, w.keys_out, w.perm, w.s_meta, w.s_origin, w.s_nargs, w.s_atag, w.s_abits};
        e = rs_sort(src, n, key_bits, w.keys_in, (PackedEvO*)w.pv_in, w.head_scan, (PackedEvO*)w.pv_out, fin,
                    w.sort_tmp, s);
    } else {
        const RsSinkFinal<PackedEv> fin{b, w.keys_out, w.perm, w.s_meta, nullptr, w.s_nargs, w.s_atag, w.s_abits};
        e = rs_sort(src, n, key_bits, w.keys_in, w.pv_in, w.head_scan, w.pv_out, fin, w.sort_tmp, s);
    }
    if (e != hipSuccess) return e;
    hipMemsetAsync(w.segflag, 0, (size_t)(n < st.R ? n : st.R) * 4, s);
    if (timing) hipEventRecord(ev[EV_SORTED], s);
    // segment table, head scan and (window rules loaded) the acquireCount prefix: reduce, scan, rescan
    if (st.n_window_rules) launch_segs3<true>(st, w, b, s);
    else launch_segs3<false>(st, w, b, s);
    if (classify) launch_classify(st, w, b, s, ev, timing);
    return hipGetLastError();
}

}  // namespace sf
