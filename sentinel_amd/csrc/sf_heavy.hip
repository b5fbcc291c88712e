// sf_heavy.hip — the heavy segment classes of the decide phase (sf_decide.hip;
// algorithms in sf_heavy.h and sf_stream.h).  Product code.
//   k_heavy_decide   one wavefront per heavy QPS / WarmUp / ParamFlow / generic segment (stream B)
//   k_heavy_stream   persistent, one workgroup per THREAD / RateLimiter segment (stream A; sf_stream.h,
//                    which only this file includes: it defines the kernel)
//   k_thr_*          the state-independent THREAD run tables ahead of it (launch_thr_prep)
//   k_heavy_fill     verdicts + per-window counter deltas of one class from the pass bits
//   k_heavy_apply    the deltas applied to the LeapArray state in time order
#include "sf_stream.h"

namespace sf {

HeavyCtx heavy_ctx(const Work& w) {
    HeavyCtx hc;
    hc.seg_start = w.seg_start; hc.seg_res = w.seg_res; hc.seg_mode = w.seg_mode;
    hc.heavy_list = w.heavy_list; hc.n_heavy = w.counters + WC_HEAVY_FRONT; hc.pcg = w.pcg; hc.seg_cap = w.seg_cap;
    hc.acc_hw = (Acc*)w.acc_hw; hc.acc_sec = (Acc*)w.acc_sec;
    hc.acc_hw_base = w.acc_hw_base; hc.acc_sec_base = w.acc_sec_base;
    hc.seg_hw0 = w.seg_hw0; hc.seg_sec0 = w.seg_sec0;
    hc.hticks = nullptr;
    hc.passbits = w.passbits;
    hc.exit_of = w.exit_of;
    hc.lxfar = w.lxfar;
    hc.thr_rec = w.thr_rec;
    hc.rid = w.keys_in; hc.run_start = w.head_scan; hc.run_pre = w.keys_out; hc.rrec = (uint2*)w.pv_in;
    hc.seg_rb = w.seg_rb; hc.seg_re = w.seg_re; hc.segflag = w.segflag;
    return hc;
}

// SM_PARAM: a ParamFlow-only resource whose rules are QPS-grade on one
// argument index (heavy_mode).  ParamFlowChecker's state is per (rule, value)
// (ParameterMetric token / time maps) and the node counters are only summed,
// so events of different values are independent: the wavefront takes 64
// events at a time, and the first lane of each distinct value in the 64 runs
// that value's events in order, rule by rule, with the (rule, value) state in
// registers (param_run_rule: one table find and one write per rule, however
// often the value recurs -- a Zipf head value recurs in most groups).  The
// finds of a rule all complete before any of its inserts (the wavefront runs
// them in lock-step; distinct values never share a key).  Verdict inputs go to
// the pass bits, v_wait (throttled passes) and v_rule (the blocking rule);
// k_heavy_fill and k_heavy_apply then do the StatisticSlot accounting as for
// the other window modes.
__device__ void heavy_param(const DevState& st, const SegIO& io, const HeavyCtx& hc, uint32_t res, uint32_t lo,
                            uint32_t hi) {
    __shared__ int64_t s_now[64], s_wait[64];
    __shared__ int32_t s_c[64];
    __shared__ uint8_t s_rule[64], s_ok[64];
    const int lane = (int)(threadIdx.x & 63);
    const uint32_t p0 = st.prule_off[res], np = st.prule_off[res + 1] - p0;
    const int32_t pidx = st.prules[p0].param_idx;
    const uint8_t pm_init = (uint8_t)(st.pm_init[res] | (1u << pidx));   // initParamMetricsFor on the first entry
    ParamTable pt{st.ptab, st.pcap_mask, st.err, st.pins};
    for (uint32_t q = lo; q < hi; q += 64) {
        const uint32_t j = q + (uint32_t)lane;
        const bool valid = j < hi;
        const uint32_t jc = valid ? j : hi - 1;
        const uint32_t mw = ev_word(io, jc);
        const int64_t now = ev_time(io, mw, jc);
        const int32_t c = ev_count(io, mw, jc);
        const uint32_t na = io.arg_slots ? (io.nargs ? io.nargs[jc] : io.arg_slots) : 0;
        uint32_t tag = SF_TAG_NULL; uint64_t bits = 0;
        if ((int32_t)na > pidx) { tag = io.atag[(size_t)pidx * io.n + jc]; bits = io.abits[(size_t)pidx * io.n + jc]; }
        const bool sysb = valid && (ev_flags(mw) & EVF_SYSBLK);   // blocked before ParamFlowSlot
        const bool key = valid && !sysb && tag != SF_TAG_NULL;  // a null value skips every rule (passCheck :53-60)
        s_now[lane] = now; s_c[lane] = c; s_wait[lane] = 0; s_rule[lane] = 0; s_ok[lane] = 0;
        // the lanes of each distinct value: `mine` on the value's first lane
        unsigned long long pend = __ballot(key), mine = 0;
        while (pend) {
            const int l = __ffsll((long long)pend) - 1;
            const uint32_t kt = (uint32_t)__builtin_amdgcn_readlane((int)tag, l);
            const uint64_t kb = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(bits >> 32), l) << 32) |
                                (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)bits, l);
            const unsigned long long same = __ballot(key && tag == kt && bits == kb);
            if (lane == l) mine = same;
            pend &= ~same;
        }
        __syncthreads();
        if (mine) {
            uint64_t live = mine;
            for (uint32_t k = 0; k < np && live; k++) {
                const uint64_t before = live;
                live = param_run_rule(pt, res, (int)k, st.prules[p0 + k], st.items, tag, bits, live,
                                      [&](int o) { return s_now[o]; }, [&](int o) { return s_c[o]; },
                                      [&](int o, int64_t w) { s_wait[o] += w; });
                for (uint64_t m = before & ~live; m; m &= m - 1) s_rule[__builtin_ctzll(m)] = (uint8_t)k;
            }
            for (uint64_t m = live; m; m &= m - 1) s_ok[__builtin_ctzll(m)] = 1;
            // ParamFlowStatisticEntryCallback: the value's thread count, once for all its passes
            if (live && ((pm_init >> pidx) & 1)) pm_thread_add(pt, res, pidx, tag, bits, __popcll(live));
        }
        __syncthreads();
        const bool blocked = sysb || (key && !s_ok[lane]);
        const unsigned long long pm = __ballot(valid && !blocked);
        if (lane == 0 && pm) {
            const uint32_t sh = q & 63;
            atomicOr(hc.passbits + (q >> 6), pm << sh);
            if (sh) atomicOr(hc.passbits + (q >> 6) + 1, pm >> (64 - sh));
        }
        // (s_wait is 0 on a lane without a key; a blocked entry keeps what the rules that passed it made it wait)
        if (valid) { io.v_wait[j] = (int32_t)s_wait[lane]; io.v_rule[j] = blocked && key ? s_rule[lane] : 0; }
    }
    if (lane == 0) st.pm_init[res] = pm_init;
}

// One wavefront per heavy QPS / WarmUp / no-rule / generic segment (64-thread
// workgroups: the team needs no barriers).  THREAD and RateLimiter segments
// run in k_heavy_stream (sf_stream.h).
template <int MAXS>
__global__ void __launch_bounds__(64) k_heavy_decide(DevState st, SegIO io, HeavyCtx hc) {
    ev_open(io.ev);
    // grid-stride over the list (medium ParamFlow segments can outnumber the
    // grid sized for segments above heavy_min); long segments are listed first
    uint32_t s;
    for (uint32_t b = blockIdx.x; heavy_at(hc, b, &s); b += gridDim.x) {
        const uint32_t lo = hc.seg_start[s], hi = hc.seg_start[s + 1], res = hc.seg_res[s];
        Team tm{(int)threadIdx.x};
        const uint64_t t_start = hc.hticks ? wall_clock64() : 0;
        switch (hc.seg_mode[s]) {
        case SM_QPS: heavy_qps<MAXS>(tm, st, io, hc, s, res, lo, hi, false); break;
        case SM_WARM: heavy_qps<MAXS>(tm, st, io, hc, s, res, lo, hi, true); break;
        case SM_NORULE: break;                      // every entry passes (k_heavy_fill)
        case SM_PARAM: heavy_param(st, io, hc, res, lo, hi); break;
        default:
            if (tm.leader()) decide_segment<MAXS>(st, io, res, lo, hi);
            break;
        }
        if (hc.hticks && tm.leader() && b < gridDim.x) hc.hticks[b] = wall_clock64() - t_start;
    }
}

struct PAcc {            // per-thread partial of one accumulator slot
    unsigned long long pass, block, succ, rt, exc, n_pass, n_exit, n_touch;
    long long min_rt;
    __device__ void clear() { pass = block = succ = rt = exc = n_pass = n_exit = n_touch = 0; min_rt = INT64_MAX; }
    __device__ void add(const EvContrib& e) {
        n_touch++;
        if (e.live_exit) {
            succ += (unsigned long long)e.c; rt += (unsigned long long)e.rt; n_exit++;
            if (e.err) exc += (unsigned long long)e.c;
            if (e.rt < min_rt) min_rt = e.rt;
        } else if (e.passed) { pass += (unsigned long long)e.c; n_pass++; }
        else block += (unsigned long long)e.c;
    }
    __device__ void merge(const PAcc& o) {
        pass += o.pass; block += o.block; succ += o.succ; rt += o.rt; exc += o.exc;
        n_pass += o.n_pass; n_exit += o.n_exit; n_touch += o.n_touch;
        if (o.min_rt < min_rt) min_rt = o.min_rt;
    }
    __device__ void flush(Acc* table, uint32_t key) const {
        if (!n_touch) return;
        Acc* a = table + key;
        atomicAdd(&a->pass, pass); atomicAdd(&a->block, block); atomicAdd(&a->succ, succ);
        atomicAdd(&a->rt, rt); atomicAdd(&a->exc, exc); atomicAdd(&a->n_pass, n_pass);
        atomicAdd(&a->n_exit, n_exit); atomicAdd(&a->n_touch, n_touch);
        if (min_rt != INT64_MAX) atomicMin(&a->min_rt, min_rt);
    }
};

__device__ long long wave_min(long long v) {
    for (int o = 32; o > 0; o >>= 1) { long long u = __shfl_xor(v, o); v = u < v ? u : v; }
    return v;
}
// flush at wave level: one set of atomics per wave when all active lanes share a key
__device__ void wave_flush(PAcc& p, uint32_t key, Acc* table) {
    const uint32_t NONE = 0xffffffffu;
    bool act = key != NONE && p.n_touch;
    unsigned long long m = __ballot(act);
    if (!m) return;
    int l0 = __ffsll((long long)m) - 1;
    uint32_t k0 = __shfl(key, l0);
    bool differ = __ballot(act && key != k0) != 0;
    if (differ) { if (act) p.flush(table, key); return; }
    if (!act) p.clear();
    PAcc r;
    r.pass = wave_sum(p.pass); r.block = wave_sum(p.block); r.succ = wave_sum(p.succ); r.rt = wave_sum(p.rt);
    r.exc = wave_sum(p.exc); r.n_pass = wave_sum(p.n_pass); r.n_exit = wave_sum(p.n_exit);
    r.n_touch = wave_sum(p.n_touch); r.min_rt = wave_min(p.min_rt);
    if ((int)(threadIdx.x & 63) == l0) r.flush(table, k0);
}

// workgroup flush: the waves' partials of one key are merged in LDS first,
// so a hot window row takes one set of atomics per workgroup
struct PAccSlot { PAcc p; uint32_t key; };
__device__ void block_flush(PAcc& p, uint32_t key, Acc* table, PAccSlot* lds) {
    const uint32_t NONE = 0xffffffffu;
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6), nw = (int)(blockDim.x >> 6);
    bool act = key != NONE && p.n_touch;
    const unsigned long long m = __ballot(act);
    uint32_t k0 = NONE;
    bool uni = false;
    if (m) {
        const int l0 = __ffsll((long long)m) - 1;
        k0 = __shfl(key, l0);
        uni = __ballot(act && key != k0) == 0;
    }
    if (m && !uni) { if (act) p.flush(table, key); }      // mixed keys: lane atomics
    PAcc r; r.clear();
    if (m && uni) {
        if (!act) p.clear();
        r.pass = wave_sum(p.pass); r.block = wave_sum(p.block); r.succ = wave_sum(p.succ); r.rt = wave_sum(p.rt);
        r.exc = wave_sum(p.exc); r.n_pass = wave_sum(p.n_pass); r.n_exit = wave_sum(p.n_exit);
        r.n_touch = wave_sum(p.n_touch); r.min_rt = wave_min(p.min_rt);
    }
    if (lane == 0) { lds[wv].p = r; lds[wv].key = (m && uni) ? k0 : NONE; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int a = 0; a < nw; a++) {
            if (lds[a].key == NONE) continue;
            PAcc acc = lds[a].p;
            for (int b = a + 1; b < nw; b++) {
                if (lds[b].key != lds[a].key) continue;
                const PAcc& o = lds[b].p;
                acc.pass += o.pass; acc.block += o.block; acc.succ += o.succ; acc.rt += o.rt; acc.exc += o.exc;
                acc.n_pass += o.n_pass; acc.n_exit += o.n_exit; acc.n_touch += o.n_touch;
                if (o.min_rt < acc.min_rt) acc.min_rt = o.min_rt;
                lds[b].key = NONE;
            }
            acc.flush(table, lds[a].key);
        }
    }
    __syncthreads();
}

// THREAD-grade stream segments, state-independent preparation (at the head of
// the decide phase, launch_thr_prep), grid-stride over the stream class's fill
// tiles.  A run is a maximal stretch of a segment's checked entries, or of its
// other events (sf_stream.h run mode).
//   k_thr_heads  run heads of each tile; the segment flag of an acquireCount
//                beyond THR_CBIG
__global__ void __launch_bounds__(256) k_thr_heads(SortedEv ev, HeavyCtx hc,
                                                   const uint2* tiles, const uint32_t* ntiles, uint32_t* tile_rc,
                                                   uint32_t* segflag) {
    __shared__ uint32_t heads;
    const uint32_t nt = ntiles[1];
    for (uint32_t t = blockIdx.x; t < nt; t += gridDim.x) {
        const uint2 tl = tiles[t];
        const uint32_t s = tl.x;
        if (hc.seg_mode[s] != SM_THREAD) { if (threadIdx.x == 0) tile_rc[t] = 0; continue; }
        if (threadIdx.x == 0) heads = 0;
        __syncthreads();
        const uint32_t lo = hc.seg_start[s], hi = hc.seg_start[s + 1];
        uint32_t nh = 0;
        bool big = false;
        for (uint32_t j = max(tl.y * FILL_TILE, lo) + threadIdx.x; j < min(tl.y * FILL_TILE + FILL_TILE, hi); j += 256) {
            const uint32_t m = ev.meta[j];
            const bool ent = is_checked_entry(ev_flags(m));
            if (ent) big |= ev_count(ev, m, j) > THR_CBIG;
            nh += (j == lo || ent != is_checked_entry(ev_flags(ev, j - 1))) ? 1u : 0u;
        }
        if (__ballot(big) && (threadIdx.x & 63) == 0) atomicOr(&segflag[s], SEGF_BIGC);
        nh = (uint32_t)wave_sum(nh);
        if ((threadIdx.x & 63) == 0 && nh) atomicAdd(&heads, nh);
        __syncthreads();
        if (threadIdx.x == 0) tile_rc[t] = heads;
        __syncthreads();
    }
}

//   k_thr_rscan  exclusive scan of the tiles' run counts (global run ids:
//                the runs of a segment are a contiguous range, in order)
//   k_thr_rid    run id of every event, run starts, the segment's run range
//   k_thr_rec    the event records the stream kernel reads: run-mode segments
//                (thr_run_mode) entry records (run id of the exit,
//                acquireCount), exits live from before the batch counted per
//                run; the others one 8-B window-walk record per event
__global__ void __launch_bounds__(1024) k_thr_rscan(uint32_t* tile_rc, const uint32_t* ntiles) {
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry;
    const uint32_t nt = ntiles[1];
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < nt; b0 += 1024) {
        const uint32_t i = b0 + threadIdx.x;
        const uint32_t v = i < nt ? tile_rc[i] : 0u;
        const uint32_t incl = (uint32_t)wave_scan_add((int)v);
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        uint32_t before = carry;
        for (int k = 0; k < wv; k++) before += wsum[k];
        if (i < nt) tile_rc[i] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023) carry = before + incl;
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_thr_rid(SortedEv ev, HeavyCtx hc, const uint2* tiles,
                                                 const uint32_t* ntiles, const uint32_t* tile_rb) {
    __shared__ uint32_t wsum[4];
    constexpr uint32_t PER = FILL_TILE / 256;
    const uint32_t nt = ntiles[1];
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    for (uint32_t t = blockIdx.x; t < nt; t += gridDim.x) {
        const uint2 tl = tiles[t];
        const uint32_t s = tl.x;
        if (hc.seg_mode[s] != SM_THREAD) continue;
        const uint32_t lo = hc.seg_start[s], hi = hc.seg_start[s + 1];
        const uint32_t base = tl.y * FILL_TILE + PER * threadIdx.x;
        uint32_t hm = 0;                                   // heads among this thread's PER events
#pragma unroll
        for (uint32_t k = 0; k < PER; k++) {
            const uint32_t j = base + k;
            if (j >= lo && j < hi && (j == lo || is_checked_entry(ev_flags(ev, j)) != is_checked_entry(ev_flags(ev, j - 1))))
                hm |= 1u << k;
        }
        const uint32_t c = (uint32_t)__popc(hm);
        const uint32_t incl = (uint32_t)wave_scan_add((int)c);
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        uint32_t run = tile_rb[t] + incl - c;              // heads before this thread's events in the tile
        for (int k = 0; k < wv; k++) run += wsum[k];
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < PER; k++) {
            const uint32_t j = base + k;
            if (j < lo || j >= hi) continue;
            if ((hm >> k) & 1u) { run++; hc.run_start[run - 1] = j; hc.run_pre[run - 1] = 0u; }
            hc.rid[j] = run - 1;                           // (a tile's events before its first head: the last run before it)
            if (j == lo) hc.seg_rb[s] = run - 1;
            if (j == hi - 1) hc.seg_re[s] = run;
        }
    }
}

__global__ void __launch_bounds__(256) k_thr_rec(SortedEv ev, const int64_t* eref,
                                                 HeavyCtx hc, const uint2* tiles, const uint32_t* ntiles,
                                                 const uint32_t* segflag) {
    const uint32_t nt = ntiles[1];
    for (uint32_t t = blockIdx.x; t < nt; t += gridDim.x) {
        const uint2 tl = tiles[t];
        const uint32_t s = tl.x;
        if (hc.seg_mode[s] != SM_THREAD) continue;
        const uint32_t lo = hc.seg_start[s], hi = hc.seg_start[s + 1];
        const bool runs = thr_run_mode(hc, s, lo, hi, segflag[s]);
        for (uint32_t j = max(tl.y * FILL_TILE, lo) + threadIdx.x; j < min(tl.y * FILL_TILE + FILL_TILE, hi); j += 256) {
            const uint32_t m = ev.meta[j];
            const uint8_t f = ev_flags(m);
            if (runs) {
                if (is_checked_entry(f)) {
                    const uint32_t x = hc.exit_of[j];
                    hc.rrec[j] = make_uint2(x < hi ? hc.rid[x] : XO_NONE, (uint32_t)ev_count(ev, m, j));
                } else if ((f & SF_EV_EXIT) && (eref ? eref[j] : -1) == -1) {
                    atomicAdd(&hc.run_pre[hc.rid[j]], 1u);      // its entry passed before this batch: live
                }
                continue;
            }
            uint2 r;
            if (is_checked_entry(f)) { r.x = hc.exit_of[j]; r.y = (uint32_t)ev_count(ev, m, j); }
            else if (!(f & SF_EV_EXIT)) { r.x = 0u; r.y = THR_REC_EXIT; }   // blocked before: a no-op (dead exit)
            else {
                const int64_t ref = eref ? eref[j] : -1;
                r.x = ref >= 0 ? j - (uint32_t)ref : 0u;
                r.y = THR_REC_EXIT | (ref == -1 ? THR_REC_LIVE : 0u);
            }
            ((uint2*)hc.thr_rec)[j] = r;
        }
    }
}

// Verdicts and per-window counter deltas of the heavy segments of one class.
// A tile is one segment's part of an aligned FILL_TILE-event block of the
// sorted batch; lane t owns the aligned group of 16 events at block + 16 t, so
// every array is read and written with 16-byte vector accesses (groups cut by
// a segment edge fall back to per-event accesses) and all of a lane's loads
// are in flight together.  Each event is one pass-bit lookup (its entry's bit
// for an exit).  Persistent grid, each workgroup a contiguous run of tiles; a
// thread's partial sums carry across the run while the window row repeats.
// Window rows of a run of tiles accumulated in LDS: ACC_K consecutive
// accumulator slots from `base`, 64-bit LDS atomics; flushed to the global
// rows (one set of atomics per touched slot) only when a tile's window range
// leaves the table or the workgroup's run ends, so the rows of a hot
// resource take one flush per window, not one per thread or tile.
constexpr int ACC_K = 32;
struct LdsAcc {
    unsigned long long v[8][ACC_K];                 // pass, block, succ, rt, exc, n_pass, n_exit, n_touch
    long long min_rt[ACC_K];
};
__device__ __forceinline__ void lds_acc_clear(LdsAcc& A) {
    for (int i = threadIdx.x; i < 8 * ACC_K; i += blockDim.x) A.v[i / ACC_K][i % ACC_K] = 0ull;
    for (int i = threadIdx.x; i < ACC_K; i += blockDim.x) A.min_rt[i] = INT64_MAX;
}
__device__ __forceinline__ void lds_acc_add(LdsAcc& A, uint32_t k, const PAcc& p) {
    if (!p.n_touch) return;
    if (p.pass) atomicAdd(&A.v[0][k], p.pass);
    if (p.block) atomicAdd(&A.v[1][k], p.block);
    if (p.succ) atomicAdd(&A.v[2][k], p.succ);
    if (p.rt) atomicAdd(&A.v[3][k], p.rt);
    if (p.exc) atomicAdd(&A.v[4][k], p.exc);
    if (p.n_pass) atomicAdd(&A.v[5][k], p.n_pass);
    if (p.n_exit) atomicAdd(&A.v[6][k], p.n_exit);
    atomicAdd(&A.v[7][k], p.n_touch);
    if (p.min_rt != INT64_MAX) atomicMin(&A.min_rt[k], p.min_rt);
}
// flush slots to table[base + k] (thread k), then clear; callers bracket with barriers
__device__ __forceinline__ void lds_acc_flush(LdsAcc& A, Acc* table, uint32_t base) {
    const int k = (int)threadIdx.x;
    if (k < ACC_K && A.v[7][k]) {
        PAcc p;
        p.pass = A.v[0][k]; p.block = A.v[1][k]; p.succ = A.v[2][k]; p.rt = A.v[3][k]; p.exc = A.v[4][k];
        p.n_pass = A.v[5][k]; p.n_exit = A.v[6][k]; p.n_touch = A.v[7][k]; p.min_rt = A.min_rt[k];
        p.flush(table, base + (uint32_t)k);
    }
}

constexpr int FG = (int)FILL_TILE / 256;         // events per lane
struct FillGrp { uint32_t m[FG]; uint8_t f[FG]; int32_t c[FG]; int64_t t[FG]; };

// vector copy of an aligned group: 16-byte accesses (8-byte for an 8-byte group)
__device__ __forceinline__ void load16(void* dst, const void* src, int bytes) {
    if (bytes == 8) { *(uint2*)dst = *(const uint2*)src; return; }
    uint4* d = (uint4*)dst; const uint4* q = (const uint4*)src;
#pragma unroll
    for (int k = 0; k < bytes / 16; k++) d[k] = q[k];
}
__device__ __forceinline__ void store16(void* dst, const void* src, int bytes) {
    if (bytes == 8) { *(uint2*)dst = *(const uint2*)src; return; }
    uint4* d = (uint4*)dst; const uint4* q = (const uint4*)src;
#pragma unroll
    for (int k = 0; k < bytes / 16; k++) d[k] = q[k];
}

#ifndef SF_FILL_MINB
#define SF_FILL_MINB 1
#endif
__global__ void __launch_bounds__(256, SF_FILL_MINB) k_heavy_fill(DevState st, SegIO io, HeavyCtx hc, const uint2* tiles,
                                                    const uint32_t* ntiles, int cls) {
    ev_open(io.ev);
    __shared__ LdsAcc acc_h, acc_s;
    const uint32_t NONE = 0xffffffffu;
    const uint32_t nt = ntiles[cls];
    const uint32_t wl = (uint32_t)st.wl;
    const uint32_t tb = (uint32_t)((uint64_t)nt * blockIdx.x / gridDim.x);
    const uint32_t te = (uint32_t)((uint64_t)nt * (blockIdx.x + 1) / gridDim.x);
    lds_acc_clear(acc_h); lds_acc_clear(acc_s);
    uint32_t bh_k = NONE, bs_k = NONE;                // LDS table bases (workgroup-uniform)
    __syncthreads();
    for (uint32_t t = tb; t < te; t++) {
        const uint2 tl = tiles[t];
        const uint32_t s = tl.x;
        const uint32_t lo = hc.seg_start[s], hi = hc.seg_start[s + 1];
        const uint8_t mode = hc.seg_mode[s];
        const bool all = mode == SM_NORULE, rl = mode == SM_RL, prm = mode == SM_PARAM;
        const uint32_t hwb = hc.acc_hw_base[s], secb = hc.acc_sec_base[s];
        const int64_t hw0 = hc.seg_hw0[s], sec0 = hc.seg_sec0[s];
        const int64_t bh = hw0 * st.wl, bs = sec0 * 1000;
        const bool rel32 = ev_time(io, hi - 1) - bs < (int64_t)0xffffffffLL;   // window keys by 32-bit division
        auto key_of = [&](int64_t tj, uint32_t& kh_, uint32_t& ks_) {
            if (rel32) { kh_ = hwb + (uint32_t)(tj - bh) / wl; ks_ = secb + (uint32_t)(tj - bs) / 1000u; }
            else { kh_ = hwb + (uint32_t)(tj / st.wl - hw0); ks_ = secb + (uint32_t)(tj / 1000 - sec0); }
        };
        // the tile's window rows; a range that leaves the LDS tables flushes them first
        uint32_t th0, ts0, th1, ts1;
        key_of(ev_time(io, max(tl.y * FILL_TILE, lo)), th0, ts0);
        key_of(ev_time(io, min(tl.y * FILL_TILE + FILL_TILE, hi) - 1), th1, ts1);
        const bool wide = th1 - th0 >= (uint32_t)ACC_K || ts1 - ts0 >= (uint32_t)ACC_K;
        if (wide || bh_k == NONE || th0 < bh_k || th1 >= bh_k + ACC_K || ts0 < bs_k || ts1 >= bs_k + ACC_K) {
            __syncthreads();
            if (bh_k != NONE) { lds_acc_flush(acc_h, hc.acc_hw, bh_k); lds_acc_flush(acc_s, hc.acc_sec, bs_k); }
            __syncthreads();
            lds_acc_clear(acc_h); lds_acc_clear(acc_s);
            bh_k = wide ? NONE : th0; bs_k = wide ? NONE : ts0;
            __syncthreads();
        }
        const uint32_t base = tl.y * FILL_TILE + (uint32_t)FG * threadIdx.x;
        const uint32_t a = max(base, lo), b = min(base + (uint32_t)FG, hi);
        if (a >= b) continue;
        const bool full = a == base && b == base + (uint32_t)FG;
        FillGrp g;
        int32_t wt[FG];
        if (full) {
            load16(g.m, io.ev.meta + base, FG * 4);
            if (rl || prm) load16(wt, io.v_wait + base, FG * 4);
        } else {
#pragma unroll
            for (int k = 0; k < FG; k++) {
                const uint32_t j = base + (uint32_t)k;
                const bool in = j >= a && j < b;
                g.m[k] = in ? ev_word(io, j) : PV_DTS_FAR;
                wt[k] = (in && (rl || prm)) ? io.v_wait[j] : 0;
            }
        }
        // decode (events outside the tile's part of the segment: no flags, count and time 0)
#pragma unroll
        for (int k = 0; k < FG; k++) {
            const uint32_t j = base + (uint32_t)k;
            const bool in = j >= a && j < b;
            g.f[k] = in ? ev_flags(g.m[k]) : (uint8_t)0;
            g.c[k] = in ? ev_count(io, g.m[k], j) : 0;
            g.t[k] = in ? ev_time(io, g.m[k], j) : 0;
        }
        const unsigned long long pw = hc.passbits[base >> 6];
        uint32_t sysm = 0;                                 // entries blocked before the controllers (EVF_SYSBLK)
#pragma unroll
        for (int k = 0; k < FG; k++)
            if ((g.f[k] & (SF_EV_EXIT | EVF_SYSBLK)) == EVF_SYSBLK) sysm |= 1u << k;
        const uint32_t bits = (all ? 0xffffu : (uint32_t)(pw >> (base & 63)) & ((1u << FG) - 1u)) & ~sysm;
        // exits: their entries' bits and times (gathers, all issued together)
        uint32_t exm = 0;
#pragma unroll
        for (int k = 0; k < FG; k++)
            if (base + (uint32_t)k >= a && base + (uint32_t)k < b && (g.f[k] & SF_EV_EXIT)) exm |= 1u << k;
        int64_t rf[FG], rts[FG]; uint32_t rlive = 0;
        if (exm) {
            if (io.eref) {
                if (full) load16(rf, io.eref + base, FG * 8);
                else {
#pragma unroll
                    for (int k = 0; k < FG; k++) rf[k] = ((exm >> k) & 1u) ? io.eref[base + k] : -1;
                }
            } else {
#pragma unroll
                for (int k = 0; k < FG; k++) rf[k] = -1;
            }
            unsigned long long rw[FG]; uint8_t rfl[FG];
#pragma unroll
            for (int k = 0; k < FG; k++) {
                const int64_t r = ((exm >> k) & 1u) ? rf[k] : -1;
                const uint32_t rc = r >= 0 && r < (int64_t)io.n ? (uint32_t)r : base;
                rw[k] = hc.passbits[rc >> 6];
                const uint32_t mr = ev_word(io, rc);
                rts[k] = r >= 0 ? ev_time(io, mr, rc) : (io.cts ? io.cts[base + k] : g.t[k]);
                rfl[k] = ev_flags(mr);
            }
#pragma unroll
            for (int k = 0; k < FG; k++) {
                if (!((exm >> k) & 1u)) continue;
                const int64_t r = rf[k];
                const uint32_t j = base + (uint32_t)k;
                if (r >= 0 && (r < (int64_t)lo || r >= (int64_t)j || !is_entry(rfl[k]))) *st.err = SF_ERR_INVALID;
                const bool live = r == -1 || (r >= (int64_t)lo && r < (int64_t)j && !(rfl[k] & EVF_SYSBLK) &&
                                            (all || ((rw[k] >> ((uint32_t)r & 63)) & 1ull)));
                if (live) rlive |= 1u << k;
            }
        }
        // verdicts and the group's contribution
        uint8_t vs[FG]; int32_t vw[FG]; uint16_t vr[FG];
        PAcc gp; gp.clear();
#pragma unroll
        for (int k = 0; k < FG; k++) {
            const uint32_t j = base + (uint32_t)k;
            vr[k] = 0; vw[k] = 0; vs[k] = 0;
            if (j < a || j >= b) continue;
            EvContrib e{};
            e.c = g.c[k];
            if (!(g.f[k] & SF_EV_EXIT)) {
                e.passed = (bits >> k) & 1u;
                // (a ParamFlow entry that a later rule blocks has slept in the throttle rules before it)
                e.wait = (prm || (rl && e.passed)) ? wt[k] : 0;
                if ((sysm >> k) & 1u) { e.status = sysblk_status(g.f[k]); vr[k] = (uint16_t)sysblk_rule(g.f[k]); }
                else {
                    e.status = e.passed ? (e.wait > 0 ? SF_V_PASS_WAIT : SF_V_PASS) : (prm ? SF_V_BLOCK_PARAM : SF_V_BLOCK_FLOW);
                    if (prm && !e.passed) vr[k] = io.v_rule[j];
                }
                e.touch = true;
            } else {
                e.live_exit = (rlive >> k) & 1u;
                e.status = e.live_exit ? SF_V_EXIT : SF_V_EXIT_IGNORED;
                e.touch = e.live_exit;
                e.rt = g.t[k] - rts[k];
                e.err = (g.f[k] & SF_EV_ERROR) != 0;
            }
            vs[k] = e.status; vw[k] = e.wait;
            if (e.touch) gp.add(e);
        }
        // statuses in sorted order (launch_scatter moves them); the few nonzero
        // waits and rule indices straight to the caller's arrays
        if (full) store16(io.v_status + base, vs, FG);     // (aligned like the flags loaded above)
        else {
#pragma unroll
            for (int k = 0; k < FG; k++)
                if (base + (uint32_t)k >= a && base + (uint32_t)k < b) io.v_status[base + k] = vs[k];
        }
        bool sparse = false;
#pragma unroll
        for (int k = 0; k < FG; k++) sparse |= (io.o_wait && vw[k]) || (io.o_rule && vr[k]);
        if (sparse) {
#pragma unroll
            for (int k = 0; k < FG; k++) {
                const uint32_t j = base + (uint32_t)k;
                if (j < a || j >= b || !((io.o_wait && vw[k]) || (io.o_rule && vr[k]))) continue;
                const uint32_t pi = io.perm[j];
                if (io.o_wait && vw[k]) io.o_wait[pi] = vw[k];       // (cleared before the decide phase)
                if (io.o_rule && vr[k]) io.o_rule[pi] = vr[k];
            }
        }
#ifdef SF_EXP_NOACC
        continue;
#endif
        if (!gp.n_touch) continue;
        // window rows of the group's first and last event (time-sorted): usually one
        int64_t tfirst = 0, tlast = 0;                    // unrolled selects (no dynamic register indexing)
#pragma unroll
        for (int k = 0; k < FG; k++) {
            if (base + (uint32_t)k == a) tfirst = g.t[k];
            if (base + (uint32_t)k + 1 == b) tlast = g.t[k];
        }
        uint32_t h0, s0, h1, s1;
        key_of(tfirst, h0, s0);
        key_of(tlast, h1, s1);
        if (h0 == h1 && s0 == s1) {
            if (bh_k != NONE) { lds_acc_add(acc_h, h0 - bh_k, gp); lds_acc_add(acc_s, s0 - bs_k, gp); }
            else { gp.flush(hc.acc_hw, h0); gp.flush(hc.acc_sec, s0); }
        } else {
            PAcc ph, ps; ph.clear(); ps.clear();
            uint32_t kh = NONE, ks = NONE;
            auto out = [&](PAcc& p, uint32_t key, bool sec) {
                if (key == NONE) return;
                if (bh_k != NONE) lds_acc_add(sec ? acc_s : acc_h, key - (sec ? bs_k : bh_k), p);
                else p.flush(sec ? hc.acc_sec : hc.acc_hw, key);
            };
#pragma unroll
            for (int k = 0; k < FG; k++) {
                const uint32_t j = base + (uint32_t)k;
                if (j < a || j >= b) continue;
                EvContrib e{};
                e.c = g.c[k];
                if (!(g.f[k] & SF_EV_EXIT)) { e.passed = (bits >> k) & 1u; e.touch = true; }
                else {
                    e.live_exit = (rlive >> k) & 1u; e.touch = e.live_exit;
                    e.rt = g.t[k] - rts[k]; e.err = (g.f[k] & SF_EV_ERROR) != 0;
                }
                if (!e.touch) continue;
                uint32_t kh_, ks_;
                key_of(g.t[k], kh_, ks_);
                if (kh_ != kh) { out(ph, kh, false); ph.clear(); kh = kh_; }
                if (ks_ != ks) { out(ps, ks, true); ps.clear(); ks = ks_; }
                ph.add(e); ps.add(e);
            }
            out(ph, kh, false); out(ps, ks, true);
        }
    }
    __syncthreads();
    if (bh_k != NONE) { lds_acc_flush(acc_h, hc.acc_hw, bh_k); lds_acc_flush(acc_s, hc.acc_sec, bs_k); }
}

__global__ void k_heavy_apply(DevState st, HeavyCtx hc, StreamCtx sc, const uint32_t* seg_nhw,
                              const uint32_t* seg_nsec, int cls) {
    uint32_t s;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;; t += gridDim.x * blockDim.x) {
        if (cls == 0) { if (!heavy_at(hc, t, &s)) return; }
        else if (!stream_at(sc, t, &s)) return;
        if (hc.seg_mode[s] >= SM_QPS) heavy_apply(st, hc, s, hc.seg_res[s], seg_nhw[s], seg_nsec[s]);
    }
}

// THREAD stream records and run tables (state-independent; at the head of the
// decide phase on stream A, before k_heavy_stream reads them: the sort phase of
// the next batch is the longer of the two pipelined phases)
void launch_thr_prep(Work& w, const DevBatch& b, hipStream_t s) {
    const uint32_t n = b.n;
    HeavyCtx hc = heavy_ctx(w);
    // (grids sized to the most tiles a batch of n events can have: small
    // SystemRule sub-batches do not pay for full-chip launches)
    const uint32_t tile_ub = n / FILL_TILE + n / (w.heavy_min + 1) + 2;
    const uint2* tiles1 = w.fill_tiles + w.fill_tile_cap;
    const int64_t* seref = b.eref ? w.s_eref : nullptr;
    const SortedEv ev = sorted_ev(w, b);
    const dim3 tgrid(std::min<uint32_t>(1024u, tile_ub));
    hipLaunchKernelGGL(k_thr_heads, tgrid, dim3(256), 0, s, ev, hc, tiles1, w.fill_ntiles,
                       w.tile_rc, w.segflag);
    // THREAD run mode tables (sf_stream.h thr_runs_segment)
    hipLaunchKernelGGL(k_thr_rscan, dim3(1), dim3(1024), 0, s, w.tile_rc, w.fill_ntiles);
    hipLaunchKernelGGL(k_thr_rid, tgrid, dim3(256), 0, s, ev, hc, tiles1, w.fill_ntiles, w.tile_rc);
    hipLaunchKernelGGL(k_thr_rec, tgrid, dim3(256), 0, s, ev, seref, hc, tiles1, w.fill_ntiles,
                       w.segflag);
}

// the decide phase's launches of this file's kernels (grids as launch_decide sizes them)
void launch_heavy_stream(const DevState& st, const SegIO& io, const HeavyCtx& hc, const StreamCtx& sc, const Work& w,
                         uint32_t max_heavy, hipStream_t s) {
    hipLaunchKernelGGL(k_heavy_stream, dim3(std::min(max_heavy, w.stream_grid)), dim3(HS_T), 0, s, st, io, hc, sc);
}
void launch_heavy_decide(const DevState& st, const SegIO& io, const HeavyCtx& hc, uint32_t max_heavy, hipStream_t s) {
    for_sample_count(st, [&](auto S) {
        hipLaunchKernelGGL(k_heavy_decide<decltype(S)::value>, dim3(max_heavy), dim3(64), 0, s, st, io, hc);
    });
}
void launch_heavy_fill(const DevState& st, const SegIO& io, const HeavyCtx& hc, const Work& w, uint32_t fgrid, int cls,
                       hipStream_t s) {
    hipLaunchKernelGGL(k_heavy_fill, dim3(fgrid), dim3(256), 0, s, st, io, hc,
                       w.fill_tiles + (cls ? w.fill_tile_cap : 0), w.fill_ntiles, cls);
}
void launch_heavy_apply(const DevState& st, const HeavyCtx& hc, const StreamCtx& sc, const Work& w, uint32_t max_heavy,
                        int cls, hipStream_t s) {
    hipLaunchKernelGGL(k_heavy_apply, dim3(blocks(max_heavy, 64)), dim3(64), 0, s, st, hc, sc, w.seg_nhw, w.seg_nsec,
                       cls);
}

}  // namespace sf
