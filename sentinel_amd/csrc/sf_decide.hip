// sf_decide.hip — the decide phase of a batch (launch_decide): the exit
// pairing, the light lanes, the xflow lane walk, and the host function that
// is the phase's stream graph (product code).
//
// The phase is stateful and runs in batch order.  Its kernels leave every
// status in sorted order (Work::v_status) and the few nonzero waits and rule
// indices in the caller's arrays; the verdict scatter (sf_scatter.hip) then
// moves the statuses to submission order.  Streams: A (s), B (s2), C (s3),
// 4 (s4) and the side stream (sv, an asynchronous batch's; else the scatter
// stays on A).  Events: PipeEvent (sf_internal.h); those marked (t) are
// recorded only when the engine times its kernels.
//
//   A: [launch_classify, when the sort phase did not run it]
//      k_fill                clears exit_of and the caller's wait / rule arrays
//      k_gather_exit         each exit's entry (sorted position), exit_of, create time
//      EV_FORK ------------> B, C and (wave walk on) 4 wait on it
//      launch_thr_prep       THREAD run tables (stream rules loaded)
//      EV_STREAM_START
//      k_heavy_stream        persistent; THREAD / RateLimiter heavy segments (sf_heavy.hip, sf_stream.h)
//      EV_STREAM_DONE
//      k_heavy_fill / k_heavy_apply of class 1 (the stream class)
//   B: k_heavy_decide        QPS / WarmUp / ParamFlow / generic heavy segments (sf_heavy.hip)
//      EV_HEAVY_DECIDED (t)
//      k_heavy_fill class 0  verdicts + per-window counter deltas from the pass bits
//      EV_HEAVY_FILLED (t)
//      k_heavy_apply class 0 deltas applied to the LeapArray state in time order
//      k_decide_light_qps, k_decide_short_qps   the lean QPS walks (window rules loaded)
//      EV_LEAN_DONE, EV_JOIN_B
//   C: k_decide_light, k_decide_short           one lane per light segment (sf_decide.h)
//      k_decide_x            one lane per xflow group segment (xflow rules loaded)
//      EV_LIGHT_DONE
//   4: k_decide_xw           the wave walk of long xflow segments (sf_xwave.hip)
//      EV_XWAVE_DONE
//   A: waits on EV_JOIN_B and EV_LIGHT_DONE; EV_JOINED_BC; waits on EV_XWAVE_DONE; EV_JOINED (t)
//   B: (origins) waits on EV_JOINED_BC; the origin pass (launch_ox_apply, sf_origin.hip),
//      beside the wave walk and the scatter; EV_ORIGIN_DONE
//   A: (side stream given) EV_SCATTER_FORK, which the side stream waits on
//   A or side: launch_scatter; then both A and the scatter's stream wait on
//      EV_ORIGIN_DONE (the next batch reads the origin nodes); EV_SCATTERED (t)
#include "sf_launch.h"
#include "sf_system.h"
#include "sf_xflow.h"

namespace sf {

// Exits only: the sorted position of each exit's entry.  The sort is stable
// and the segment holds one resource's events in submission order, so the
// entry is found by a binary search of the segment's submission indices (no
// inverse permutation scattered over the whole batch).  Forward map exit_of
// for THREAD-grade liveness; s_cts for entries of earlier batches.
__global__ void k_gather_exit(DevBatch b, const uint32_t* perm, const uint32_t* s_meta,
                              const uint32_t* head_scan, const uint32_t* seg_start, int64_t* s_eref,
                              int64_t* s_cts, uint32_t* exit_of, int32_t* err) {
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= b.n || !(ev_flags(s_meta[j]) & SF_EV_EXIT)) return;
    const uint32_t i = perm[j];
    const int64_t raw = b.eref[i];
    // -1: the entry passed before this batch (live, create_ts gives its time);
    // EREF_DEAD: it was blocked before this batch (the exit is ignored)
    if (raw < 0) { s_eref[j] = raw == EREF_DEAD ? EREF_DEAD : -1; s_cts[j] = b.cts ? b.cts[i] : 0; return; }
    const int64_t r = raw - b.base;                                      // view-local index
    if (r < 0) {
        // the entry was decided in an earlier sub-batch of this batch: live
        // (-1, its time as create_ts) unless it was blocked (-2: the exit is ignored)
        if (!b.vprev || b.res[r] != b.res[i] || (b.flags[r] & SF_EV_EXIT)) {
            *err = SF_ERR_INVALID; s_eref[j] = -1; s_cts[j] = 0; return;
        }
        s_eref[j] = v_blocked_any(b.vprev[r]) ? -2 : -1;
        s_cts[j] = b.ts[r];
        return;
    }
    const uint32_t lo = seg_start[head_scan[j] - 1];          // entry in [segment start, j)
    if (r >= (int64_t)i) { *err = SF_ERR_INVALID; s_eref[j] = -1; s_cts[j] = 0; return; }
    // galloping back from j (an entry is usually a few of its resource's events
    // before its exit: the probes stay on the lines the neighbours read), then
    // a binary search of the bracket
    uint32_t a = lo, e = j;
    for (uint32_t step = 1; j - lo > step; step <<= 1) {
        const uint32_t m = j - step;
        if ((int64_t)perm[m] < r) { a = m + 1; break; }
        e = m;
        if ((int64_t)perm[m] == r) { a = m; break; }
    }
    while (a < e) { const uint32_t m = (a + e) >> 1; if ((int64_t)perm[m] < r) a = m + 1; else e = m; }
    if (a >= j || (int64_t)perm[a] != r) { *err = SF_ERR_INVALID; s_eref[j] = -1; s_cts[j] = 0; return; }
    s_eref[j] = a;
    exit_of[a] = j;
}

// One lane per light segment; thread t walks the length classes from the
// longest down, so a wavefront holds segments of one class (similar length)
// and the long ones are dispatched first.
#ifndef SF_LIGHT_MINB
#define SF_LIGHT_MINB 1
#endif
#ifndef SF_LIGHT_NOPF_MINB
#define SF_LIGHT_NOPF_MINB 1          // (3 wavefronts per SIMD: 96 B of spills, config 3 15.2 vs 14.1 ms)
#endif
template <int MAXS, bool PF>
__global__ void __launch_bounds__(128, PF ? SF_LIGHT_MINB : SF_LIGHT_NOPF_MINB) k_decide_light(DevState st, SegIO io, const uint32_t* seg_start,
                                                      const uint32_t* seg_res, LightLists ll) {
    ev_open(io.ev);
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    int c = LCLS - 1;
    for (; c >= 0; c--) {
        const uint32_t n = ll.counts[c];
        if (t < n) break;
        t -= n;
    }
    if (c < 0) return;
    const uint32_t s = ll.list[ll.off[c] + t];
    decide_segment<MAXS, SF_EV_CH, PF>(st, io, seg_res[s], seg_start[s], seg_start[s + 1]);
}

// The lean QPS light segments (SM_LIGHTQ, > SHORT_MAX events) from the back
// of each class region, longest class first (decide_qps_segment).
template <int MAXS>
__global__ void __launch_bounds__(128) k_decide_light_qps(DevState st, SegIO io, const uint32_t* seg_start,
                                                          const uint32_t* seg_res, LightLists ll) {
    ev_open(io.ev);
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    int c = LCLS - 1;
    for (; c >= 0; c--) {
        const uint32_t n = ll.counts[LCLS + c];
        if (t < n) break;
        t -= n;
    }
    if (c < 0) return;
    const uint32_t s = ll.list[ll.off[c] + ll.cap[c] - 1 - t];
    decide_qps_segment<MAXS>(st, io, seg_res[s], seg_start[s], seg_start[s + 1]);
}

// One lane per short light segment, from the dense short list (k_classify;
// see SHORT_MAX).
template <int MAXS, bool PF>
__global__ void __launch_bounds__(128, PF ? SF_LIGHT_MINB : SF_LIGHT_NOPF_MINB) k_decide_short(DevState st, SegIO io, const uint32_t* seg_start,
                                                      const uint32_t* seg_res, LightLists ll,
                                                      const uint32_t* n_short) {
    ev_open(io.ev);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_short[0]) return;
    const uint32_t s = ll.list[ll.off[0] + t];
    decide_segment<MAXS, SF_EV_CH, PF>(st, io, seg_res[s], seg_start[s], seg_start[s + 1]);
}

// One lane per xflow group segment (sf_xflow.h): origin / context / RELATE
// rules (the long segments k_decide_xw takes excepted).  EMB: with an embedded
// token server (st.emb), bound cluster rules take their tokens from it.
template <int MAXS, bool EMB>
__global__ void __launch_bounds__(64) k_decide_x(DevState st, SegIO io, const uint32_t* seg_start,
                                                 const uint32_t* seg_res, const uint8_t* seg_mode,
                                                 const uint32_t* n_seg) {
    ev_open(io.ev);
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= *n_seg || seg_mode[s] != SM_XFLOW) return;
    if (xw_take(st, seg_res[s], seg_start[s + 1] - seg_start[s])) return;
    if constexpr (EMB)
        if (xcl_take(st, seg_res[s], seg_start[s + 1] - seg_start[s])) return;       // k_decide_xcl's
    decide_xgroup<MAXS, EMB>(st, io, seg_start[s], seg_start[s + 1]);
}

// One lane per short segment routed to the lean QPS walk (SM_LIGHTQ), from
// the back of the dense short list like k_decide_short.
template <int MAXS>
__global__ void __launch_bounds__(128) k_decide_short_qps(DevState st, SegIO io, const uint32_t* seg_start,
                                                          const uint32_t* seg_res, LightLists ll,
                                                          const uint32_t* n_short) {
    ev_open(io.ev);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_short[WC_SHORT_QPS - WC_SHORT]) return;
    const uint32_t s = ll.list[ll.off[0] + ll.cap[0] - 1 - t];
    decide_qps_segment<MAXS>(st, io, seg_res[s], seg_start[s], seg_start[s + 1]);
}

// the light lanes of a batch (k_classify's lists), longest class first; the
// lean QPS walks only where a QPS DefaultController rule is loaded
// (the lean QPS walks go on stream B after its heavy kernels, beside the
// generic walks on C: different segments, different resources)
template <int MAXS, bool PF>
static void launch_light(const DevState& st, const SegIO& io, const Work& w, const LightLists& ll, uint32_t max_seg,
                         hipStream_t s3, hipStream_t s2) {
    const unsigned TD = 128;
    const uint32_t* n_short = w.counters + WC_SHORT;      // [0] generic, [WC_SHORT_QPS - WC_SHORT] lean QPS
    hipLaunchKernelGGL((k_decide_light<MAXS, PF>), dim3(blocks(max_seg, TD)), dim3(TD), 0, s3, st, io, w.seg_start,
                       w.seg_res, ll);
    if (st.n_window_rules) {
        hipLaunchKernelGGL(k_decide_light_qps<MAXS>, dim3(blocks(max_seg, TD)), dim3(TD), 0, s2, st, io, w.seg_start,
                           w.seg_res, ll);
        hipLaunchKernelGGL(k_decide_short_qps<MAXS>, dim3(blocks(max_seg, TD)), dim3(TD), 0, s2, st, io, w.seg_start,
                           w.seg_res, ll, n_short);
    }
    hipLaunchKernelGGL((k_decide_short<MAXS, PF>), dim3(blocks(max_seg, TD)), dim3(TD), 0, s3, st, io, w.seg_start,
                       w.seg_res, ll, n_short);
}
static void launch_light(const DevState& st, const SegIO& io, const Work& w, uint32_t max_seg, hipStream_t s3,
                         hipStream_t s2) {
    LightLists ll{w.light_list, w.lcounts, {}, {}};
    for (int c = 0; c < LCLS; c++) { ll.off[c] = w.loff[c]; ll.cap[c] = w.lcap[c]; }
    // (no ParamFlow / degrade rule loaded: the lanes without that code)
    const bool pf = st.n_prule != 0 || st.dg_rr_of != nullptr;
    for_sample_count(st, [&](auto S) {
        constexpr int MAXS = decltype(S)::value;
        if (pf) launch_light<MAXS, true>(st, io, w, ll, max_seg, s3, s2);
        else launch_light<MAXS, false>(st, io, w, ll, max_seg, s3, s2);
    });
}

static void launch_gather_exit(const DevState& st, Work& w, const DevBatch& b, hipStream_t s) {
    hipLaunchKernelGGL(k_gather_exit, dim3(blocks(b.n, 256)), dim3(256), 0, s, b, w.perm, w.s_meta,
                       w.head_scan, w.seg_start, w.s_eref, w.s_cts, w.exit_of, st.err);
}

static void launch_decide_x(const DevState& st, const SegIO& io, const Work& w, uint32_t max_seg, hipStream_t s) {
    for_sample_count(st, [&](auto S) {
        if (st.emb)
            hipLaunchKernelGGL((k_decide_x<decltype(S)::value, true>), dim3(blocks(max_seg, 64)), dim3(64), 0, s, st,
                               io, w.seg_start, w.seg_res, w.seg_mode, w.n_seg);
        else
            hipLaunchKernelGGL((k_decide_x<decltype(S)::value, false>), dim3(blocks(max_seg, 64)), dim3(64), 0, s, st,
                               io, w.seg_start, w.seg_res, w.seg_mode, w.n_seg);
    });
}

// what the deciding kernels read and write of the batch
static SegIO seg_io(const DevState& st, const Work& w, const DevBatch& b, const DevVerdicts& out) {
    SegIO io;
    io.ts = nullptr; io.cnt = nullptr; io.flags = nullptr;     // (host build only)
    io.ev = sorted_ev(w, b);
    io.eref = b.eref ? w.s_eref : nullptr; io.cts = b.eref ? w.s_cts : nullptr;
    io.arg_slots = b.arg_slots; io.nargs = (b.arg_slots && b.nargs) ? w.s_nargs : nullptr;
    io.atag = w.s_atag; io.abits = w.s_abits; io.n = b.n;
    io.aoff = b.aoff; io.etag = b.etag; io.ebits = b.ebits;
    io.v_status = w.v_status; io.v_wait = w.v_wait; io.v_rule = w.v_rule;
    io.perm = w.perm; io.o_status = out.status; io.o_wait = out.wait; io.o_rule = out.rule;
    io.ev_res = b.res; io.ev_origin = b.origin; io.ev_ctx = b.ctx; io.shard_count = st.shard_count;
    return io;
}

// The decide phase of a batch: the stream graph of the file header.  s, s2, s3
// and s4 are streams A, B, C and 4; sv is the side stream (null: the scatter
// stays on A).
hipError_t launch_decide(const DevState& st, Work& w, const DevBatch& b, const DevVerdicts& out,
                         hipStream_t s, hipStream_t s2, hipStream_t s3, hipStream_t s4, hipEvent_t* ev, bool timing,
                         const OxPlan* ox, bool classify, hipStream_t sv) {
    const uint32_t n = b.n;
    if (n == 0) return hipSuccess;
    if (classify) launch_classify(st, w, b, s, ev, timing);
    const SegIO io = seg_io(st, w, b, out);
    HeavyCtx hc = heavy_ctx(w);
    if (timing) hc.hticks = w.hticks;
    const uint32_t max_seg = n < st.R ? n : st.R;
    const uint32_t max_heavy = n / (w.heavy_min + 1) + 1;
    StreamCtx sc{w.stream_list, w.counters + WC_STREAM_FRONT, w.seg_cap, timing ? w.sticks : nullptr,
                 w.counters + WC_STREAM_NEXT};
    // each exit's entry (sorted position, exit_of) and create time: state-
    // independent, but here at the head of the decide phase rather than in the
    // sort phase, the longer of the two pipelined phases (k_classify does not
    // read them; every deciding kernel does)
    {
        FillSet f;
        if (b.eref || st.n_stream_rules) f.add(w.exit_of, (size_t)n * 4, 0xff);   // (read by k_gather_exit, k_thr_rec)
        // waits and rule indices are zero for almost every event: clear them with
        // coalesced stores, then the deciding kernels scatter only the nonzero ones
        f.add(out.wait, (size_t)n * sizeof(int32_t), 0);
        f.add(out.rule, (size_t)n * sizeof(uint16_t), 0);
        launch_fill(f, s);
    }
    if (b.eref) launch_gather_exit(st, w, b, s);
    hipEventRecord(ev[EV_FORK], s);
    // (the THREAD / RateLimiter class exists only with such rules loaded)
    if (st.n_stream_rules) launch_thr_prep(w, b, s);
    hipEventRecord(ev[EV_STREAM_START], s);
    if (st.n_stream_rules) launch_heavy_stream(st, io, hc, sc, w, max_heavy, s);
    hipEventRecord(ev[EV_STREAM_DONE], s);
    hipStreamWaitEvent(s2, ev[EV_FORK], 0);
    hipStreamWaitEvent(s3, ev[EV_FORK], 0);
    // long one-resource xflow segments: the wave walk, on its own stream from
    // the fork (its segments share no node or rule with any other kernel of the
    // phase; the longest of them is usually the phase's critical path)
    const bool xw_on = st.xmap && st.xw;
    if (xw_on) {
        hipStreamWaitEvent(s4, ev[EV_FORK], 0);
        launch_xw(st, io, w, n, s4);
        if (st.emb) launch_xcl(st, io, w, n, s4);      // bound-rule segments (sf_xcluster.hip), after the wave walk
        hipEventRecord(ev[EV_XWAVE_DONE], s4);
    }
    launch_heavy_decide(st, io, hc, max_heavy, s2);
    if (timing) hipEventRecord(ev[EV_HEAVY_DECIDED], s2);
    // verdicts + window deltas of each heavy class as soon as its decisions are done
    const uint32_t fgrid = std::min<uint32_t>(w.fill_grid, n / FILL_TILE + max_heavy + 1);   // tiles of this batch at most
    launch_heavy_fill(st, io, hc, w, fgrid, 0, s2);
    if (timing) hipEventRecord(ev[EV_HEAVY_FILLED], s2);
    launch_heavy_apply(st, hc, sc, w, max_heavy, 0, s2);
    if (st.n_stream_rules) {
        launch_heavy_fill(st, io, hc, w, fgrid, 1, s);
        launch_heavy_apply(st, hc, sc, w, max_heavy, 1, s);
    }

    launch_light(st, io, w, max_seg, s3, s2);
    if (st.xmap) launch_decide_x(st, io, w, max_seg, s3);
    hipEventRecord(ev[EV_LIGHT_DONE], s3);         // light done (also the join of C)
    hipEventRecord(ev[EV_LEAN_DONE], s2);          // the lean QPS walks done (after B's heavy kernels)
    hipEventRecord(ev[EV_JOIN_B], s2);             // join B and C
    hipStreamWaitEvent(s, ev[EV_JOIN_B], 0);
    hipStreamWaitEvent(s, ev[EV_LIGHT_DONE], 0);
    hipEventRecord(ev[EV_JOINED_BC], s);           // (the origin pass below does not wait for the wave walk)
    if (xw_on) hipStreamWaitEvent(s, ev[EV_XWAVE_DONE], 0);
    if (timing) hipEventRecord(ev[EV_JOINED], s);
    // origin nodes no rule reads (sf_origin.hip): from the sorted verdicts
    // of the other segments, beside the wave walk and the verdict scatter
    if (ox) {
        hipStreamWaitEvent(s2, ev[EV_JOINED_BC], 0);
        const hipError_t e = launch_ox_apply(st, w, b, ox->n_heavy, ox->n_pairs, ox->win, s2);
        if (e != hipSuccess) return e;
        hipEventRecord(ev[EV_ORIGIN_DONE], s2);
    }
    // the verdict scatter on sv when given (an asynchronous batch: beside the
    // next batch's decide phase, which reads no status of this one)
    hipStream_t vs = sv ? sv : s;
    if (vs != s) {
        hipEventRecord(ev[EV_SCATTER_FORK], s);
        hipStreamWaitEvent(vs, ev[EV_SCATTER_FORK], 0);
    }
    launch_scatter(w, n, out.status, vs);
    if (ox) {
        hipStreamWaitEvent(s, ev[EV_ORIGIN_DONE], 0);          // the next batch reads the origin nodes
        if (vs != s) hipStreamWaitEvent(vs, ev[EV_ORIGIN_DONE], 0);
    }
    if (timing) hipEventRecord(ev[EV_SCATTERED], vs);
    return hipGetLastError();
}

}  // namespace sf
