// sf_xcluster.hip — the wave route of the embedded token server (product code):
// k_decide_xcl, one wavefront per long one-resource segment whose only flow
// rule is a bound cluster rule (sf_load_cluster_binds; xcl_take, sf_xflow.h),
// so a hot cluster-limited resource is not one lane's serial replay.
//
// The shape follows k_rls_wave (sf_rls.hip) and k_decide_xw (sf_xwave.hip).  A
// segment is cut into chunks of at most 64 events that share one
// ClusterMetric bucket window (the cluster rule's wl), one second bucket and
// one minute bucket of the ClusterNode.  Inside a chunk the sum
// of PASS over the other buckets is constant (the bucket that would leave
// during the window is the current one, which currentWindow has just reset), so
// with no prioritized entry and every acquireCount > 0
//     entry l passes  iff  thr - (sum0 + P_l) / isec - c_l >= 0
// (ClusterFlowChecker.java:68-80) where P_l is the sum of the counts of the
// chunk's passing entries before it.  As sf_rls.hip:24-35 describes, the
// iteration "assume every candidate passes, rescan, repeat until stable"
// settles entry l at the latest in round l + 1: each round fixes at least the
// first entry not yet final, because its prefix only counts final entries.  So
// at most 65 rounds give the serial result.  Exits and entries that carry a
// forced or authority block make no request (FlowSlot is never reached), are
// no candidates and keep their verdict.  The chunk's PASS / PASS_REQUEST /
// BLOCK / BLOCK_REQUEST sums go to the metric bucket once.
//
// StatisticSlot's accounting of the chunk goes to the ClusterNode as sums, as
// xw_apply does (sf_xwave.hip): pass and block counts and the thread delta of
// the chunk's entries once, into the one second bucket and the one minute
// bucket they share; every lane writes its own entry's status.  Lane 0 keeps
// the node in a NodeWin for the segment.  Exits and forced blocks of the chunk
// go through the walk's own xg_event after the sums (their additions to the
// same buckets commute with them; an exit reads its entry's status, written
// before).
//
// A chunk with a prioritized entry, an acquireCount <= 0, a window older than
// its bucket (currentWindow's throwaway case) or, in a batch with origins, any
// chunk, is replayed by lane 0 through xg_event / emb_request: the lane route
// on that chunk.  EmbState::stats counts wave chunks [0] and serial chunks [1].
#include "sf_launch.h"
#include "sf_xflow.h"

namespace sf {

__device__ __forceinline__ long long xcl_scan_excl(long long v, uint32_t lane) {
    long long x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const long long y = __shfl_up(x, o);
        if ((int)lane >= o) x += y;
    }
    return x - v;
}

template <int MAXS>
__global__ void __launch_bounds__(64) k_decide_xcl(DevState st, SegIO io, const uint32_t* seg_start,
                                                   const uint32_t* seg_res, const uint32_t* list,
                                                   const uint32_t* n_list) {
    ev_open(io.ev);
    const uint32_t lane = threadIdx.x;
    const ParamTable pt{st.ptab, st.pcap_mask, st.err, st.pins};
    const EmbState& emb = *st.emb;
    const TokState& ts = emb.ts;
    const uint32_t nl = *n_list;
    for (uint32_t q = blockIdx.x; q < nl; q += gridDim.x) {
        const uint32_t s = list[q];
        const uint32_t lo = seg_start[s], hi = seg_start[s + 1], l = seg_res[s];
        const int64_t fid = emb.bind[st.rule_off[l]];
        const int32_t r = id_lookup(ts, fid, false);           // (xcl_take: the flowId is loaded, no limiter)
        if (r < 0) { if (lane == 0) *st.err = SF_ERR_INVALID; continue; }
        const ClRule rule = ts.rules[r];
        const int32_t connected = rule.ns >= 0 ? ts.ns[rule.ns].connected : 0;
        const double thr = (rule.threshold_type == SF_THRESHOLD_GLOBAL ? rule.count : rule.count * connected) * ts.exceed_count;
        const double isec = rule.interval / 1000.0;
        ClMetric m{&ts.fstate[r], rule.S, rule.wl, rule.interval, isec};
        // lane 0 keeps the ClusterNode (and, on serial chunks, origin / context nodes) for the segment
        NodeWin<MAXS> cn, on, dn;
        uint32_t cl = XNONE, oi = XNONE, di = XNONE;
        if (lane == 0) { nw_load(cn, st, cluster_rows(st, l)); cl = l; }
        unsigned long long n_wave = 0, n_serial = 0;
        uint32_t p = lo;
        while (p < hi) {
            // the chunk: up to 64 events of the metric window, the node's second bucket and its minute
            // bucket of event p
            const int64_t t0 = ev_time(io, p);
            int64_t wend = t0 - t0 % rule.wl + rule.wl;
            { const int64_t a = t0 - t0 % st.wl + st.wl, b = t0 - t0 % 1000 + 1000; wend = a < wend ? a : wend; wend = b < wend ? b : wend; }
            const uint32_t j = p + lane;
            const bool in = j < hi;
            uint32_t mw = 0; int64_t t = 0; int32_t c = 0; uint8_t fl = 0;
            if (in) { mw = ev_word(io, j); t = ev_time(io, mw, j); c = ev_count(io, mw, j); fl = ev_flags(mw); }
            const unsigned long long beyond = __ballot(!in || t >= wend);
            const uint32_t len = beyond ? (uint32_t)(__ffsll((long long)beyond) - 1) : 64u;      // >= 1: event p itself
            const bool mine = lane < len;
            const bool cand = mine && !(fl & (SF_EV_EXIT | EVF_SYSBLK));
            const unsigned long long cm = __ballot(cand);
            bool serial = io.ev_origin != nullptr || __ballot(cand && ((fl & SF_EV_PRIO) || c <= 0)) != 0;
            long long sum0 = 0;
            if (!serial && cm) {                                 // (no candidate: no request, the metric is not touched)
                int k = 0;
                if (lane == 0) { k = m.cur(t0); if (k >= 0) sum0 = m.sum(CE_PASS, t0); }
                k = __shfl(k, 0);
                sum0 = __shfl(sum0, 0);
                if (k < 0) serial = true;                        // the throwaway bucket: what is added is lost
            }
            if (serial) {
                if (lane == 0) {
                    for (uint32_t e = p; e < p + len; e++) xg_event<MAXS, true>(st, io, pt, lo, e, cn, on, dn, cl, oi, di);
                    n_serial++;
                }
                __syncthreads();
                p += len;
                continue;
            }
            // fixed point: start from "every candidate passes"
            unsigned long long pass = cm;
            for (int round = 0; round < 65; round++) {
                const bool pl = (pass >> lane) & 1ull;
                const long long pre = xcl_scan_excl(pl ? (long long)c : 0ll, lane);
                const bool ok = cand && (thr - (double)wadd(sum0, pre) / isec - c >= 0);
                const unsigned long long np = __ballot(ok);
                if (np == pass) break;
                pass = np;
            }
            const bool pl = cand && ((pass >> lane) & 1ull);
            // every lane writes its entry's status (wait 0, rule_idx 0: the cleared arrays already say so)
            if (cand) io.v_status[j] = pl ? SF_V_PASS : SF_V_BLOCK_FLOW;
            const long long pc = (long long)wave_sum((unsigned long long)(pl ? (long long)c : 0ll));
            const long long bc = (long long)wave_sum((unsigned long long)((cand && !pl) ? (long long)c : 0ll));
            const int npass = __popcll(pass), nblock = __popcll(cm) - npass;
            unsigned long long others = __ballot(mine && !cand);
            __syncthreads();                                     // (the statuses above: read by the exits below)
            if (lane == 0) {
                if (npass) { m.add(CE_PASS, pc, t0); m.add(CE_PASS_REQUEST, npass, t0); }
                if (nblock) { m.add(CE_BLOCK, bc, t0); m.add(CE_BLOCK_REQUEST, nblock, t0); }
                // StatisticSlot's accounting (StatisticSlot.java:64-123) of the chunk's entries as sums: they
                // share the node's second and minute bucket, and every update of a bucket is an addition
                if (npass) {
                    cn.threads += npass;
                    cn.sec_apply(t0, [&](Bucket& b) { b.pass = wadd(b.pass, pc); });
                    cn.min_apply(t0, [&](Bucket& b) { b.pass = wadd(b.pass, pc); });
                }
                if (nblock) {
                    cn.sec_apply(t0, [&](Bucket& b) { b.block = wadd(b.block, bc); });
                    cn.min_apply(t0, [&](Bucket& b) { b.block = wadd(b.block, bc); });
                }
                // exits and forced blocks of the chunk (same buckets: their additions commute with the sums)
                while (others) {
                    const uint32_t k = (uint32_t)(__ffsll((long long)others) - 1);
                    others &= others - 1;
                    xg_event<MAXS, true>(st, io, pt, lo, p + k, cn, on, dn, cl, oi, di);
                }
                n_wave++;
            }
            __syncthreads();
            p += len;
        }
        if (lane == 0) {
            if (cl != XNONE) nw_store(cn, st, cluster_rows(st, cl));
            if (oi != XNONE) nw_store(on, st, aux_rows(st, oi));
            if (di != XNONE) nw_store(dn, st, aux_rows(st, di));
            if (emb.stats) {
                if (n_wave) atomicAdd(&emb.stats[0], n_wave);
                if (n_serial) atomicAdd(&emb.stats[1], n_serial);
            }
        }
        __syncthreads();
    }
}

// the wave route of a batch of n events over Work::xcl_list (k_classify)
void launch_xcl(const DevState& st, const SegIO& io, const Work& w, uint32_t n, hipStream_t s) {
    const unsigned g = (unsigned)std::min<size_t>((size_t)n / XW_MIN + 1, 2048);
    for_sample_count(st, [&](auto S) {
        hipLaunchKernelGGL(k_decide_xcl<decltype(S)::value>, dim3(g), dim3(64), 0, s, st, io, w.seg_start, w.seg_res,
                           w.xcl_list, w.counters + WC_XCL_LIST);
    });
}

}  // namespace sf
