// sf_xwave.hip — the wave walk of long one-resource xflow segments
// (k_decide_xw, launch_xw): one wavefront per segment of k_classify's xw_list,
// on stream 4 of the decide phase (sf_decide.hip).  Product code.
#include "sf_launch.h"
#include "sf_xflow.h"

namespace sf {

// ---- the wave walk of a long xflow segment (one resource, DIRECT rules)
// A wavefront takes the segment in chunks of at most 64 events that share
// one second-window bucket and one minute bucket.  Per chunk:
//  1. every lane checks its entry against the first rule that selects a node
//     (FlowRuleComparator order: origin-specific and `other` rules before
//     `default`), on the node and rule state as they stand at the chunk's
//     start.  Within one bucket a node's pass count and a RateLimiter's
//     latestPassedTime only grow, the WarmUp threshold is fixed for the second
//     (syncToken reads the previous second; on an origin node it waits until
//     the walk has synced the second, since the rule's tokens are shared by
//     every origin and the first check of the second decides them), and a
//     THREAD count can fall at most by the exits ahead of the lane in the
//     chunk, so an entry blocked at the start state is blocked in the serial
//     order too, by that rule;
//  2. lane 0 runs the reference walk (xg_event) over the other entries --
//     those the start state lets pass, prioritized entries, and the exits when
//     a THREAD rule reads thread counts -- in order;
//  3. the blocked entries' blocks and the remaining exits' completions only
//     add to the chunk's buckets (which no check of this chunk reads), so they
//     are summed per node in LDS and added once per node.
// Verdicts, node state and rule state equal the serial walk's.
enum : uint8_t { XWC_SERIAL = 1, XWC_BLOCK = 2, XWC_EXIT = 3, XWC_PASS = 4 };
constexpr uint32_t XW_KCAP = 128;                 // LDS node rows of a chunk (<= 64 origins + the ClusterNode)
struct XwRow {
    unsigned long long blk, succ, rt, exc, pass; long long thr, minrt;
    unsigned int nblk, ncmp, nexc, npass, key, pad;
};
__device__ __forceinline__ void xw_add(XwRow& r, int64_t blk, int nblk, int64_t succ, int64_t rt, int64_t minrt,
                                       int64_t exc, int nexc, int64_t thr, int ncmp, int64_t pass = 0, int npass = 0) {
    if (nblk) { atomicAdd(&r.blk, (unsigned long long)blk); atomicAdd(&r.nblk, 1u); }
    if (npass) {
        atomicAdd(&r.pass, (unsigned long long)pass); atomicAdd(&r.npass, 1u);
        atomicAdd((unsigned long long*)&r.thr, 1ull);
    }
    if (ncmp) {
        atomicAdd(&r.succ, (unsigned long long)succ); atomicAdd(&r.rt, (unsigned long long)rt);
        atomicMin(&r.minrt, (long long)minrt); atomicAdd((unsigned long long*)&r.thr, (unsigned long long)thr);
        atomicAdd(&r.ncmp, 1u);
    }
    if (nexc) { atomicAdd(&r.exc, (unsigned long long)exc); atomicAdd(&r.nexc, 1u); }
}
// a row's sums into a node (all events of the chunk are in the bucket of t0):
// one currentWindow lookup per window for all of the row's counters
template <int MAXS>
__device__ __forceinline__ void xw_apply(NodeWin<MAXS>& nd, const XwRow& r, int64_t t0) {
    const bool hp = r.npass != 0, hb = r.nblk != 0, hc = r.ncmp != 0, he = r.nexc != 0;
    if (!(hp || hb || hc || he)) return;
    const int64_t p = (int64_t)r.pass, b = (int64_t)r.blk, sc = (int64_t)r.succ, rt = (int64_t)r.rt, mr = r.minrt,
                  e = (int64_t)r.exc;
    auto f = [&](Bucket& x) {
        if (hp) x.pass = wadd(x.pass, p);
        if (hb) x.block = wadd(x.block, b);
        if (hc) { x.succ = wadd(x.succ, sc); x.rt = wadd(x.rt, rt); if (mr < x.min_rt) x.min_rt = mr; }
        if (he) x.exc = wadd(x.exc, e);
    };
    nd.sec_apply(t0, f);
    nd.min_apply(t0, f);
    if (hp || hc) nd.threads = wadd(nd.threads, r.thr);
}

// ---- the exact chunk solve (S <= 2, no prioritized entry in the chunk)
// The chunk's verdicts as the fixed point of the serial recurrence: each
// entry's checks read its nodes' pass counts / thread counts and each
// RateLimiter's latestPassedTime as left by the entries before it in the
// chunk; given a guess of every verdict (all pass to start), every lane
// re-evaluates its entry from prefix sums over the earlier lanes (pass counts
// per node, thread deltas per node with the exits' liveness from their
// entries' verdicts, a max-plus scan x -> max(x + cost, t) per RateLimiter
// rule over the entries that passed it).  Each round makes at least the
// earliest wrong lane right (its inputs come only from earlier lanes), so the
// iteration reaches the serial result within L + 1 rounds; under saturation
// two or three.  Node bases are read once per chunk: a pass count is its
// window sum at the chunk's time plus the chunk's earlier passes (all events
// of the chunk fall in the same current bucket, every older bucket stays
// valid through it), the WarmUp threshold and the RateLimiter cost are fixed
// for the second (the ClusterNode's syncToken is applied on a copy: its
// previous-second QPS is the same for every event).
struct XwRuleC { double thr, qps; int64_t lstart; DevRuleState rs; int32_t sync, pad; };
struct XwScratch {
    long long base[XW_KCAP], thr[XW_KCAP];
    uint32_t ko[XW_KCAP];
    int os[64];
    long long cm[64], td[64];
    XwRuleC rc[MAX_RULES];
};
constexpr long long XW_MPNEG = INT64_MIN / 4;                  // max-plus "minus infinity"
// the segment's origin nodes held in LDS across chunks (exact-solve chunks
// read and write them there; a chunk on the serial path, the end of the
// segment, or a full cache writes them back)
constexpr uint32_t XW_OC = XW_KCAP - 1;                        // (chunk row r = cache slot r - 1)
struct XwCache { unsigned int key[XW_OC]; uint32_t ko[XW_OC]; unsigned int n; };
__device__ __forceinline__ NodeWin<2>& xw_node(unsigned char* ocnw, uint32_t slot) {
    return reinterpret_cast<NodeWin<2>*>(ocnw)[slot];
}
__device__ void xw_cache_flush(const DevState& st, XwCache& oc, unsigned char* ocnw, uint32_t lane) {
    __syncthreads();
    for (uint32_t k = lane; k < XW_OC; k += 64) {
        if (oc.key[k] && oc.ko[k] != XNONE) nw_store(xw_node(ocnw, k), st, aux_rows(st, oc.ko[k]));
        oc.key[k] = 0;
    }
    if (lane == 0) oc.n = 0;
    __syncthreads();
}

// wavefront scans on DPP (row shifts inside each 16-lane row, then the row
// broadcasts of lanes 15 and 31): a handful of ALU cycles per step instead of
// an LDS-crossbar shuffle; 64-bit values move as two 32-bit halves, lanes
// without a source keep `idv` (the operation's identity)
template <int CTRL, int ROWMASK>
__device__ __forceinline__ long long xw_dpp(long long v, long long idv) {
    const unsigned long long u = (unsigned long long)v, iu = (unsigned long long)idv;
    const int lo = __builtin_amdgcn_update_dpp((int)(unsigned)iu, (int)(unsigned)u, CTRL, ROWMASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(unsigned)(iu >> 32), (int)(unsigned)(u >> 32), CTRL, ROWMASK, 0xf, false);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}
template <class F>
__device__ __forceinline__ long long xw_scan_op(long long x, long long idv, F f) {
    x = f(x, xw_dpp<0x111, 0xf>(x, idv));        // row_shr:1
    x = f(x, xw_dpp<0x112, 0xf>(x, idv));        // row_shr:2
    x = f(x, xw_dpp<0x114, 0xf>(x, idv));        // row_shr:4
    x = f(x, xw_dpp<0x118, 0xf>(x, idv));        // row_shr:8
    x = f(x, xw_dpp<0x142, 0xa>(x, idv));        // row_bcast:15 -> rows 1, 3
    x = f(x, xw_dpp<0x143, 0xc>(x, idv));        // row_bcast:31 -> rows 2, 3
    return x;
}
__device__ __forceinline__ long long xw_excl_scan(long long v, uint32_t) {
    return xw_scan_op(v, 0, [](long long x, long long y) { return x + y; }) - v;
}
// wavefront total / minimum (lane 63 of the inclusive scan)
__device__ __forceinline__ long long xw_wsum(long long v) {
    return __shfl(xw_scan_op(v, 0, [](long long x, long long y) { return x + y; }), 63);
}
__device__ __forceinline__ long long xw_wmin(long long v) {
    return __shfl(xw_scan_op(v, INT64_MAX, [](long long x, long long y) { return y < x ? y : x; }), 63);
}
// inclusive max-plus scan of f(x) = max(x + a, b) in lane order (an earlier
// lane's (pa, pb) composed under this lane's: (pa + a, max(pb + a, b)))
template <int CTRL, int ROWMASK>
__device__ __forceinline__ void xw_mp_step(long long& a, long long& b) {
    const long long pa = xw_dpp<CTRL, ROWMASK>(a, 0), pb = xw_dpp<CTRL, ROWMASK>(b, XW_MPNEG);
    b = max(pb + a, b);
    a = pa + a;
}
__device__ __forceinline__ void xw_mp_scan(long long& a, long long& b, uint32_t) {
    xw_mp_step<0x111, 0xf>(a, b);
    xw_mp_step<0x112, 0xf>(a, b);
    xw_mp_step<0x114, 0xf>(a, b);
    xw_mp_step<0x118, 0xf>(a, b);
    xw_mp_step<0x142, 0xa>(a, b);
    xw_mp_step<0x143, 0xc>(a, b);
}

__device__ __forceinline__ void xw_solve_chunk(const DevState& st, NodeWin<2>& snap, XwRow* rows, XwScratch& xs,
                               XwCache& oc, unsigned char* ocnw,
                               uint32_t lane, uint32_t L, int64_t t0, int64_t t,
                               uint8_t fl, int32_t c, uint32_t origin, int eidx, bool live_pre, uint32_t l, uint32_t r0,
                               uint32_t r1, uint8_t* myc, uint8_t* mst, int* mrule, int64_t* mwait, int* my_row,
                               bool* x_live, unsigned long long* pfs = nullptr) {
#ifdef SF_XW_PROFILE
    unsigned long long pt_ = wall_clock64();
#define XS_PF(k) if (lane == 0 && pfs) { const unsigned long long x_ = wall_clock64(); pfs[k] += x_ - pt_; pt_ = x_; }
#else
#define XS_PF(k)
#endif
    const bool valid = lane < L;
    const bool is_exit = valid && (fl & SF_EV_EXIT);
    const bool is_sys = valid && !is_exit && (fl & EVF_SYSBLK);
    const bool is_solve = valid && !is_exit && !is_sys;
    const uint32_t nrules = r1 - r0;
    // the chunk's origin rows (row 0: the ClusterNode; row r: cache slot r - 1),
    // a node loaded into the cache at its first event of the segment; the
    // cache is written back only when this chunk's new origins do not fit
    {
        bool miss = false;
        if (valid && origin != SF_ORIGIN_NONE) {
            uint32_t h = (uint32_t)(mix64(origin) % XW_OC);
            miss = true;
            for (uint32_t q = 0; q < XW_OC; q++) {
                const unsigned int k = oc.key[h];
                if (k == origin + 1u) { miss = false; break; }
                if (k == 0u) break;
                h = h + 1 < XW_OC ? h + 1 : 0;
            }
        }
        if (oc.n + (uint32_t)__popcll(__ballot(miss)) > XW_OC) xw_cache_flush(st, oc, ocnw, lane);
    }
    int osr = -1;
    if (valid && origin != SF_ORIGIN_NONE) {
        uint32_t h = (uint32_t)(mix64(origin) % XW_OC);
        for (;;) {
            const unsigned int prev = atomicCAS(&oc.key[h], 0u, origin + 1u);
            if (prev == 0u) {                                  // new in the cache: load it
                atomicAdd(&oc.n, 1u);
                const uint32_t ko = aux_get(st, l, AX_ORIGIN, origin);
                oc.ko[h] = ko;
                if (ko != XNONE) nw_load(xw_node(ocnw, h), st, aux_rows(st, ko));
                break;
            }
            if (prev == origin + 1u) break;
            h = h + 1 < XW_OC ? h + 1 : 0;
        }
        osr = (int)h + 1;
    }
    XS_PF(0)
    xs.os[lane] = osr;
    __syncthreads();
    uint64_t sm = 0;                                           // earlier lanes of the same origin
    if (osr >= 0)
        for (int q = 0; q < 64; q++)
            if (xs.os[q] == osr) sm |= 1ull << q;
    sm &= (1ull << lane) - 1ull;
    XS_PF(1)
    // node bases (the first lane of each origin) and the rules' constants
    if (osr >= 0 && sm == 0) {
        const uint32_t ko = oc.ko[osr - 1];
        xs.ko[osr] = ko;
        long long b = 0, th = 0;
        if (ko != XNONE) {
            NodeWin<2> x = xw_node(ocnw, osr - 1);
            b = x.sec_sum_pass(t0);
            th = x.threads;
        }
        xs.base[osr] = b; xs.thr[osr] = th;
    }
    if (lane == 0) {
        NodeWin<2> x = snap;
        xs.base[0] = x.sec_sum_pass(t0);
        xs.thr[0] = x.threads;
        // (the previous second's QPS: read only at a second's first sync -- it is
        // a minute-bucket load from HBM)
        int64_t prevq = 0;
        bool have_prevq = false;
        for (uint32_t k = r0; k < r1; k++) {
            const DevRule& r = st.rules[k];
            XwRuleC& q = xs.rc[k - r0];
            q.rs = st.rstate[k];
            q.sync = 0;
            q.thr = r.count; q.qps = r.count;
            if (r.kind == CT_WARM_UP || r.kind == CT_WARM_UP_RATE_LIMITER) {
                if (r.limit_app == SF_APP_DEFAULT && q.rs.last_filled < t0 - t0 % 1000) {
                    if (!have_prevq) { prevq = j_d2l(x.previous_pass_qps(t0)); have_prevq = true; }
                    warm_sync(r, q.rs, t0, prevq);           // (the ClusterNode's previous second)
                    q.sync = 1;
                }
                const int64_t rest = q.rs.stored_tokens;
                if (rest >= r.warning_token) {
                    const int64_t above = rest - r.warning_token;
                    const double wq = j_next_up(1.0 / ((double)above * r.slope + 1.0 / r.count));
                    q.thr = wq; q.qps = wq;
                }
            }
            q.lstart = q.rs.latest_passed;
        }
    }
    __syncthreads();
    XS_PF(2)
    const double isec = st.interval / 1000.0;
    uint8_t sel[MAX_RULES];                                    // 0 none, 1 ClusterNode, 2 origin node
    long long cost[MAX_RULES];
    for (uint32_t kr = 0; kr < (uint32_t)MAX_RULES; kr++) {
        sel[kr] = 0; cost[kr] = -1;
        if (kr >= nrules) continue;
        const DevRule& r = st.rules[r0 + kr];
        if (is_solve && !r.always_pass) {
            const int s_ = xflow_select(st, r, r0, r1, origin, 0u);
            if (s_ == XS_CLUSTER) sel[kr] = 1;
            else if (s_ == XS_ORIGIN && osr >= 0 && xs.ko[osr] != XNONE) sel[kr] = 2;
        }
        if (r.kind == CT_RATE_LIMITER) {
            if (c > 0 && r.count > 0) cost[kr] = j_round(1.0 * c / r.count * 1000);
        } else if (r.kind == CT_WARM_UP_RATE_LIMITER) {
            cost[kr] = j_round(1.0 * c / xs.rc[kr].qps * 1000);
        }
    }
    // an exit's liveness: its entry passed (in this chunk: that lane's verdict,
    // eidx; before it: live_pre, from the walk's exit descriptor)
    XS_PF(3)
    int d = is_solve ? 1 : 0, ri = 0;
    uint32_t reach = 0, passk = 0;
    long long w = 0;
    for (int it = 0; it < 72; it++) {
        const int ed = __shfl(d, eidx >= 0 ? eidx : (int)lane);
        const bool live = is_exit && (eidx >= 0 ? ed != 0 : live_pre);
        const long long pc = (is_solve && d) ? (long long)c : 0;
        const long long td = ((is_solve && d) ? 1 : 0) - (live ? 1 : 0);
        const long long Pc = xw_excl_scan(pc, lane), Tc = xw_excl_scan(td, lane);
        xs.cm[lane] = pc; xs.td[lane] = td;
        __syncthreads();
        long long Po = 0, To = 0;
        for (uint64_t m = sm; m; m &= m - 1) {
            const int q = __ffsll((long long)m) - 1;
            Po += xs.cm[q]; To += xs.td[q];
        }
        __syncthreads();
        int nd = is_solve ? 1 : 0, nri = 0;
        uint32_t nreach = 0, npass = 0;
        long long nw = 0;
        for (uint32_t kr = 0; kr < nrules; kr++) {
            const DevRule& r = st.rules[r0 + kr];
            const bool rlk = r.kind == CT_RATE_LIMITER || r.kind == CT_WARM_UP_RATE_LIMITER;
            long long lat = 0;
            if (rlk) {                                         // latestPassedTime before this lane
                long long a = 0, b = XW_MPNEG;
                if (((passk >> kr) & 1u) && cost[kr] >= 0) { a = cost[kr]; b = t; }
                xw_mp_scan(a, b, lane);
                long long ea = __shfl_up(a, 1), eb = __shfl_up(b, 1);
                if (lane == 0) { ea = 0; eb = XW_MPNEG; }
                lat = max(xs.rc[kr].lstart + ea, eb);
            }
            if (!nd || !sel[kr]) continue;
            nreach |= 1u << kr;
            const bool on_c = sel[kr] == 1;
            const long long base = on_c ? xs.base[0] : xs.base[osr];
            const long long P = on_c ? Pc : Po;
            const long long T = on_c ? xs.thr[0] + Tc : xs.thr[osr] + To;
            bool ok = true;
            long long ww = 0;
            if (r.kind == CT_DEFAULT) {                        // DefaultController.canPass (prio excluded)
                const int32_t cur = r.grade == SF_GRADE_THREAD ? (int32_t)T : j_d2i((double)(base + P) / isec);
                ok = !((double)(int32_t)((uint32_t)cur + (uint32_t)c) > r.count);
            } else if (r.kind == CT_WARM_UP) {                 // WarmUpController.canPass
                const int64_t pq = j_d2l((double)(base + P) / isec);
                ok = (double)(pq + c) <= xs.rc[kr].thr;
            } else if (r.kind == CT_RATE_LIMITER && c <= 0) {
                ok = true;
            } else if (r.kind == CT_RATE_LIMITER && r.count <= 0) {
                ok = false;
            } else {                                           // RateLimiter / WarmUpRateLimiter
                const long long expected = cost[kr] + lat;
                if (expected > t) {
                    ww = expected - t;
                    ok = ww <= r.max_queue_ms;
                    if (!ok) ww = 0;
                }
            }
            if (!ok) { nd = 0; nri = (int)kr; }
            else { npass |= 1u << kr; nw += ww; }
        }
        const bool changed = nd != d || nreach != reach || npass != passk || nw != w || nri != ri;
        d = nd; reach = nreach; passk = npass; w = nw; ri = nri;
        if (lane == 0 && st.xw_stats) atomicAdd(&st.xw_stats[2], 1ull);
        if (!__ballot(changed)) break;
    }
    XS_PF(4)
    // the rules' state after the chunk (lane 0 writes)
    for (uint32_t kr = 0; kr < nrules; kr++) {
        const DevRule& r = st.rules[r0 + kr];
        const bool rlk = r.kind == CT_RATE_LIMITER || r.kind == CT_WARM_UP_RATE_LIMITER;
        const bool any_reach = __ballot((reach >> kr) & 1u) != 0ull;
        bool any_pass = false;
        long long fin = 0;
        if (rlk) {
            long long a = 0, b = XW_MPNEG;
            const bool el = ((passk >> kr) & 1u) && cost[kr] >= 0;
            if (el) { a = cost[kr]; b = t; }
            any_pass = __ballot(el) != 0ull;
            xw_mp_scan(a, b, lane);
            a = __shfl(a, 63); b = __shfl(b, 63);
            fin = max(xs.rc[kr].lstart + a, b);
        }
        if (lane == 0 && ((xs.rc[kr].sync && any_reach) || any_pass)) {
            DevRuleState rs = st.rstate[r0 + kr];
            if (xs.rc[kr].sync && any_reach) { rs.stored_tokens = xs.rc[kr].rs.stored_tokens; rs.last_filled = xs.rc[kr].rs.last_filled; }
            if (any_pass) rs.latest_passed = fin;
            st.rstate[r0 + kr] = rs;
        }
    }
    XS_PF(5)
    if (is_solve) {
        *myc = d ? XWC_PASS : XWC_BLOCK;
        *mst = d ? (uint8_t)(w > 0 ? SF_V_PASS_WAIT : SF_V_PASS) : (uint8_t)SF_V_BLOCK_FLOW;
        *mrule = d ? 0 : ri;
        *mwait = w;
    } else if (is_sys) {
        *myc = XWC_BLOCK; *mst = sysblk_status(fl); *mrule = sysblk_rule(fl); *mwait = 0;
    } else if (is_exit) {
        *myc = XWC_EXIT;
    }
    {   // the exits' final liveness, for the accounting
        const int ed = __shfl(d, eidx >= 0 ? eidx : (int)lane);
        *x_live = is_exit && (eidx >= 0 ? ed != 0 : live_pre);
    }
    *my_row = osr;
}

// One chunk's event fields, loaded a chunk ahead: the walk is a chain of
// dependent chunks, so HBM latency, not bandwidth, is its cost.  First level
// (sorted position j): time, flags, count, submission index, entry ref;
// second level (addresses from the first): the origin, and an exit's entry
// flags / time and -- when the entry was decided before the chunk that issues
// the loads (jd) -- its status; create time of an exit whose entry is older.
// k_gather_exit leaves a ref >= 0 only inside the exit's own segment.
struct XwEv {
    int64_t t, ref, rts, cts;
    int32_t c;
    uint32_t i, origin;
    uint8_t fl, rfl, rvs, pad;
};
__device__ __forceinline__ void xw_ld1(const SegIO& io, uint32_t j, uint32_t hi, XwEv& e) {
    if (j < hi) {
        const uint32_t m = ev_word(io, j);
        e.t = ev_time(io, m, j); e.fl = ev_flags(m); e.c = ev_count(io, m, j); e.i = io.perm[j];
        e.ref = io.eref ? io.eref[j] : -1;
    } else {
        e.t = INT64_MAX; e.fl = 0; e.c = 0; e.i = 0; e.ref = -1;
    }
}
__device__ __forceinline__ void xw_ld2(const SegIO& io, uint32_t j, uint32_t lo, uint32_t hi, uint32_t jd, XwEv& e) {
    e.origin = SF_ORIGIN_NONE; e.rfl = 0; e.rvs = 0; e.rts = 0; e.cts = 0;
    if (j >= hi) return;
    if (io.ev_origin) e.origin = io.ev_origin[e.i];
    if (e.fl & SF_EV_EXIT) {
        if (e.ref >= (int64_t)lo && e.ref < (int64_t)j) {
            const uint32_t mr = ev_word(io, (uint32_t)e.ref);
            e.rfl = ev_flags(mr); e.rts = ev_time(io, mr, (uint32_t)e.ref);
            if (e.ref < (int64_t)jd) e.rvs = io.v_status[e.ref];
        } else if (e.ref < 0 && io.cts) {
            e.cts = io.cts[j];
        }
    }
}
// the o_wait / o_rule half of emit_verdict with the submission index at hand
__device__ __forceinline__ void xw_emit(const SegIO& io, uint32_t i, int32_t wait, uint16_t rule) {
    if (!io.perm) return;
    if (io.o_wait && wait) io.o_wait[i] = wait;
    if (io.o_rule && rule) io.o_rule[i] = rule;
}

template <int MAXS>
__global__ void __launch_bounds__(64) k_decide_xw(DevState st, SegIO io, const uint32_t* seg_start,
                                                  const uint32_t* seg_res, const uint32_t* list,
                                                  const uint32_t* n_list) {
    ev_open(io.ev);
    __shared__ __align__(16) unsigned char snap_raw[sizeof(NodeWin<MAXS>)];
    __shared__ uint8_t cls[64];
    __shared__ uint8_t vch[64];                             // the previous chunk's final statuses
#ifdef SF_XW_PROFILE
    __shared__ unsigned long long pfs[8];
#else
    unsigned long long* pfs = nullptr;
#endif
    __shared__ XwRow rows[XW_KCAP];
    __shared__ XwScratch xs;
    __shared__ XwCache oc;
    __shared__ __align__(16) unsigned char ocnw[MAXS == 2 ? XW_OC * sizeof(NodeWin<2>) : 16];
    NodeWin<MAXS>& snap = *reinterpret_cast<NodeWin<MAXS>*>(snap_raw);
    const uint32_t lane = threadIdx.x;
    const ParamTable pt{st.ptab, st.pcap_mask, st.err, st.pins};
    const uint32_t nl = *n_list;
    for (uint32_t q = blockIdx.x; q < nl; q += gridDim.x) {
        const uint32_t s = list[q];
        const uint32_t lo = seg_start[s], hi = seg_start[s + 1], l = seg_res[s];
        const uint32_t r0 = st.rule_off[l], r1 = st.rule_off[l + 1];
        const bool thr_sens = (st.xw[l] & XWF_THREAD) != 0;
        // the ClusterNode lives in LDS (lane 0 updates it, every lane reads it):
        // no registers held across the chunk loop for it
        NodeWin<MAXS>& cn = snap;
        uint32_t cl = XNONE;
        if (lane == 0) { nw_load(cn, st, cluster_rows(st, l)); cl = l; }
        for (uint32_t k = lane; k < XW_OC; k += 64) oc.key[k] = 0;
        if (lane == 0) oc.n = 0;
        XwEv e;
        xw_ld1(io, lo + lane, hi, e);
        xw_ld2(io, lo + lane, lo, hi, lo, e);
        uint32_t jprev = lo;                               // start of the previous chunk (vch)
        __syncthreads();
#ifdef SF_XW_PROFILE
        unsigned long long pf_setup = 0, pf_solve = 0, pf_post = 0, pf_n = 0, pf_t = 0, pf_p[6] = {0, 0, 0, 0, 0, 0};
        if (lane < 8) pfs[lane] = 0;
#define XW_PF(k) { const unsigned long long x_ = wall_clock64(); pf_p[k] += x_ - pf_t; pf_t = x_; pf_post += 0; }
#else
#define XW_PF(k)
#endif
        for (uint32_t j0 = lo; j0 < hi;) {
#ifdef SF_XW_PROFILE
            pf_t = wall_clock64(); pf_n++;
#endif
            const int64_t t0 = __shfl(e.t, 0);
            const int64_t bs = t0 - t0 % st.wl, bm = t0 - t0 % 1000;
            const uint32_t j = j0 + lane;
            const bool valid = j < hi;
            const int64_t t = valid ? e.t : t0;
            const bool same = valid && t >= bs && t < bs + st.wl && t >= bm && t < bm + 1000;
            const unsigned long long nb = __ballot(!same);
            const uint32_t L = nb ? (uint32_t)(__ffsll((long long)nb) - 1) : 64u;   // (lane 0 is always in)
            const uint32_t jn = j0 + L;
            // the next chunk's first-level fields, in flight while this one is decided
            XwEv nx;
            xw_ld1(io, jn + lane, hi, nx);
            for (uint32_t k = lane; k < XW_KCAP; k += 64) {
                rows[k].blk = rows[k].succ = rows[k].rt = rows[k].exc = rows[k].pass = 0; rows[k].thr = 0;
                rows[k].minrt = INT64_MAX;
                rows[k].nblk = rows[k].ncmp = rows[k].nexc = rows[k].npass = 0; rows[k].key = 0;
            }
            // 1. classify
            uint8_t myc = 0, mst = 0;
            int mrule = 0;
            int64_t mwait = 0;
            const bool act = lane < L;
            const uint32_t origin = act ? e.origin : SF_ORIGIN_NONE;
            const int32_t c = act ? e.c : 0;
            const uint8_t fl = act ? e.fl : 0;
            // an exit's entry: in this chunk (eidx: that lane's verdict), or decided
            // before it (live_pre), or before this batch (ref < 0)
            int eidx = -1;
            bool live_pre = false;
            int64_t xcts = t;
            if (act && (fl & SF_EV_EXIT)) {
                const int64_t ref = e.ref;
                if (ref >= 0) {
                    if (ref < (int64_t)lo || ref >= (int64_t)j || (e.rfl & SF_EV_EXIT)) {
                        *st.err = SF_ERR_INVALID;                  // (an exit of itself: blocked)
                    } else {
                        xcts = e.rts;
                        if (ref >= (int64_t)j0) eidx = (int)(ref - j0);
                        else live_pre = !v_blocked(ref >= (int64_t)jprev ? vch[ref - jprev] : e.rvs);
                    }
                } else {
                    live_pre = ref != EREF_DEAD;
                    xcts = io.cts ? e.cts : t;
                }
            }
            // the exact chunk solve (below) unless a prioritized entry is in the chunk
            // (its occupy path) or an origin-node WarmUp rule has not synced this second
            bool jac = false;
            if constexpr (MAXS == 2) {
                jac = __ballot(act && !(fl & (SF_EV_EXIT | EVF_SYSBLK)) && (fl & SF_EV_PRIO)) == 0ull;
                for (uint32_t k = r0; k < r1 && jac; k++) {
                    const DevRule& r = st.rules[k];
                    if ((r.kind == CT_WARM_UP || r.kind == CT_WARM_UP_RATE_LIMITER) && r.limit_app != SF_APP_DEFAULT &&
                        st.rstate[k].last_filled < t0 - t0 % 1000)
                        jac = false;
                }
            }
            if constexpr (MAXS == 2) {
                if (!jac && oc.n) xw_cache_flush(st, oc, ocnw, lane);   // (the serial walk reads HBM)
            }
            if (lane == 0) {
                if (cl != l) { if (cl != XNONE) nw_store(cn, st, cluster_rows(st, cl)); nw_load(cn, st, cluster_rows(st, l)); cl = l; }
                cn.min_flush();                              // (a copy that moves to another minute slot reads HBM)
            }
            __syncthreads();
            int my_row = -1;
            bool x_live = false;
#ifdef SF_XW_PROFILE
            { const unsigned long long x = wall_clock64(); pf_setup += x - pf_t; pf_t = x; }
#endif
            if (jac) {
                if constexpr (MAXS == 2)
                    xw_solve_chunk(st, snap, rows, xs, oc, ocnw, lane, L, t0, t, fl, c, origin, eidx, live_pre, l,
                                   r0, r1, &myc, &mst, &mrule, &mwait, &my_row, &x_live, pfs);
            } else {
                if (act) {
                    if (fl & SF_EV_EXIT) myc = thr_sens ? XWC_SERIAL : XWC_EXIT;
                    else if (fl & EVF_SYSBLK) { myc = XWC_BLOCK; mst = sysblk_status(fl); mrule = sysblk_rule(fl); }
                    else myc = XWC_SERIAL;
                }
                const unsigned long long exits = __ballot(act && (fl & SF_EV_EXIT));
                const int64_t ex_before = (int64_t)__popcll(exits & ((1ull << lane) - 1ull));
                if (myc == XWC_SERIAL && !(fl & (SF_EV_EXIT | SF_EV_PRIO))) {
                    for (uint32_t k = r0; k < r1; k++) {
                        const DevRule& r = st.rules[k];
                        if (r.always_pass) continue;
                        const int sel = xflow_select(st, r, r0, r1, origin, 0u);
                        if (sel == XS_NONE) continue;
                        DevRuleState rs = st.rstate[k];
                        int64_t w = 0; bool pw = false; int ok = 1;
                        if (sel == XS_CLUSTER) {
                            NodeWin<MAXS> x = snap;                  // (minute bucket clean: never written back)
                            x.threads -= ex_before;
                            ok = can_pass<MAXS>(r, rs, x, t, c, false, st.occupy_timeout, &w, &pw);
                        } else if (sel == XS_ORIGIN) {
                            // a WarmUp rule shared by several origin nodes (`other`) syncs its
                            // tokens at the second's first check, with THAT event's origin's
                            // previous QPS: until the walk has synced this second, its entries
                            // stay in the serial part
                            const bool warm = r.kind == CT_WARM_UP || r.kind == CT_WARM_UP_RATE_LIMITER;
                            if (warm && rs.last_filled < t - t % 1000) break;
                            const uint32_t ko = aux_get(st, l, AX_ORIGIN, origin);
                            if (ko != XNONE) {
                                NodeWin<MAXS> x;
                                nw_load(x, st, aux_rows(st, ko));
                                x.threads -= ex_before;
                                ok = can_pass<MAXS>(r, rs, x, t, c, false, st.occupy_timeout, &w, &pw);
                            }
                        }
                        if (!ok) { myc = XWC_BLOCK; mst = SF_V_BLOCK_FLOW; mrule = (int)(k - r0); }
                        break;                                   // only the first selecting rule decides here
                    }
                }
            }
#ifdef SF_XW_PROFILE
            { const unsigned long long x = wall_clock64(); pf_solve += x - pf_t; pf_t = x; }
#endif
            // the next chunk's second-level fields (its entries decided before this
            // chunk are final; those in this chunk come from vch below)
            xw_ld2(io, jn + lane, lo, hi, j0, nx);
            if (act) cls[lane] = myc;
            if (myc == XWC_BLOCK || myc == XWC_PASS) io.v_status[j] = mst;   // (before the walk: its exits read it)
            __syncthreads();
            XW_PF(0)
            // 2. the serial walk over the undecided events (entered only when there
            // are some: the walk's calls save and restore the live registers)
            const unsigned long long nser = __popcll(__ballot(act && myc == XWC_SERIAL));
            if (nser) {
                if (lane == 0) {
                    NodeWin<MAXS> on, dn;                    // (origin / context node of the walk)
                    uint32_t oi = XNONE, di = XNONE;
                    for (uint32_t k = 0; k < L; k++)
                        if (cls[k] == XWC_SERIAL) xg_event<MAXS>(st, io, pt, lo, j0 + k, cn, on, dn, cl, oi, di);
                    if (oi != XNONE) nw_store(on, st, aux_rows(st, oi));
                    if (di != XNONE) nw_store(dn, st, aux_rows(st, di));
                }
                __syncthreads();
            }
            if (lane == 0 && st.xw_stats) {
                atomicAdd(&st.xw_stats[jac ? 0 : 1], 1ull);
                if (nser) atomicAdd(&st.xw_stats[3], nser);
            }
            XW_PF(1)
            // 3. the blocks and completions, summed per node
            int64_t blk = 0, succ = 0, rt = 0, exc = 0, thr = 0, minrt = INT64_MAX;
            int nblk = 0, ncmp = 0, nexc = 0;
            int64_t pss = 0;
            int npss = 0;
            uint8_t vfin = mst;                                  // this lane's final status (vch)
            if (myc == XWC_BLOCK) {
                xw_emit(io, e.i, (int32_t)mwait, (uint16_t)mrule);
                blk = c; nblk = 1;
            } else if (myc == XWC_PASS) {
                xw_emit(io, e.i, (int32_t)mwait, 0);
                pss = c; npss = 1;
            } else if (myc == XWC_EXIT) {                    // StatisticSlot.exit :134-165
                // (liveness from the solve; on the serial path an entry of this
                // chunk has its status in v_status by now)
                const bool live = jac ? x_live
                                      : (eidx >= 0 ? !v_blocked(io.v_status[j0 + eidx]) : live_pre);
                uint8_t v = SF_V_EXIT_IGNORED;
                if (live) {
                    v = SF_V_EXIT;
                    succ = c; rt = t - xcts; minrt = rt; thr = -1; ncmp = 1;
                    if (fl & SF_EV_ERROR) { exc = c; nexc = 1; }
                }
                io.v_status[j] = v;
                vfin = v;
            } else if (myc == XWC_SERIAL) {
                vfin = io.v_status[j];                       // (lane 0's walk wrote it)
            }
            // the ClusterNode's sums: wavefront reductions (every lane adds to it)
            XwRow crow;
            {
                long long v[6] = {blk, succ, rt, exc, thr, pss};
#pragma unroll
                for (int f = 0; f < 6; f++) v[f] = xw_wsum(v[f]);
                const long long mr = xw_wmin(minrt);
                crow.blk = (unsigned long long)v[0]; crow.succ = (unsigned long long)v[1];
                crow.rt = (unsigned long long)v[2]; crow.exc = (unsigned long long)v[3];
                crow.thr = v[4] + (long long)__popcll(__ballot(npss != 0)); crow.pass = (unsigned long long)v[5];
                crow.minrt = mr;
                crow.nblk = (unsigned)__popcll(__ballot(nblk != 0)); crow.ncmp = (unsigned)__popcll(__ballot(ncmp != 0));
                crow.nexc = (unsigned)__popcll(__ballot(nexc != 0)); crow.npass = (unsigned)__popcll(__ballot(npss != 0));
            }
            XW_PF(2)
            if (nblk || ncmp || npss) {
                if (jac) {
                    if (my_row > 0) xw_add(rows[my_row], blk, nblk, succ, rt, minrt, exc, nexc, thr, ncmp, pss, npss);
                } else if (origin != SF_ORIGIN_NONE) {
                    uint32_t h = 1 + (uint32_t)(mix64(origin) % (XW_KCAP - 1));
                    for (;;) {
                        const unsigned int prev = atomicCAS(&rows[h].key, 0u, origin + 1u);
                        if (prev == 0u || prev == origin + 1u) break;
                        h = h + 1 < XW_KCAP ? h + 1 : 1;
                    }
                    xw_add(rows[h], blk, nblk, succ, rt, minrt, exc, nexc, thr, ncmp, pss, npss);
                }
            }
            __syncthreads();
            XW_PF(3)
            if (lane == 0) xw_apply<MAXS>(cn, crow, t0);
            if constexpr (MAXS == 2) {
                if (jac) {                                       // into the cached origin nodes
                    for (uint32_t k = 1 + lane; k < XW_KCAP; k += 64)
                        if ((rows[k].nblk | rows[k].ncmp | rows[k].npass | rows[k].nexc) && oc.ko[k - 1] != XNONE)
                            xw_apply<2>(xw_node(ocnw, k - 1), rows[k], t0);
                }
            }
            for (uint32_t k = 1 + lane; k < XW_KCAP && !jac; k += 64) {
                if (!rows[k].key) continue;
                const uint32_t ko = aux_get(st, l, AX_ORIGIN, rows[k].key - 1u);
                if (ko == XNONE) continue;
                NodeWin<MAXS> x;
                const NodeRows nr = aux_rows(st, ko);
                nw_load(x, st, nr);
                xw_apply<MAXS>(x, rows[k], t0);
                nw_store(x, st, nr);
            }
            XW_PF(4)
            // the next chunk: its exits of entries in this chunk read vch
            if (act) vch[lane] = vfin;
            __syncthreads();
            jprev = j0;
            e = nx;
            XW_PF(5)
            j0 = jn;
        }
#ifdef SF_XW_PROFILE
        if (lane == 0 && hi - lo > 20000)
            printf("xw seg n=%u chunks=%llu setup=%llu solve=%llu (%llu %llu %llu %llu %llu %llu) post %llu %llu %llu %llu %llu %llu (x10ns)\n", hi - lo,
                   pf_n, pf_setup, pf_solve, pfs[0], pfs[1], pfs[2], pfs[3], pfs[4], pfs[5], pf_p[0], pf_p[1], pf_p[2], pf_p[3], pf_p[4], pf_p[5]);
#endif
        if constexpr (MAXS == 2) xw_cache_flush(st, oc, ocnw, lane);
        if (lane == 0 && cl != XNONE) nw_store(cn, st, cluster_rows(st, cl));
        __syncthreads();
    }
}

// the wave walk of a batch of n events over Work::xw_list (k_classify)
void launch_xw(const DevState& st, const SegIO& io, const Work& w, uint32_t n, hipStream_t s) {
    const unsigned g = (unsigned)std::min<size_t>((size_t)n / XW_MIN + 1, 2048);
    for_sample_count(st, [&](auto S) {
        hipLaunchKernelGGL(k_decide_xw<decltype(S)::value>, dim3(g), dim3(64), 0, s, st, io, w.seg_start, w.seg_res,
                           w.xw_list, w.counters + WC_XW_LIST);
    });
}

}  // namespace sf
