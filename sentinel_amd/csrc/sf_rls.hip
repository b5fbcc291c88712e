// sf_rls.hip — gfx950 kernels of one sf_request_rls (product code): a batch of
// Envoy RateLimitRequests decided as SentinelEnvoyRlsServiceImpl.shouldRateLimit
// would decide them one by one, descriptor by descriptor (sf_rls.h).
//
//   k_rls_check     the offset tables are non-decreasing, every string index
//                   is < n_str, no time is negative (else *err =
//                   SF_ERR_INVALID: nothing is decided)
//   k_rls_domain    string form: key state (hash, blank, well-formed) after
//                   the domain, one lane per request
//   k_rls_keys      string form: one lane per descriptor continues from its
//                   request's domain state over its entries -> flowId
//   k_rls_prep      flowId -> flow rule index (the token server's id table);
//                   error and no-rule descriptors get their final outputs
//   sort            tok_sort_segments (sf_token.hip): descriptors grouped per
//                   rule, batch order kept inside a rule
//   k_rls_route     segments of >= wave_min descriptors are listed for the wave
//                   route
//   k_rls_lane      one lane per short segment replays SimpleClusterFlowChecker
//                   on the rule's ClusterMetric staged in LDS
//   k_rls_wave      one wavefront per long segment: chunks of <= 64 descriptors
//                   of one bucket window, verdicts by fixed-point iteration
//   k_rls_fold      overall code of each request
//
// Wave route.  Inside one bucket window the sum of the metric's other buckets
// is constant (as for the namespace limiter, sf_token.hip), so descriptor l of
// a chunk passes iff  thr - (sum0 + P_l) / isec - c_l >= 0  where P_l is the
// sum of the counts of the chunk's passing descriptors before l.  Start from
// "all pass", re-evaluate every lane with the prefix of the current guess
// (a wave scan), repeat until no lane changes.  After round k the first k
// lanes hold their serial verdicts (lane l depends on lanes < l only), so the
// fixed point is the serial result and at most RLS_CHUNK + 1 rounds are run.
// sum0 + P_l is Java's wrapping long sum whatever the order of the additions
// (addition modulo 2^64 is associative), so no overflow case is left out.
// A chunk whose window is older than its bucket (currentWindow's throwaway
// bucket) is replayed by lane 0 with the lane route's code.
#include <algorithm>

#include "sf_rls.h"

namespace sf {

static inline unsigned rblocks(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

// adds popcount(flag over the wavefront) to *ctr with one atomic
__device__ __forceinline__ void rls_count(unsigned long long* ctr, bool flag) {
    const unsigned long long m = __ballot(flag);
    if (m && (int)(threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicAdd(ctr, (unsigned long long)__popcll(m));
}

__global__ void k_rls_check(RlsBatch b, int32_t* err) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < b.n) bad |= b.desc_off[i] > b.desc_off[i + 1] || b.ts[i] < 0;
    if (i == 0) bad |= b.desc_off[0] != 0;
    if (!b.desc_fid) {
        if (i < b.n) bad |= b.domain[i] >= b.n_str;
        if (i < b.n_desc) bad |= b.ent_off[i] > b.ent_off[i + 1];
        if (i < b.n_ent) bad |= b.ent_key[i] >= b.n_str || b.ent_val[i] >= b.n_str;
        if (i < b.n_str) bad |= b.str_off[i] > b.str_off[i + 1];
    }
    if (bad) *err = SF_ERR_INVALID;
}

// the lengths of a device-memory batch's tables (their last offsets), gathered for one copy
__global__ void k_rls_lengths(RlsBatch b, uint32_t* out) {
    const uint32_t nd = b.desc_off[b.n];
    out[0] = nd;
    out[1] = b.desc_fid ? 0 : b.ent_off[nd];
    out[2] = b.desc_fid ? 0 : b.str_off[b.n_str];
}
hipError_t rls_lengths(const RlsBatch& b, uint32_t* d_out, hipStream_t s) {
    hipLaunchKernelGGL(k_rls_lengths, dim3(1), dim3(1), 0, s, b, d_out);
    return hipGetLastError();
}

__device__ __forceinline__ void rls_feed_str(const RlsBatch& b, RlsKey& k, uint32_t s) {
    const uint32_t lo = b.str_off[s];
    rls_key_feed(k, b.bytes + lo, b.str_off[s + 1] - lo);
}

__global__ void k_rls_domain(RlsBatch b, RlsWork rw, const int32_t* err) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.n || *err) return;
    RlsKey k = rls_key_begin();
    rls_feed_str(b, k, b.domain[i]);
    rw.dom[i] = k;
    rw.req_err[i] = !k.ok;
}

// request of descriptor d: the i with desc_off[i] <= d < desc_off[i + 1]
__device__ __forceinline__ uint32_t rls_req_of(const RlsBatch& b, uint32_t d) {
    uint32_t lo = 0, hi = b.n - 1;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (b.desc_off[mid + 1] <= d) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ void k_rls_keys(RlsBatch b, RlsWork rw, const int32_t* err) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= b.n_desc || *err) return;
    const uint32_t req = rls_req_of(b, d);
    rw.d_req[d] = req;
    RlsKey k = rw.dom[req];
    const uint32_t e1 = b.ent_off[d + 1];
    for (uint32_t e = b.ent_off[d]; e < e1 && k.ok; e++) {       // generateKey :111-117
        rls_key_cp(k, '|');
        rls_feed_str(b, k, b.ent_key[e]);
        if (!k.ok) break;
        rls_key_cp(k, '|');
        rls_feed_str(b, k, b.ent_val[e]);
    }
    if (!k.ok) rw.req_err[req] = 1;                              // (every writer stores 1)
    rw.d_fid[d] = k.ok ? rls_key_id(k) : -1;
}

__global__ void k_rls_prep(TokState ts, RlsBatch b, TokWork w, RlsWork rw, RlsOut out) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= b.n_desc || *ts.err) return;
    uint32_t req;
    if (b.desc_fid) { req = rls_req_of(b, d); rw.d_req[d] = req; }
    else req = rw.d_req[d];
    const int32_t hits = b.hits[req];
    const bool error = hits < 0 || (!b.desc_fid && rw.req_err[req]);      // onError :36-40: nothing is checked
    int64_t id = -1;
    uint64_t key = KEY_NONE;
    bool no_rule = false;
    if (error) {
        out.code[d] = SF_RLS_UNKNOWN;
        if (out.limit) out.limit[d] = SF_RLS_NO_LIMIT;
        if (out.remaining) out.remaining[d] = 0;
    } else {
        id = b.desc_fid ? b.desc_fid[d] : rw.d_fid[d];
        const int32_t r = id > 0 ? id_lookup(ts, id, false) : -1;         // getFlowRuleById: flow rules only
        if (r < 0) {                                                      // NO_RULE_EXISTS becomes OK :55-58
            no_rule = true;
            out.code[d] = SF_RLS_OK;
            if (out.limit) out.limit[d] = SF_RLS_NO_LIMIT;
            if (out.remaining) out.remaining[d] = 0;
        } else {
            key = (uint32_t)r;
            rw.d_ts[d] = b.ts[req];
            rw.d_cnt[d] = hits == 0 ? 1 : hits;                           // :41-44
            if (out.limit) out.limit[d] = j_d2i(ts.rules[r].count);       // (int) rule.getCount() :70
        }
    }
    if (out.flow_id) out.flow_id[d] = id;
    w.key_in[d] = key;
    w.idx_in[d] = d;
    rls_count(&rw.ctr->no_rule, no_rule);
}

__global__ void k_rls_route(TokWork w, RlsWork rw, uint32_t wave_min, const int32_t* err) {
    const uint32_t sg = blockIdx.x * blockDim.x + threadIdx.x;
    if (*err || sg >= *w.n_seg) return;
    const bool wave = w.seg_start[sg + 1] - w.seg_start[sg] >= wave_min;
    if (wave) w.head[atomicAdd(&rw.ctr->n_wave, 1u)] = sg;       // (head is free once the segment table is built)
    rls_count(&rw.ctr->segs_wave, wave);
    rls_count(&rw.ctr->segs_lane, !wave);
}

__global__ void __launch_bounds__(RLS_LANE_T) k_rls_lane(TokState ts, TokWork w, RlsWork rw, RlsOut out,
                                                         uint32_t wave_min) {
    __shared__ ClFlowState lds[RLS_LANE_T];
    const uint32_t sg = blockIdx.x * blockDim.x + threadIdx.x;
    if (sg >= *w.n_seg) return;
    const uint32_t lo = w.seg_start[sg], hi = w.seg_start[sg + 1];
    if (hi - lo >= wave_min) return;
    const uint32_t r = (uint32_t)w.key_out[lo];
    const ClRule rule = ts.rules[r];
    ClFlowState* st = &lds[threadIdx.x];
    *st = ts.fstate[r];
    ClMetric m{st, rule.S, rule.wl, rule.interval, rule.interval / 1000.0};
    const double thr = rule.count * ts.exceed_count;
    for (uint32_t j = lo; j < hi; j++) {
        const uint32_t d = w.idx_out[j];
        uint8_t code; int32_t rem;
        rls_decide(m, thr, rw.d_ts[d], rw.d_cnt[d], &code, &rem);
        out.code[d] = code;
        if (out.remaining) out.remaining[d] = rem;
    }
    ts.fstate[r] = *st;
}

// inclusive prefix sum over the wavefront
__device__ __forceinline__ long long rls_scan(long long x, int lane) {
    for (int off = 1; off < 64; off <<= 1) {
        const long long v = __shfl_up(x, off);
        if (lane >= off) x += v;
    }
    return x;
}

__global__ void __launch_bounds__(RLS_CHUNK) k_rls_wave(TokState ts, TokWork w, RlsWork rw, RlsOut out) {
    __shared__ ClFlowState st;
    __shared__ int64_t sh_sum;
    __shared__ int sh_k;
    constexpr int WORDS = (int)(sizeof(ClFlowState) / sizeof(int64_t));
    const int lane = (int)threadIdx.x;
    const uint32_t sg = w.head[blockIdx.x];
    const uint32_t lo = w.seg_start[sg], hi = w.seg_start[sg + 1];
    const uint32_t r = (uint32_t)w.key_out[lo];
    const ClRule rule = ts.rules[r];
    for (int k = lane; k < WORDS; k += RLS_CHUNK) ((int64_t*)&st)[k] = ((const int64_t*)&ts.fstate[r])[k];
    __syncthreads();
    ClMetric m{&st, rule.S, rule.wl, rule.interval, rule.interval / 1000.0};
    const double thr = rule.count * ts.exceed_count;
    unsigned long long chunks = 0, serial = 0, rounds = 0;
    uint32_t p = lo;
    bool have = p + lane < hi;
    uint32_t d = have ? w.idx_out[p + lane] : 0;
    int64_t t = have ? rw.d_ts[d] : 0;
    int32_t c = have ? rw.d_cnt[d] : 0;
    while (p < hi) {
        // the next chunk, should this one be a whole one: its loads are in flight while this one is solved
        const bool have_n = p + RLS_CHUNK + lane < hi;
        const uint32_t d_n = have_n ? w.idx_out[p + RLS_CHUNK + lane] : 0;
        const int64_t t_n = have_n ? rw.d_ts[d_n] : 0;
        const int32_t c_n = have_n ? rw.d_cnt[d_n] : 0;
        // the chunk: the leading descriptors inside the bucket window of the first
        const int64_t t0 = __shfl(t, 0);
        const int64_t ws0 = t0 - t0 % rule.wl;
        const unsigned long long in = __ballot(have && t >= ws0 && t - ws0 < rule.wl);
        // lane 0 is inside its own window (times are >= 0, k_rls_check); never less than one, so p advances
        const int nch = max(~in ? __ffsll((long long)~in) - 1 : RLS_CHUNK, 1);
        const bool active = lane < nch;
        if (lane == 0) {
            sh_k = m.cur(t0);                                   // the roll, with transferOccupyToBucket
            sh_sum = m.sum(CE_PASS, t0);
        }
        __syncthreads();
        const int bk = sh_k;
        const int64_t sum0 = sh_sum;
        chunks++;
        if (bk < 0) {
            serial++;
            if (lane == 0) {
                for (uint32_t j = p; j < p + (uint32_t)nch; j++) {
                    const uint32_t dj = w.idx_out[j];
                    uint8_t code; int32_t rem;
                    rls_decide(m, thr, rw.d_ts[dj], rw.d_cnt[dj], &code, &rem);
                    out.code[dj] = code;
                    if (out.remaining) out.remaining[dj] = rem;
                }
            }
        } else {
            const long long cc = active ? c : 0;
            bool pass = active;
            long long incl = 0;
            double next = 0;
            for (int it = 0; it <= RLS_CHUNK; it++) {
                rounds++;
                incl = rls_scan(pass ? cc : 0, lane);
                const long long before = incl - (pass ? cc : 0);
                next = thr - (double)wadd(sum0, before) / m.isec - c;
                const bool np = active && next >= 0;
                const unsigned long long changed = __ballot(np != pass);
                pass = np;
                if (!changed) break;
            }
            if (active) {
                out.code[d] = pass ? SF_RLS_OK : SF_RLS_OVER_LIMIT;
                if (out.remaining) out.remaining[d] = pass ? j_d2i(next) : 0;
            }
            const long long pass_c = __shfl(incl, RLS_CHUNK - 1);
            const long long all_c = __shfl(rls_scan(cc, lane), RLS_CHUNK - 1);
            const int n_pass = __popcll(__ballot(pass));
            if (lane == 0) {
                ClBucket& b = st.b[bk];
                b.c[CE_PASS] = wadd(b.c[CE_PASS], pass_c);
                b.c[CE_PASS_REQUEST] = wadd(b.c[CE_PASS_REQUEST], n_pass);
                b.c[CE_BLOCK] = wadd(b.c[CE_BLOCK], all_c - pass_c);
                b.c[CE_BLOCK_REQUEST] = wadd(b.c[CE_BLOCK_REQUEST], nch - n_pass);
            }
        }
        __syncthreads();
        p += (uint32_t)nch;
        if (nch == RLS_CHUNK) {
            have = have_n; d = d_n; t = t_n; c = c_n;
        } else {
            have = p + lane < hi;
            d = have ? w.idx_out[p + lane] : 0;
            t = have ? rw.d_ts[d] : 0;
            c = have ? rw.d_cnt[d] : 0;
        }
    }
    for (int k = lane; k < WORDS; k += RLS_CHUNK) ((int64_t*)&ts.fstate[r])[k] = ((const int64_t*)&st)[k];
    if (lane == 0) {
        atomicAdd(&rw.ctr->chunks, chunks);
        atomicAdd(&rw.ctr->chunks_serial, serial);
        atomicAdd(&rw.ctr->rounds, rounds);
    }
}

__global__ void k_rls_fold(RlsBatch b, RlsWork rw, RlsOut out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.n) return;
    const bool error = b.hits[i] < 0 || (!b.desc_fid && rw.req_err[i]);
    bool blocked = false;
    if (!error)
        for (uint32_t d = b.desc_off[i]; d < b.desc_off[i + 1]; d++) blocked |= out.code[d] != SF_RLS_OK;
    out.overall[i] = error ? SF_RLS_ERROR : blocked ? SF_RLS_OVER_LIMIT : SF_RLS_OK;   // :77
    rls_count(&rw.ctr->error_requests, error);
}

hipError_t rls_launch(const TokState& ts, TokWork& w, const RlsWork& rw, const RlsBatch& b, const RlsOut& out,
                      uint32_t wave_min, hipStream_t s) {
    const unsigned T = RLS_T;
    hipError_t e = hipMemsetAsync(rw.ctr, 0, sizeof(RlsCounters), s);
    if (e != hipSuccess) return e;
    const bool strings = !b.desc_fid;
    const size_t most = strings ? std::max<size_t>({b.n, b.n_desc, b.n_ent, b.n_str}) : b.n;
    hipLaunchKernelGGL(k_rls_check, dim3(rblocks(most, T)), dim3(T), 0, s, b, ts.err);
    // the domain pass writes every request's error flag, which the fold reads: also without descriptors
    if (strings) hipLaunchKernelGGL(k_rls_domain, dim3(rblocks(b.n, T)), dim3(T), 0, s, b, rw, ts.err);
    if (b.n_desc) {
        if (strings) hipLaunchKernelGGL(k_rls_keys, dim3(rblocks(b.n_desc, T)), dim3(T), 0, s, b, rw, ts.err);
        hipLaunchKernelGGL(k_rls_prep, dim3(rblocks(b.n_desc, T)), dim3(T), 0, s, ts, b, w, rw, out);
        unsigned bits = 1;                      // rule indices are < 2^bits - 1: KEY_NONE's low bits sort last
        while ((ts.n_flow >> bits) != 0) bits++;
        e = tok_sort_segments(w, b.n_desc, bits, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_rls_route, dim3(rblocks(b.n_desc, T)), dim3(T), 0, s, w, rw, wave_min, ts.err);
    }
    int32_t err = 0;
    uint32_t n_seg = 0, n_wave = 0;
    if ((e = hipMemcpyAsync(&err, ts.err, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if (b.n_desc) {
        if ((e = hipMemcpyAsync(&n_seg, w.n_seg, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
        if ((e = hipMemcpyAsync(&n_wave, &rw.ctr->n_wave, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    }
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    if (err) return hipSuccess;                 // the caller reads *ts.err
    // kernels whose work is absent are not launched
    if (n_seg > n_wave)
        hipLaunchKernelGGL(k_rls_lane, dim3(rblocks(n_seg, RLS_LANE_T)), dim3(RLS_LANE_T), 0, s, ts, w, rw, out, wave_min);
    if (n_wave) hipLaunchKernelGGL(k_rls_wave, dim3(n_wave), dim3(RLS_CHUNK), 0, s, ts, w, rw, out);
    hipLaunchKernelGGL(k_rls_fold, dim3(rblocks(b.n, T)), dim3(T), 0, s, b, rw, out);
    return hipGetLastError();
}

}  // namespace sf
