// sf_token.h — device state and launch interface of the batched cluster
// token server (product code): DefaultTokenService.requestToken /
// requestParamToken for a time-ordered batch of requests.
//
// Reference (CS = sentinel-cluster/sentinel-cluster-server-default/src/main/java/com/alibaba/csp/sentinel/cluster):
//   DefaultTokenService          CS/flow/DefaultTokenService.java:39-72
//   ClusterFlowChecker           CS/flow/ClusterFlowChecker.java:38-112
//   ClusterParamFlowChecker      CS/flow/ClusterParamFlowChecker.java:42-120
//   ClusterMetric                CS/flow/statistic/metric/ClusterMetric.java:39-98
//   ClusterMetricLeapArray       CS/flow/statistic/metric/ClusterMetricLeapArray.java:34-92
//   ClusterParamMetric           CS/flow/statistic/metric/ClusterParamMetric.java:52-88
//   ClusterParameterLeapArray    CS/flow/statistic/metric/ClusterParameterLeapArray.java:39-49
//   GlobalRequestLimiter         CS/flow/statistic/limit/GlobalRequestLimiter.java:46-55
//   RequestLimiter               CS/flow/statistic/limit/RequestLimiter.java:51-87
//
// HBM layout:
//   rules   [n_flow + n_param]  ClRule: flow rules first, then param rules
//   fstate  [n_flow]            ClFlowState: the ClusterMetricLeapArray of one flowId
//   idtab   open-addressed      flow_id -> (flow rule index, param rule index)
//   ns / lim [n_ns]             namespace table and its RequestLimiter (UnaryLeapArray(10, 1000))
//   cptab   open-addressed      (param rule, value) -> per-value window counts
#pragma once
#include "sf_decide.h"
#include "sf_internal.h"

namespace sf {

constexpr int CL_MAXS = 16;                  // sampleCount of a cluster rule (ClusterFlowConfig, default 10)
constexpr int CE_PASS = 0, CE_BLOCK = 1, CE_PASS_REQUEST = 2, CE_BLOCK_REQUEST = 3, CE_OCCUPIED_PASS = 4,
              CE_OCCUPIED_BLOCK = 5, CE_WAITING = 6, CE_COUNT = 7;   // ClusterFlowEvent.java ordinals
constexpr int LIM_S = 10, LIM_WL = 100, LIM_INTERVAL = 1000;        // RequestLimiter: UnaryLeapArray(10, 1000)

struct ClRule {                  // 56 B
    double count;
    int64_t flow_id;
    int32_t threshold_type, ns;  // ns: namespace index, -1 when the namespace is not loaded
    int32_t S, wl;
    int32_t interval, is_param;
    uint32_t item_off, item_cnt;
    uint32_t owner, pad;         // shard deciding this rule's requests (sf_token_shard)
};
struct ClBucket { int64_t ws; int64_t c[CE_COUNT]; };          // WindowWrap<ClusterMetricBucket>, 64 B
struct ClFlowState {                                            // ClusterMetricLeapArray, 1056 B
    ClBucket b[CL_MAXS];
    int64_t occ_pass, occ_req;                                  // occupyCounter[PASS], [PASS_REQUEST]
    int64_t has_occ, pad;
};
struct ClNs { int32_t connected, has_limiter; double max_qps; };
struct LimState { int64_t ws[LIM_S]; int64_t v[LIM_S]; };
struct IdSlot { int64_t id; int32_t flow, param; };             // id == 0: empty (valid ids are > 0)
struct CpSlot {                  // (param rule, value): one value's column of ClusterParameterLeapArray
    uint64_t hi, lo;             // hi: (rule + 1) << 32 | tag, bit 63 while being claimed; 0 empty
    int64_t ws[CL_MAXS];         // window each count belongs to (WS_NONE: never)
    int64_t cnt[CL_MAXS];
};
constexpr uint64_t CP_CLAIM = 1ull << 63;
constexpr uint64_t KEY_NONE = ~0ull;          // sort key of a request that reached no checker (sorted last)

struct TokState {
    uint32_t n_flow, n_rules, n_ns;
    const ClRule* rules;
    ClFlowState* fstate;
    const IdSlot* idtab; uint64_t id_mask;
    const ClNs* ns; LimState* lim;
    CpSlot* cptab; uint64_t cp_mask;
    const DevHotItem* items;
    double exceed_count, max_occupy_ratio;
    int32_t* err;
    uint8_t* rmulti;             // [n_rules] per call: a param rule with a multi-value request (serial group)
    uint32_t shard_count, shard_index;
};

// flowId -> rule index of the flow (or param) rule table, -1: none (shared with sf_concur.hip)
SF_HD uint64_t id_hash(int64_t id) { return mix64((uint64_t)id * 0x9e3779b97f4a7c15ULL); }
SF_HD int32_t id_lookup(const TokState& ts, int64_t id, bool param) {
    uint64_t i = id_hash(id) & ts.id_mask;
    for (uint64_t p = 0; p <= ts.id_mask; p++) {
        const IdSlot& s = ts.idtab[i];
        if (s.id == 0) return -1;
        if (s.id == id) return param ? s.param : s.flow;
        i = (i + 1) & ts.id_mask;
    }
    return -1;
}

// ---------------------------------------------------------------- ClusterMetric (one flowId; in LDS
// for k_tok_decide, in HBM for the embedded requests of the slot chain; host-compilable for tests/)
struct ClMetric {
    ClFlowState* s;
    int S, wl, I;
    double isec;
    // LeapArray.currentWindow(t) with ClusterMetricLeapArray.resetWindowTo (:45-71); -1: throwaway
    SF_HD int cur(int64_t t) {
        const int idx = (int)((t / wl) % S);
        const int64_t ws = t - t % wl;
        ClBucket& b = s->b[idx];
        if (b.ws == WS_NONE) {                                   // newEmptyBucket: no transfer
            b.ws = ws;
            for (int k = 0; k < CE_COUNT; k++) b.c[k] = 0;
            return idx;
        }
        if (b.ws == ws) return idx;
        if (ws > b.ws) {
            b.ws = ws;
            for (int k = 0; k < CE_COUNT; k++) b.c[k] = 0;
            if (s->has_occ) {                                    // transferOccupyToBucket :54-60
                b.c[CE_OCCUPIED_PASS] = wadd(b.c[CE_OCCUPIED_PASS], s->occ_pass);
                b.c[CE_PASS] = wadd(b.c[CE_PASS], s->occ_pass); s->occ_pass = 0;
                b.c[CE_PASS_REQUEST] = wadd(b.c[CE_PASS_REQUEST], s->occ_req); s->occ_req = 0;
                s->has_occ = 0;
            }
            return idx;
        }
        return -1;
    }
    SF_HD int64_t sum(int ev, int64_t t) {                  // ClusterMetric.getSum :47-55
        cur(t);
        int64_t r = 0;
        for (int k = 0; k < S; k++) {
            const ClBucket& b = s->b[k];
            if (b.ws != WS_NONE && !(wsub(t, b.ws) > I)) r = wadd(r, b.c[ev]);
        }
        return r;
    }
    SF_HD double avg(int ev, int64_t t) { return (double)sum(ev, t) / isec; }
    SF_HD void add(int ev, int64_t n, int64_t t) {
        const int k = cur(t);
        if (k >= 0) s->b[k].c[ev] = wadd(s->b[k].c[ev], n);
    }
    SF_HD int64_t head_pass(int64_t t) {                    // getFirstCountOfWindow -> getValidHead
        const int idx = (int)(((t + wl) / wl) % S);
        const ClBucket& b = s->b[idx];
        if (b.ws == WS_NONE || wsub(t, b.ws) > I) return 0;
        return b.c[CE_PASS];
    }
};

// ClusterFlowChecker.acquireClusterToken (:55-112) for one request that passed the namespace gate
SF_HD void flow_decide(ClMetric& m, const ClRule& r, const TokState& ts, int32_t connected, int64_t t, int32_t c,
                       bool prio, int8_t* st, int32_t* rem, int32_t* wt) {
    const double latest = m.avg(CE_PASS, t);
    const double thr = (r.threshold_type == SF_THRESHOLD_GLOBAL ? r.count : r.count * connected) * ts.exceed_count;
    const double next = thr - latest - c;
    if (next >= 0) {
        m.add(CE_PASS, c, t); m.add(CE_PASS_REQUEST, 1, t);
        if (prio) m.add(CE_OCCUPIED_PASS, c, t);
        *st = SF_TOKEN_OK; *rem = j_d2i(next); *wt = 0;
        return;
    }
    if (prio) {
        const double occ_avg = m.avg(CE_WAITING, t);
        if (occ_avg <= ts.max_occupy_ratio * thr) {
            // ClusterMetric.tryOccupyNext :69-79, canOccupy :81-86
            const double latest2 = m.avg(CE_PASS, t);
            const int64_t head = m.head_pass(t);
            const int64_t occupied = m.s->occ_pass;
            if (latest2 + (double)((int64_t)c + occupied) - (double)head <= thr) {
                m.s->occ_pass = wadd(m.s->occ_pass, c);          // addOccupyPass :74-78
                m.s->occ_req = wadd(m.s->occ_req, 1);
                m.s->has_occ = 1;
                m.add(CE_WAITING, c, t);
                const int32_t w = 1000 / m.S;
                if (w > 0) { *st = SF_TOKEN_SHOULD_WAIT; *rem = 0; *wt = w; return; }
            }
        }
    }
    m.add(CE_BLOCK, c, t); m.add(CE_BLOCK_REQUEST, 1, t);
    if (prio) m.add(CE_OCCUPIED_BLOCK, c, t);
    *st = SF_TOKEN_BLOCKED; *rem = 0; *wt = 0;
}

// GlobalRequestLimiter.tryPass of one request at time t (RequestLimiter.java:51-87:
// canPass is getQps() + 1 <= qpsAllowed, then add(1)); what k_ns_limit decides
// for a window of requests, one request at a time
SF_HD bool lim_try_pass(LimState& L, double qps, int64_t t) {
    const int cur = (int)((t / LIM_WL) % LIM_S);
    const int64_t ws = t - t % LIM_WL;
    if (L.ws[cur] != ws) { L.ws[cur] = ws; L.v[cur] = 0; }
    int64_t sum = 0;
    for (int k = 0; k < LIM_S; k++)
        if (k == cur || (L.ws[k] != WS_NONE && !(t - L.ws[k] > LIM_INTERVAL))) sum = wadd(sum, L.v[k]);
    if (!((double)sum / 1.0 + 1 <= qps)) return false;
    L.v[cur] = wadd(L.v[cur], 1);
    return true;
}

// ---------------------------------------------------------------- embedded token server
// The tables a slot-chain walk needs to ask the engine's own token server
// (DefaultEmbeddedTokenServer: FlowRuleChecker.passClusterCheck calls
// DefaultTokenService.requestToken in-process, FlowRuleChecker.java:163-203).
// Lives in HBM; DevState::emb points to it (null: no bind loaded).
struct EmbState {
    TokState ts;                 // the token server's state, as sf_request_tokens uses it
    const int64_t* bind;         // [flow rules, CSR position] flowId of a bound cluster rule, 0: not bound
    unsigned long long* stats;   // [2] k_decide_xcl: chunks the wavefront solved, chunks lane 0 replayed
    uint32_t xcl_min, pad;       // shortest segment k_decide_xcl takes (XCL_MIN; diagnostics: SF_XCL_MIN)
};

// DefaultTokenService.requestToken(flow_id, c, prio) at time t
// (DefaultTokenService.java:39-64): what sf_request_tokens decides for a batch
// of this one request -- notValidRequest, the rule lookup, the namespace's
// GlobalRequestLimiter, then ClusterFlowChecker.acquireClusterToken on the
// flowId's ClusterMetric in HBM.  One lane at a time per flowId and per limiter
// namespace (the xflow groups, build_xmap).
// Not inlined on the device: the walks that call it (k_decide_x) are at their
// register limit already, and a rule without a bind never gets here.
#if defined(__HIPCC__)
__host__ __device__ __attribute__((noinline)) inline
#else
inline
#endif
void emb_request(const TokState& ts, int64_t flow_id, int64_t t, int32_t c, bool prio, int8_t* st, int32_t* wt) {
    *wt = 0;
    if (flow_id <= 0 || c <= 0) { *st = SF_TOKEN_BAD_REQUEST; return; }            // notValidRequest :66-68
    const int32_t r = id_lookup(ts, flow_id, false);
    if (r < 0) { *st = SF_TOKEN_NO_RULE_EXISTS; return; }                           // :45-47
    const ClRule rule = ts.rules[r];
    int32_t connected = 0;
    if (rule.ns >= 0) {
        const ClNs ns = ts.ns[rule.ns];
        connected = ns.connected;
        if (ns.has_limiter) {                                                       // ClusterFlowChecker.java:57-60
            LimState L = ts.lim[rule.ns];
            const bool ok = lim_try_pass(L, ns.max_qps, t);
            ts.lim[rule.ns] = L;
            if (!ok) { *st = SF_TOKEN_TOO_MANY_REQUEST; return; }
        }
    }
    ClMetric m{&ts.fstate[r], rule.S, rule.wl, rule.interval, rule.interval / 1000.0};
    int32_t rem;
    flow_decide(m, rule, ts, connected, t, c, prio, st, &rem, wt);
}

struct TokBatch {
    uint32_t n;
    const int64_t* flow_id; const int32_t* count; const uint8_t* flags; const int64_t* ts;
    const uint8_t* ptag; const uint64_t* pbits;
    const uint32_t* poff;        // [n+1] Collection<Object> params (values at [poff[i], poff[i+1])), or null
};
struct TokOut { int8_t* status; int32_t* remaining; int32_t* wait; };

struct TokWork {                 // sized for cfg.max_batch requests
    uint8_t* nskey_in; uint8_t* nskey_out;
    uint32_t* idx_in; uint32_t* idx_out;
    uint64_t* key_in; uint64_t* key_out;
    uint32_t* rule_of;           // [n] rule index of a request (valid where pending)
    uint8_t* pending;            // [n] 1: reached the checker
    uint32_t* head; uint32_t* head_scan;
    uint32_t* seg_start; uint32_t* n_seg;
    void* sort8_tmp; size_t sort8_bytes;
    void* sort64_tmp; size_t sort64_bytes;
    void* scan_tmp; size_t scan_bytes;
};

hipError_t tok_query_temp(uint32_t max_n, size_t* sort8, size_t* sort64, size_t* scan);
hipError_t tok_launch(const TokState& ts, TokWork& w, const TokBatch& b, const TokOut& out, hipStream_t s);
// the sort and segment table of tok_launch on keys the caller wrote (sf_rls.hip)
hipError_t tok_sort_segments(TokWork& w, uint32_t n, unsigned end_bit, hipStream_t s);
hipError_t tok_init_flow_state(ClFlowState* fs, uint32_t n, hipStream_t s);
// ClusterMetric.getSum(event) at time now (rolls the current window like the reference)
hipError_t tok_cluster_sum(const TokState& ts, uint32_t rule, int event, int64_t now, int64_t* d_out, hipStream_t s);

}  // namespace sf
