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

#if defined(__HIPCC__)
// flowId -> rule index of the flow (or param) rule table, -1: none (shared with sf_concur.hip)
__device__ __forceinline__ uint64_t id_hash(int64_t id) { return mix64((uint64_t)id * 0x9e3779b97f4a7c15ULL); }
__device__ __forceinline__ int32_t id_lookup(const TokState& ts, int64_t id, bool param) {
    uint64_t i = id_hash(id) & ts.id_mask;
    for (uint64_t p = 0; p <= ts.id_mask; p++) {
        const IdSlot& s = ts.idtab[i];
        if (s.id == 0) return -1;
        if (s.id == id) return param ? s.param : s.flow;
        i = (i + 1) & ts.id_mask;
    }
    return -1;
}

// ---------------------------------------------------------------- ClusterMetric (one flowId, in LDS)
struct ClMetric {
    ClFlowState* s;
    int S, wl, I;
    double isec;
    // LeapArray.currentWindow(t) with ClusterMetricLeapArray.resetWindowTo (:45-71); -1: throwaway
    __device__ int cur(int64_t t) {
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
    __device__ int64_t sum(int ev, int64_t t) {                  // ClusterMetric.getSum :47-55
        cur(t);
        int64_t r = 0;
        for (int k = 0; k < S; k++) {
            const ClBucket& b = s->b[k];
            if (b.ws != WS_NONE && !(wsub(t, b.ws) > I)) r = wadd(r, b.c[ev]);
        }
        return r;
    }
    __device__ double avg(int ev, int64_t t) { return (double)sum(ev, t) / isec; }
    __device__ void add(int ev, int64_t n, int64_t t) {
        const int k = cur(t);
        if (k >= 0) s->b[k].c[ev] = wadd(s->b[k].c[ev], n);
    }
    __device__ int64_t head_pass(int64_t t) {                    // getFirstCountOfWindow -> getValidHead
        const int idx = (int)(((t + wl) / wl) % S);
        const ClBucket& b = s->b[idx];
        if (b.ws == WS_NONE || wsub(t, b.ws) > I) return 0;
        return b.c[CE_PASS];
    }
};
#endif

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
