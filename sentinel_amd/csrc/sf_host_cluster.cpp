// sf_host_cluster.cpp -- the cluster side of the host runtime: the token
// server (sf_token.hip) with its wire framing (sf_wire.hip), the Envoy
// rate-limit service (sf_rls.hip) and the concurrency tokens (sf_concur.hip).
#include <unordered_map>

#include "sf_host.h"

extern "C" {

// ---------------------------------------------------------------- cluster token server
// Owner shard of a cluster rule's requests (sentinel_flow.h, sf_token_shard):
// a namespace with a GlobalRequestLimiter is one sequential gate, so all its
// rules live on namespace_id % N; any other rule on flow_id % N.
static uint32_t tok_rule_owner(int64_t flow_id, uint32_t ns_id, const std::vector<sf_namespace>& ns, uint32_t N) {
    for (const sf_namespace& x : ns)
        if (x.namespace_id == ns_id) {
            if (x.max_allowed_qps >= 0) return ns_id % N;
            break;
        }
    return flow_id <= 0 ? 0u : (uint32_t)((uint64_t)flow_id % N);
}

// Rebuild the device rule table, flowId index and namespace table from the
// host copies (ClusterFlowRuleManager / ClusterParamFlowRuleManager /
// ClusterServerConfigManager state).  Metric state is reset when
// `reset_state` (a rule reload creates new ClusterMetric objects:
// ClusterFlowRuleManager.java:361-362, ClusterParamFlowRuleManager.java:354-355).
static int tok_rebuild(sf_engine* e, bool reset_state) {
    TokState& ts = e->tok.ts;
    const uint32_t nf = (uint32_t)e->tok.host_cflow.size(), np = (uint32_t)e->tok.host_cparam.size();
    std::unordered_map<uint32_t, int32_t> ns_index;
    for (size_t i = 0; i < e->tok.host_ns.size(); i++) ns_index.emplace(e->tok.host_ns[i].namespace_id, (int32_t)i);
    std::vector<ClRule> rules(nf + np);
    auto fill = [&](ClRule& r, int64_t id, double count, int32_t tt, uint32_t ns, int32_t S, int32_t I) {
        r.count = count; r.flow_id = id; r.threshold_type = tt;
        auto it = ns_index.find(ns);
        r.ns = it == ns_index.end() ? -1 : it->second;
        r.S = S; r.wl = I / S; r.interval = I;
    };
    const uint32_t N = e->cfg.shard_count;
    for (uint32_t i = 0; i < nf; i++) {
        const sf_cluster_flow_rule& f = e->tok.host_cflow[i];
        fill(rules[i], f.flow_id, f.count, f.threshold_type, f.namespace_id, f.sample_count, f.window_interval_ms);
        rules[i].is_param = 0; rules[i].item_off = rules[i].item_cnt = 0;
        rules[i].owner = tok_rule_owner(f.flow_id, f.namespace_id, e->tok.host_ns, N);
    }
    for (uint32_t i = 0; i < np; i++) {
        const sf_cluster_param_rule& f = e->tok.host_cparam[i];
        ClRule& r = rules[nf + i];
        fill(r, f.flow_id, f.count, f.threshold_type, f.namespace_id, f.sample_count, f.window_interval_ms);
        r.is_param = 1; r.item_off = f.item_offset; r.item_cnt = f.item_count;
        r.owner = tok_rule_owner(f.flow_id, f.namespace_id, e->tok.host_ns, N);
    }
    // flowId -> rule index, open addressing; the first rule of an id wins (like the oracle's lookup)
    uint64_t cap = 16;
    while (cap < 2ull * (nf + np) + 2) cap <<= 1;
    std::vector<IdSlot> tab(cap, IdSlot{0, -1, -1});
    auto put = [&](int64_t id, int32_t idx, bool param) {
        uint64_t x = (uint64_t)id * 0x9e3779b97f4a7c15ULL;
        uint64_t i = mix64(x) & (cap - 1);
        while (tab[i].id != 0 && tab[i].id != id) i = (i + 1) & (cap - 1);
        tab[i].id = id;
        int32_t& slot = param ? tab[i].param : tab[i].flow;
        if (slot < 0) slot = idx;
    };
    for (uint32_t i = 0; i < nf; i++) if (rules[i].flow_id > 0) put(rules[i].flow_id, (int32_t)i, false);
    for (uint32_t i = 0; i < np; i++) if (rules[nf + i].flow_id > 0) put(rules[nf + i].flow_id, (int32_t)(nf + i), true);
    std::vector<ClNs> ns(e->tok.host_ns.size());
    for (size_t i = 0; i < ns.size(); i++) {
        ns[i].connected = e->tok.host_ns[i].connected_count;
        ns[i].has_limiter = e->tok.host_ns[i].max_allowed_qps >= 0;   // GlobalRequestLimiter.initIfAbsent
        ns[i].max_qps = e->tok.host_ns[i].max_allowed_qps;
    }
    std::vector<DevHotItem> items(e->tok.host_citems.size());
    for (size_t i = 0; i < items.size(); i++) {
        items[i].bits = e->tok.host_citems[i].bits; items[i].count = e->tok.host_citems[i].count; items[i].tag = e->tok.host_citems[i].tag;
    }
    hipStream_t s = e->stream;
    auto upload = [&](void** dst, const void* src, size_t bytes) -> int {
        e->pool.release(*dst);
        SF_TRY(e->pool.alloc(dst, min16(bytes)));
        if (bytes) HIP_TRY(hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, s));
        return SF_OK;
    };
    SF_TRY(upload((void**)&ts.rules, rules.data(), rules.size() * sizeof(ClRule)));
    SF_TRY(upload((void**)&ts.idtab, tab.data(), tab.size() * sizeof(IdSlot)));
    SF_TRY(upload((void**)&ts.ns, ns.data(), ns.size() * sizeof(ClNs)));
    SF_TRY(upload((void**)&ts.items, items.data(), items.size() * sizeof(DevHotItem)));
    e->pool.release(ts.rmulti);
    SF_TRY(e->pool.alloc(&ts.rmulti, min16(rules.size())));   // per-call multi-value flags
    ts.id_mask = cap - 1;
    ts.n_flow = nf; ts.n_rules = nf + np; ts.n_ns = (uint32_t)ns.size();
    if (reset_state) {
        e->pool.release(ts.fstate);
        SF_TRY(e->pool.alloc(&ts.fstate, std::max<size_t>(nf, 1) * sizeof(ClFlowState)));
        HIP_TRY(tok_init_flow_state(ts.fstate, nf, s));
        if (!ts.cptab) {
            uint64_t pc = 1024;
            while (pc < std::max<uint64_t>(e->cfg.param_capacity, 1024)) pc <<= 1;
            SF_TRY(e->pool.alloc(&ts.cptab, pc * sizeof(CpSlot)));
            ts.cp_mask = pc - 1;
        }
        HIP_TRY(hipMemsetAsync(ts.cptab, 0, (ts.cp_mask + 1) * sizeof(CpSlot), s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    return SF_OK;
}

// Per-flow-rule tables of the concurrency tokens: the two time-outs (always
// rebuilt) and nowCalls (replaced by `now` if given, created zeroed if absent).
static int cc_tables(sf_engine* e, const std::vector<int32_t>* now) {
    CcState& cs = e->cc.cs;
    const size_t nf = e->tok.host_cflow.size(), m = std::max<size_t>(nf, 1);
    std::unordered_map<int64_t, const sf_concurrent_config*> by_id;
    for (const sf_concurrent_config& c : e->cc.cfg) by_id.emplace(c.flow_id, &c);
    std::vector<CcCfg> cfg(m, CcCfg{CC_DEFAULT_TIMEOUT, CC_DEFAULT_TIMEOUT});
    for (size_t i = 0; i < nf; i++) {
        auto it = by_id.find(e->tok.host_cflow[i].flow_id);
        if (it != by_id.end()) cfg[i] = CcCfg{it->second->resource_timeout_ms, it->second->client_offline_time_ms};
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->pool.release(cs.cfg);
    SF_TRY(e->pool.alloc(&cs.cfg, m * sizeof(CcCfg)));
    HIP_TRY(hipMemcpy((void*)cs.cfg, cfg.data(), m * sizeof(CcCfg), hipMemcpyHostToDevice));
    if (now || !cs.now) {
        e->pool.release(cs.now);
        SF_TRY(e->pool.alloc(&cs.now, m * 4));
        if (now) HIP_TRY(hipMemcpy(cs.now, now->data(), m * 4, hipMemcpyHostToDevice));
        else HIP_TRY(hipMemset(cs.now, 0, m * 4));
    }
    if (!cs.ctr) {
        SF_TRY(e->pool.alloc(&cs.ctr, sizeof(CcCounters)));
        HIP_TRY(hipMemset(cs.ctr, 0, sizeof(CcCounters)));
    }
    return SF_OK;
}

int sf_load_namespaces(sf_engine* e, const sf_namespace* ns, uint32_t n) {
    if (!e || (n && !ns)) return fail(SF_ERR_INVALID, "null argument");
    if (n > 255) return fail(SF_ERR_UNSUPPORTED, "at most 255 namespaces");
    std::lock_guard<std::mutex> lk(e->mu);
    const bool emb = !e->binds.empty();          // the chain asks this token server: batches in flight read its state
    if (emb) { SF_TRY(drain(e)); e->st.emb = nullptr; }      // (the tables move: set again by xgroups_rebuild)
    e->tok.host_ns.assign(ns, ns + n);
    // GlobalRequestLimiter state of the loaded namespaces starts empty
    LimState z;
    for (int k = 0; k < LIM_S; k++) { z.ws[k] = WS_NONE; z.v[k] = 0; }
    std::vector<LimState> lim(std::max<uint32_t>(n, 1), z);
    e->pool.release(e->tok.ts.lim);
    SF_TRY(e->pool.alloc(&e->tok.ts.lim, lim.size() * sizeof(LimState)));
    HIP_TRY(hipMemcpyAsync(e->tok.ts.lim, lim.data(), lim.size() * sizeof(LimState), hipMemcpyHostToDevice, e->stream));
    SF_TRY(tok_rebuild(e, false));
    return emb ? xgroups_rebuild(e) : SF_OK;     // a limiter joins the resources bound into its namespace
}

int sf_load_cluster_rules(sf_engine* e, const sf_cluster_flow_rule* flow, uint32_t n_flow,
                          const sf_cluster_param_rule* param, uint32_t n_param, const sf_hot_item* items,
                          uint32_t n_items) {
    if (!e || (n_flow && !flow) || (n_param && !param) || (n_items && !items)) return fail(SF_ERR_INVALID, "null argument");
    auto check = [&](int32_t S, int32_t I) {
        return S > 0 && S <= CL_MAXS && I > 0 && I % S == 0;   // LeapArray.java:70-87
    };
    for (uint32_t i = 0; i < n_flow; i++)
        if (!check(flow[i].sample_count, flow[i].window_interval_ms))
            return fail(SF_ERR_UNSUPPORTED, "cluster flow rule: sample_count must be 1..16 and divide window_interval_ms");
    for (uint32_t i = 0; i < n_param; i++) {
        if (!check(param[i].sample_count, param[i].window_interval_ms))
            return fail(SF_ERR_UNSUPPORTED, "cluster param rule: sample_count must be 1..16 and divide window_interval_ms");
        if ((uint64_t)param[i].item_offset + param[i].item_count > n_items) return fail(SF_ERR_INVALID, "hot item range");
    }
    std::lock_guard<std::mutex> lk(e->mu);
    const bool emb = !e->binds.empty();
    if (emb) { SF_TRY(drain(e)); e->st.emb = nullptr; }
    // nowCalls of a flowId that stays loaded is kept (ClusterFlowRuleManager.java:271-375)
    std::unordered_map<int64_t, int32_t> kept;
    if (e->cc.cs.now && !e->tok.host_cflow.empty()) {
        std::vector<int32_t> old(e->tok.host_cflow.size());
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipMemcpy(old.data(), e->cc.cs.now, old.size() * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < old.size(); i++)
            if (e->tok.host_cflow[i].flow_id > 0) kept.emplace(e->tok.host_cflow[i].flow_id, old[i]);
    }
    e->tok.host_cflow.assign(flow, flow + n_flow);
    e->tok.host_cparam.assign(param, param + n_param);
    e->tok.host_citems.assign(items, items + n_items);
    int rc = tok_rebuild(e, true);
    if (!rc && emb) rc = xgroups_rebuild(e);     // a bound flowId's namespace may have changed
    if (rc || !e->cc.cs.now) return rc;
    std::vector<int32_t> now(std::max<uint32_t>(n_flow, 1), 0);
    for (uint32_t i = 0; i < n_flow; i++) {                    // (the first rule of an id is the one looked up)
        auto it = kept.find(flow[i].flow_id);
        if (it != kept.end()) { now[i] = it->second; kept.erase(it); }
    }
    return cc_tables(e, &now);
}

// Embedded token server (DefaultEmbeddedTokenServer): which cluster-mode flow
// rules of sf_load_flow_rules ask this engine's token server from inside the
// slot chain (FlowRuleChecker.passClusterCheck, FlowRuleChecker.java:163-203).
// Every error is decided before anything changes.
int sf_load_cluster_binds(sf_engine* e, const sf_cluster_bind* binds, uint32_t n) {
    if (!e || (n && !binds)) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    // a resource's shard and a flowId's owner are different maps (sf_token_shard)
    if (n && e->cfg.shard_count != 1)
        return fail(SF_ERR_UNSUPPORTED, "sf_load_cluster_binds on a sharded engine");
    std::vector<uint8_t> seen(e->flow_csr_of.size(), 0);
    for (uint32_t i = 0; i < n; i++) {
        const sf_cluster_bind& b = binds[i];
        if (b.rule_index >= e->flow_csr_of.size()) return fail(SF_ERR_INVALID, "cluster bind: rule_index out of range");
        if (!e->flow_cluster[b.rule_index]) return fail(SF_ERR_INVALID, "cluster bind: the rule is not cluster_mode");
        if (e->flow_csr_of[b.rule_index] < 0) return fail(SF_ERR_INVALID, "cluster bind: the rule was dropped as invalid");
        if (b.flow_id <= 0) return fail(SF_ERR_INVALID, "cluster bind: flow_id must be > 0 (FlowRuleUtil.validClusterRuleId)");
        if (seen[b.rule_index]++) return fail(SF_ERR_INVALID, "cluster bind: two binds name one rule");
    }
    SF_TRY(drain(e));   // pending batches were sorted under the old groups
    const std::vector<sf_cluster_bind> old = e->binds;
    e->binds.assign(binds, binds + n);
    const int rc = xgroups_rebuild(e);
    if (rc) {                                    // a device failure: back to the old binds if they can be rebuilt,
        e->binds = old;                          // else (st.emb null) every cluster rule is decided as unbound
        if (xgroups_rebuild(e)) e->binds.clear();
    }
    return rc;
}

// the scratch sizes of the work sets (sf_worksets.h) as rocPRIM states them
static int tok_temp_query(uint32_t n, size_t* s8, size_t* s64, size_t* scan) { HIP_TRY(tok_query_temp(n, s8, s64, scan)); return SF_OK; }
static int cc_temp_query(uint32_t n, size_t* bytes) { HIP_TRY(cc_query_temp(n, bytes)); return SF_OK; }

// token state present (rules built, namespace limiter allocated); caller holds e->mu
extern "C++" int tok_ready(sf_engine* e) {
    if (!e->tok.ts.rules) SF_TRY(tok_rebuild(e, true));
    if (!e->tok.ts.lim) {
        LimState z; for (int k = 0; k < LIM_S; k++) { z.ws[k] = WS_NONE; z.v[k] = 0; }
        SF_TRY(e->pool.alloc(&e->tok.ts.lim, sizeof(LimState)));
        HIP_TRY(hipMemcpy(e->tok.ts.lim, &z, sizeof z, hipMemcpyHostToDevice));
    }
    return SF_OK;
}

int sf_request_tokens(sf_engine* e, const sf_token_batch* in, sf_token_results* out) {
    if (!e || !in || !out || !out->status) return fail(SF_ERR_INVALID, "null argument");
    if (in->n == 0) return SF_OK;
    if (!in->flow_id || !in->count || !in->flags || !in->ts_ms) return fail(SF_ERR_INVALID, "missing request array");
    if ((in->param_tag == nullptr) != (in->param_bits == nullptr)) return fail(SF_ERR_INVALID, "param_tag/param_bits");
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->binds.empty()) SF_TRY(drain(e));     // embedded mode: submit batches in flight take tokens too
    const uint32_t n = in->n;
    SF_TRY(tok_work_ensure(e->tok.tw, n, e->cfg.max_batch, tok_temp_query));
    SF_TRY(tok_ready(e));
    hipStream_t s = e->stream;
    TokBatch b{};
    b.n = n;
    const bool has_param = in->param_tag != nullptr;
    // Collection params: the value arrays hold param_off[n] elements
    uint32_t n_vals = n;
    if (in->param_off) {
        if (in->mem == SF_MEM_HOST) n_vals = in->param_off[n];
        else HIP_TRY(hipMemcpy(&n_vals, in->param_off + n, 4, hipMemcpyDeviceToHost));
    }
    const bool host_out = out->mem == SF_MEM_HOST;
    if (!host_out && (!out->remaining || !out->wait_ms)) return fail(SF_ERR_INVALID, "device results need remaining and wait_ms");
    // staging: inputs then outputs (param_tag / param_bits are passed on even
    // with no value; remaining / wait_ms have room whether or not they are asked for)
    TokOut o{};
    StagePlan plan(in->mem == SF_MEM_HOST, host_out);
    plan.in(true, &b.flow_id, in->flow_id, (size_t)n * 8); plan.in(true, &b.count, in->count, (size_t)n * 4);
    plan.in(true, &b.flags, in->flags, n); plan.in(true, &b.ts, in->ts_ms, (size_t)n * 8);
    plan.in(has_param, &b.ptag, in->param_tag, n_vals); plan.in(has_param, &b.pbits, in->param_bits, (size_t)n_vals * 8);
    plan.in(in->param_off != nullptr, &b.poff, in->param_off, ((size_t)n + 1) * 4);
    plan.out(true, &o.status, out->status, n);
    plan.out(true, &o.remaining, out->remaining, (size_t)n * 4, out->remaining != nullptr);
    plan.out(true, &o.wait, out->wait_ms, (size_t)n * 4, out->wait_ms != nullptr);
    SF_TRY(e->tok.stage.reserve(e->pool, plan.size()));
    plan.bind(e->tok.stage.p);
    SF_TRY(plan.upload(h2d_on(s)));
    HIP_TRY(hipMemsetAsync(e->st.err, 0, sizeof(int32_t), s));
    hipError_t le = tok_launch(e->tok.ts, e->tok.tw.w, b, o, s);
    if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("token launch: ") + hipGetErrorString(le));
    SF_TRY(plan.download(d2h_on(s)));
    int32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, e->st.err, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (err) return fail(err, err == SF_ERR_CAPACITY ? "cluster param table capacity exceeded"
                                                     : "invalid token batch (a request owned by another shard?)");
    return SF_OK;
}

int sf_token_shard(const sf_cluster_flow_rule* flow, uint32_t n_flow, const sf_cluster_param_rule* param,
                   uint32_t n_param, const sf_namespace* ns, uint32_t n_ns, uint32_t shard_count,
                   const int64_t* flow_id, const uint8_t* flags, uint32_t n, uint32_t* out_shard) {
    if ((n_flow && !flow) || (n_param && !param) || (n_ns && !ns) || (n && (!flow_id || !flags || !out_shard)) ||
        shard_count == 0)
        return fail(SF_ERR_INVALID, "sf_token_shard arguments");
    const std::vector<sf_namespace> nsv(ns, ns + n_ns);
    std::unordered_map<int64_t, uint32_t> fo, po;                  // first rule of an id (tok_rebuild's lookup)
    for (uint32_t i = 0; i < n_flow; i++)
        if (flow[i].flow_id > 0) fo.emplace(flow[i].flow_id, tok_rule_owner(flow[i].flow_id, flow[i].namespace_id, nsv, shard_count));
    for (uint32_t i = 0; i < n_param; i++)
        if (param[i].flow_id > 0) po.emplace(param[i].flow_id, tok_rule_owner(param[i].flow_id, param[i].namespace_id, nsv, shard_count));
    for (uint32_t i = 0; i < n; i++) {
        const int64_t id = flow_id[i];
        if (id <= 0) { out_shard[i] = 0; continue; }
        const auto& m = (flags[i] & SF_TOK_PARAM) ? po : fo;
        const auto it = m.find(id);
        out_shard[i] = it != m.end() ? it->second : (uint32_t)((uint64_t)id % shard_count);
    }
    return SF_OK;
}

uint64_t sf_string_key(const uint8_t* bytes, uint32_t len) {   // FNV-1a 64 (the wire path's String key)
    uint64_t h = 0xcbf29ce484222325ULL;
    for (uint32_t i = 0; i < len; i++) { h ^= bytes[i]; h *= 0x100000001b3ULL; }
    return h;
}

int sf_serve_frames(sf_engine* e, const sf_wire_batch* in, sf_wire_out* out) {
    if (!e || !in || !out || !in->stream_off || !out->resp_off || !out->consumed || !out->stop)
        return fail(SF_ERR_INVALID, "null argument");
    if (in->n_streams == 0) return fail(SF_ERR_INVALID, "n_streams must be > 0");
    if (e->cfg.shard_count > 1)
        return fail(SF_ERR_UNSUPPORTED, "sf_serve_frames on a sharded token server: route decoded requests with sf_token_shard");
    const uint32_t S = in->n_streams;
    std::vector<uint64_t> soff(S + 1);
    if (in->mem == SF_MEM_HOST) std::memcpy(soff.data(), in->stream_off, (S + 1) * sizeof(uint64_t));
    else HIP_TRY(hipMemcpy(soff.data(), in->stream_off, (S + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (uint32_t s = 0; s < S; s++)
        if (soff[s + 1] < soff[s]) return fail(SF_ERR_INVALID, "stream_off must be non-decreasing");
    if (soff[S] >= (1ull << 31)) return fail(SF_ERR_CAPACITY, "wire batch must be < 2^31 bytes");
    if (soff[S] && !in->bytes) return fail(SF_ERR_INVALID, "null bytes");
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->binds.empty()) SF_TRY(drain(e));
    out->n_frames = out->n_requests = out->n_responses = 0;
    const uint32_t n = (uint32_t)soff[S];
    if (soff[0] == n) {                          // nothing to read: every stream handled, no response
        for (uint32_t s = 0; s < S; s++) { out->consumed[s] = 0; out->stop[s] = SF_WIRE_DONE; }
        for (uint32_t s = 0; s <= S; s++) out->resp_off[s] = 0;
        return SF_OK;
    }
    SF_TRY(tok_ready(e));
    hipStream_t st = e->stream;
    WireBufs w{};
    w.n = n; w.S = S;
    w.n_tiles = (n + WIRE_TILE - 1) / WIRE_TILE;
    const uint32_t F = n / 2 + 1;                 // frames are >= 2 bytes
    size_t tmp = 0;
    { hipError_t qe = wire_query_temp(w.n_tiles, S, F, &tmp);
      if (qe != hipSuccess) return fail(SF_ERR_DEVICE, std::string("wire temp: ") + hipGetErrorString(qe)); }
    // one grow-only arena: the staged input (host form), then the scratch of every pass
    StagePlan plan(in->mem == SF_MEM_HOST, false);
    plan.in(true, &w.bytes, in->bytes, n, n + 16);
    plan.in(true, &w.soff, in->mem == SF_MEM_HOST ? soff.data() : in->stream_off, (S + 1) * 8);
    const auto room = [&](auto** dev, size_t bytes) { plan.scratch(dev, min16(bytes)); };
    const size_t T = w.n_tiles;
    room(&w.exitv, (size_t)n * 4); room(&w.tentry, T * 4); room(&w.bitmap, T * (WIRE_TILE / 32) * 4);
    room(&w.tcount, (T + 1) * 4); room(&w.tbase, (T + 1) * 4); room(&w.consumed, (size_t)S * 4);
    room(&w.stopoff, (size_t)S * 4); room(&w.resp_scan, ((size_t)S + 1) * 4); room(&w.frames, (size_t)F * 4);
    room(&w.wf, (size_t)F * sizeof(WFrame)); room(&w.fl, (size_t)F * 8); room(&w.pos, (size_t)F * 8);
    room(&w.counters, 16);
    room(&w.q_fid, (size_t)F * 8); room(&w.q_cnt, (size_t)F * 4); room(&w.q_flags, F); room(&w.q_ts, (size_t)F * 8);
    room(&w.q_tag, n); room(&w.q_bits, (size_t)n * 8); room(&w.r_status, F); room(&w.r_rem, (size_t)F * 4);
    room(&w.nval, (size_t)F * 4); room(&w.q_nval, ((size_t)F + 1) * 4); room(&w.q_poff, ((size_t)F + 1) * 4);
    room(&w.r_wait, (size_t)F * 4); room(&w.resp, (size_t)F * 16); room(&w.stop, S);
    room(&w.consumed_rel, (size_t)S * 8); room(&w.tmp, tmp);
    w.resp_cnt = nullptr; w.tmp_bytes = tmp;
    SF_TRY(e->tok.wire_arena.reserve(e->pool, plan.size()));
    plan.bind(e->tok.wire_arena.p);
    SF_TRY(plan.upload(h2d_on(st)));

    if (e->timing) {
        for (auto& x : e->rep.ml_ev) if (!x) HIP_TRY(hipEventCreate(&x));
        HIP_TRY(hipEventRecord(e->rep.ml_ev[0], st));
    }
    hipError_t le = wire_frame(w, st);
    if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("wire framing: ") + hipGetErrorString(le));
    uint32_t nf = 0;
    HIP_TRY(hipMemcpyAsync(&nf, w.tbase + w.n_tiles, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    uint64_t tot[2] = {0, 0};
    if (nf) {
        le = wire_decode(w, nf, in->now_ms, st);
        if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("wire decode: ") + hipGetErrorString(le));
        HIP_TRY(hipMemcpyAsync(&tot[0], w.pos + nf - 1, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&tot[1], w.fl + nf - 1, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    const uint64_t both = tot[0] + tot[1];
    const uint32_t n_req = (uint32_t)(both >> 32), n_resp = (uint32_t)both;
    HIP_TRY(hipMemsetAsync(e->st.err, 0, sizeof(int32_t), st));
    if (n_req) {
        SF_TRY(tok_work_ensure(e->tok.tw, n_req, e->cfg.max_batch, tok_temp_query));
        le = wire_compact(w, nf, n_req, in->now_ms, st);
        if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("wire compact: ") + hipGetErrorString(le));
        TokBatch b{};
        b.n = n_req; b.flow_id = w.q_fid; b.count = w.q_cnt; b.flags = w.q_flags; b.ts = w.q_ts;
        b.ptag = w.q_tag; b.pbits = w.q_bits; b.poff = w.q_poff;
        TokOut o{w.r_status, w.r_rem, w.r_wait};
        le = tok_launch(e->tok.ts, e->tok.tw.w, b, o, st);
        if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("token launch: ") + hipGetErrorString(le));
    }
    le = wire_encode(w, nf, st);
    if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("wire encode: ") + hipGetErrorString(le));
    if (e->timing) HIP_TRY(hipEventRecord(e->rep.ml_ev[1], st));
    const bool fits = (uint64_t)n_resp * SF_WIRE_RESP_BYTES <= out->cap;
    if (fits && n_resp) {
        if (!out->resp) return fail(SF_ERR_INVALID, "null resp");
        HIP_TRY(hipMemcpyAsync(out->resp, w.resp, (size_t)n_resp * SF_WIRE_RESP_BYTES, hipMemcpyDeviceToHost, st));
    }
    std::vector<uint32_t> roff(S + 1);
    uint32_t handled = 0;
    int32_t err = 0;
    HIP_TRY(hipMemcpyAsync(roff.data(), w.resp_scan, (S + 1) * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->consumed, w.consumed_rel, (size_t)S * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->stop, w.stop, S, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&handled, w.counters, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&err, e->st.err, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (e->timing) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, e->rep.ml_ev[0], e->rep.ml_ev[1]));
        e->stats.wire_ms = ms;
    }
    for (uint32_t s = 0; s <= S; s++) out->resp_off[s] = (uint64_t)roff[s] * SF_WIRE_RESP_BYTES;
    out->n_frames = handled; out->n_requests = n_req; out->n_responses = n_resp;
    if (err) return fail(err, err == SF_ERR_CAPACITY ? "cluster param table capacity exceeded" : "invalid token batch");
    if (!fits) return fail(SF_ERR_CAPACITY, "response buffer too small (n_responses * 16 bytes needed)");
    return SF_OK;
}

int sf_cluster_sum(sf_engine* e, int64_t flow_id, int event, int64_t now_ms, int64_t* out) {
    if (!e || !out) return fail(SF_ERR_INVALID, "null argument");
    if (event < 0 || event >= CE_COUNT) return fail(SF_ERR_INVALID, "event");
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->binds.empty()) SF_TRY(drain(e));
    *out = 0;
    for (size_t i = 0; i < e->tok.host_cflow.size(); i++) {
        if (e->tok.host_cflow[i].flow_id != flow_id) continue;
        HIP_TRY(tok_cluster_sum(e->tok.ts, (uint32_t)i, event, now_ms, e->tok.d_sum, e->stream));
        HIP_TRY(hipMemcpyAsync(out, e->tok.d_sum, 8, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        return SF_OK;
    }
    return SF_OK;
}

// ---------------------------------------------------------------- Envoy rate-limit service (sf_rls.h)
int64_t sf_rls_flow_id(const uint8_t* key_utf8, uint32_t len) {
    RlsKey k = rls_key_begin();
    if (len) rls_key_feed(k, key_utf8, len);
    return k.ok ? rls_key_id(k) : INT64_MIN;
}

int sf_rls_get_stats(sf_engine* e, sf_rls_stats* out) {
    if (!e || !out) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    *out = e->rls.stats;
    return SF_OK;
}

int sf_request_rls(sf_engine* e, const sf_rls_batch* in, sf_rls_results* out) {
    if (!e || !in || !out) return fail(SF_ERR_INVALID, "null argument");
    if (e->cfg.shard_count != 1)
        return fail(SF_ERR_UNSUPPORTED, "sf_request_rls on a sharded token server: route the descriptors by flowId");
    const uint32_t n = in->n;
    if (n == 0) return SF_OK;
    if (!in->ts_ms || !in->hits_addend || !in->desc_off || !out->overall) return fail(SF_ERR_INVALID, "missing request array");
    const bool strings = in->desc_flow_id == nullptr;
    if (strings && (!in->domain || !in->ent_off || !in->str_off)) return fail(SF_ERR_INVALID, "missing string table");
    const bool host_in = in->mem == SF_MEM_HOST, host_out = out->mem == SF_MEM_HOST;
    if (n > e->cfg.max_batch) return fail(SF_ERR_CAPACITY, "more requests than max_batch");
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->binds.empty()) SF_TRY(drain(e));
    RlsBatch b{};
    b.n = n; b.n_str = strings ? in->n_str : 0;
    // the lengths of the tables are their last offsets: read in place, or gathered on the device for one copy
    if (host_in) {
        b.n_desc = in->desc_off[n];
        if (strings && b.n_desc <= e->cfg.max_batch) { b.n_ent = in->ent_off[b.n_desc]; b.n_bytes = in->str_off[b.n_str]; }
    } else {
        if (!e->rls.len) SF_TRY(e->pool.alloc(&e->rls.len, 16));
        b.desc_off = in->desc_off; b.desc_fid = in->desc_flow_id; b.ent_off = in->ent_off; b.str_off = in->str_off;
        uint32_t len[3] = {0, 0, 0};
        HIP_TRY(rls_lengths(b, e->rls.len, e->stream));
        HIP_TRY(hipMemcpyAsync(len, e->rls.len, sizeof len, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        b.n_desc = len[0]; b.n_ent = len[1]; b.n_bytes = len[2];
    }
    if (b.n_desc > e->cfg.max_batch) return fail(SF_ERR_CAPACITY, "more descriptors than max_batch");
    if (b.n_desc && !out->code) return fail(SF_ERR_INVALID, "null code array");
    if (strings) {
        if (b.n_bytes >= (1u << 31)) return fail(SF_ERR_CAPACITY, "rls strings must be < 2^31 bytes");
        if ((b.n_ent && (!in->ent_key || !in->ent_val)) || (b.n_bytes && !in->bytes)) return fail(SF_ERR_INVALID, "missing string table");
    }
    const size_t nd = b.n_desc, ne = b.n_ent, ns = b.n_str;
    SF_TRY(tok_work_ensure(e->tok.tw, std::max(b.n_desc, 1u), e->cfg.max_batch, tok_temp_query));
    SF_TRY(rls_work_ensure(e->rls.ws, std::max(n, b.n_desc), e->cfg.max_batch));
    SF_TRY(tok_ready(e));
    hipStream_t s = e->stream;
    // staging: inputs (host form) then outputs (host results).  A host batch
    // has the flowId array or the string tables; a device batch's pointers
    // are passed on as they are.
    const bool ids = !strings, str = strings || !host_in;
    RlsOut o{};
    StagePlan plan(host_in, host_out);
    plan.in(true, &b.ts, in->ts_ms, (size_t)n * 8); plan.in(true, &b.hits, in->hits_addend, (size_t)n * 4);
    plan.in(true, &b.desc_off, in->desc_off, ((size_t)n + 1) * 4); plan.in(ids, &b.desc_fid, in->desc_flow_id, nd * 8);
    plan.in(str, &b.domain, in->domain, (size_t)n * 4); plan.in(str, &b.ent_off, in->ent_off, (nd + 1) * 4);
    plan.in(str, &b.ent_key, in->ent_key, ne * 4); plan.in(str, &b.ent_val, in->ent_val, ne * 4);
    plan.in(str, &b.str_off, in->str_off, (ns + 1) * 4); plan.in(str, &b.bytes, in->bytes, b.n_bytes);
    plan.out(true, &o.overall, out->overall, n); plan.out(true, &o.code, out->code, nd);
    plan.out(true, &o.limit, out->limit, nd * 4, out->limit != nullptr);
    plan.out(true, &o.remaining, out->remaining, nd * 4, out->remaining != nullptr);
    plan.out(true, &o.flow_id, out->flow_id, nd * 8, out->flow_id != nullptr);
    SF_TRY(e->rls.stage.reserve(e->pool, std::max<size_t>(plan.size(), 16)));
    plan.bind(e->rls.stage.p);
    SF_TRY(plan.upload(h2d_on(s)));
    HIP_TRY(hipMemsetAsync(e->st.err, 0, sizeof(int32_t), s));
    hipError_t le = rls_launch(e->tok.ts, e->tok.tw.w, e->rls.ws.w, b, o, e->rls.wave_min, s);
    if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("rls launch: ") + hipGetErrorString(le));
    int32_t err = 0;
    RlsCounters c{};
    HIP_TRY(hipMemcpyAsync(&err, e->st.err, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&c, e->rls.ws.w.ctr, sizeof c, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (err) return fail(err, "malformed rls batch (offsets must not decrease, string indices must be < n_str, ts_ms must be >= 0)");
    if (host_out) {
        SF_TRY(plan.download(d2h_on(s)));
        HIP_TRY(hipStreamSynchronize(s));
    }
    sf_rls_stats& st = e->rls.stats;
    st.requests += n; st.descriptors += nd; st.error_requests += c.error_requests; st.no_rule += c.no_rule;
    st.segs_lane += c.segs_lane; st.segs_wave += c.segs_wave; st.chunks += c.chunks;
    st.chunks_serial += c.chunks_serial; st.rounds += c.rounds;
    return SF_OK;
}

// ---------------------------------------------------------------- cluster concurrency tokens
// state of the concurrency tokens present; caller holds e->mu
static int cc_ready(sf_engine* e) {
    SF_TRY(tok_ready(e));
    if (!e->cc.cs.now || !e->cc.cs.cfg || !e->cc.cs.ctr) return cc_tables(e, nullptr);
    return SF_OK;
}

static int cc_read_counters(sf_engine* e) {
    HIP_TRY(hipMemcpyAsync(&e->cc.ctr, e->cc.cs.ctr, sizeof(CcCounters), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SF_OK;
}

// The pool holds at least `min_cap` slots and at least `need_free` free ones:
// a larger array with the old one copied and the new slots pushed, so slot
// numbers and live ids stay valid.  SF_ERR_CAPACITY past 2^28 slots, nothing changed.
static int cc_pool_ensure(sf_engine* e, uint64_t need_free, uint64_t min_cap) {
    CcHost& c = e->cc;
    CcState& cs = c.cs;
    const uint64_t cap = cs.cap, free_now = c.ctr.top;
    if (free_now >= need_free && cap >= min_cap && cap) return SF_OK;
    uint64_t ncap = std::max<uint64_t>(min_cap, cap);
    if (free_now < need_free) ncap = std::max<uint64_t>({ncap, cap + (need_free - free_now), 2 * cap});
    if (!cap && !min_cap) ncap = std::max<uint64_t>(ncap, 1024);
    ncap = std::max<uint64_t>(ncap, 1);
    if (ncap > CC_MAX_SLOTS) ncap = CC_MAX_SLOTS;
    if (ncap < min_cap || ncap - cap + free_now < need_free)
        return fail(SF_ERR_CAPACITY, "concurrency token pool: more than 2^28 slots needed");
    if (ncap == cap) return SF_OK;
    hipStream_t s = e->stream;
    CcSlot* slots = nullptr; uint32_t* stack = nullptr; uint32_t* claim = nullptr;
    DevPool fresh{HIP_MEM};                    // (the new arrays; an early return frees them and the old pool stays)
    SF_TRY(fresh.alloc(&slots, ncap * sizeof(CcSlot)));
    SF_TRY(fresh.alloc(&stack, ncap * 4));
    SF_TRY(fresh.alloc(&claim, ncap * 4));
    HIP_TRY(hipMemsetAsync(slots, 0, ncap * sizeof(CcSlot), s));
    if (cap) {
        HIP_TRY(hipMemcpyAsync(slots, cs.slots, cap * sizeof(CcSlot), hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(stack, cs.stack, cap * 4, hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipMemcpyAsync(claim, cs.claim, cap * 4, hipMemcpyDeviceToDevice, s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    e->pool.release_all(cs.slots, cs.stack, cs.claim);
    e->pool.adopt(fresh);
    cs.slots = slots; cs.stack = stack; cs.claim = claim; cs.cap = (uint32_t)ncap;
    HIP_TRY(cc_push_range(cs, (uint32_t)cap, (uint32_t)ncap, s));
    if (cap) c.grows++;
    return cc_read_counters(e);
}

int sf_load_concurrent_config(sf_engine* e, const sf_concurrent_config* cfg, uint32_t n) {
    if (!e || (n && !cfg)) return fail(SF_ERR_INVALID, "null argument");
    for (uint32_t i = 0; i < n; i++)
        if (cfg[i].resource_timeout_ms <= 0 || cfg[i].client_offline_time_ms <= 0)      // FlowRuleUtil.java:195
            return fail(SF_ERR_INVALID, "concurrent config: time-outs must be > 0");
    std::lock_guard<std::mutex> lk(e->mu);
    e->cc.cfg.assign(cfg, cfg + n);
    return e->cc.cs.cfg ? cc_tables(e, nullptr) : SF_OK;
}

int sf_concurrent_reserve(sf_engine* e, uint64_t tokens) {
    if (!e) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(cc_ready(e));
    return cc_pool_ensure(e, 0, std::max<uint64_t>(tokens, 1));
}

int sf_request_concurrent(sf_engine* e, const sf_concurrent_batch* in, sf_concurrent_results* out) {
    if (!e || !in || !out || !out->status || !out->token_id) return fail(SF_ERR_INVALID, "null argument");
    if (in->n == 0) return SF_OK;
    if (!in->op || !in->id || !in->count || !in->client || !in->ts_ms) return fail(SF_ERR_INVALID, "missing request array");
    if (e->cfg.shard_count > 255) return fail(SF_ERR_UNSUPPORTED, "concurrency tokens: at most 255 shards (token id layout)");
    std::lock_guard<std::mutex> lk(e->mu);
    const uint32_t n = in->n;
    SF_TRY(cc_ready(e));
    SF_TRY(cc_work_ensure(e->cc.ws, n, (uint32_t)e->tok.host_cflow.size(), cc_temp_query));
    SF_TRY(cc_pool_ensure(e, n, 0));     // a slot for every request, before any state changes
    CcHost& c = e->cc;
    hipStream_t s = e->stream;
    CcBatch b{};
    b.n = n;
    CcOut o{};
    StagePlan plan(in->mem == SF_MEM_HOST, out->mem == SF_MEM_HOST);
    plan.in(true, &b.op, in->op, n); plan.in(true, &b.id, in->id, (size_t)n * 8);
    plan.in(true, &b.count, in->count, (size_t)n * 4); plan.in(true, &b.client, in->client, (size_t)n * 4);
    plan.in(true, &b.ts, in->ts_ms, (size_t)n * 8);
    plan.out(true, &o.status, out->status, n); plan.out(true, &o.token_id, out->token_id, (size_t)n * 8);
    SF_TRY(c.stage.reserve(e->pool, plan.size()));
    plan.bind(c.stage.p);
    SF_TRY(plan.upload(h2d_on(s)));
    HIP_TRY(hipMemsetAsync(e->st.err, 0, sizeof(int32_t), s));
    hipError_t le = cc_launch(e->tok.ts, c.cs, c.ws.w, b, o, s);
    if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("concurrent launch: ") + hipGetErrorString(le));
    SF_TRY(plan.download(d2h_on(s)));
    int32_t err = 0;
    HIP_TRY(hipMemcpyAsync(&err, e->st.err, 4, hipMemcpyDeviceToHost, s));
    SF_TRY(cc_read_counters(e));
    if (err) return fail(err, err == SF_ERR_CAPACITY ? "concurrency token pool exhausted"
                                                     : "invalid concurrent batch (a request owned by another shard?)");
    return SF_OK;
}

int sf_concurrent_expire(sf_engine* e, int64_t now_ms, const uint8_t* client_online, uint32_t n_clients,
                         uint32_t* n_expired) {
    if (!e || (n_clients && !client_online)) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(cc_ready(e));
    CcHost& c = e->cc;
    SF_TRY(c.online.reserve(e->pool, n_clients));
    uint8_t* online = (uint8_t*)c.online.p;
    if (n_clients) HIP_TRY(hipMemcpyAsync(online, client_online, n_clients, hipMemcpyHostToDevice, e->stream));
    const uint64_t before = c.ctr.expired;
    HIP_TRY(cc_expire(e->tok.ts, c.cs, now_ms, online, n_clients, e->stream));
    SF_TRY(cc_read_counters(e));
    if (n_expired) *n_expired = (uint32_t)(c.ctr.expired - before);
    return SF_OK;
}

int sf_concurrent_now(sf_engine* e, int64_t flow_id, int64_t* now_calls) {
    if (!e || !now_calls) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    if (flow_id > 0)
        for (size_t i = 0; i < e->tok.host_cflow.size(); i++) {
            if (e->tok.host_cflow[i].flow_id != flow_id) continue;
            SF_TRY(cc_ready(e));
            int32_t v = 0;
            HIP_TRY(hipStreamSynchronize(e->stream));
            HIP_TRY(hipMemcpy(&v, e->cc.cs.now + i, 4, hipMemcpyDeviceToHost));
            *now_calls = v;
            return SF_OK;
        }
    return fail(SF_ERR_INVALID, "sf_concurrent_now: flowId not loaded");
}

int sf_read_token(sf_engine* e, int64_t token_id, sf_token_node* out) {
    if (!e || !out) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    const uint64_t tid = (uint64_t)token_id;
    const uint32_t slot = (uint32_t)tid & CC_SLOT_MASK, gen = (uint32_t)(tid >> CC_SLOT_BITS) & CC_SLOT_MASK;
    if ((tid >> 56) != (uint64_t)e->cfg.shard_index + 1 || slot >= e->cc.cs.cap)
        return fail(SF_ERR_INVALID, "sf_read_token: not a live token");
    CcSlot sl;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipMemcpy(&sl, e->cc.cs.slots + slot, sizeof sl, hipMemcpyDeviceToHost));
    if (!sl.live || sl.gen != gen) return fail(SF_ERR_INVALID, "sf_read_token: not a live token");
    out->flow_id = sl.flow_id; out->client_deadline_ms = sl.client_deadline; out->resource_deadline_ms = sl.resource_deadline;
    out->count = sl.count; out->client = sl.client;
    return SF_OK;
}

int sf_concurrent_get_stats(sf_engine* e, sf_concurrent_stats* out) {
    if (!e || !out) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    const CcHost& c = e->cc;
    out->live_tokens = (uint64_t)c.cs.cap - c.ctr.top; out->pool_capacity = c.cs.cap; out->pool_grows = c.grows;
    out->chunks = c.ctr.chunks; out->chunks_all_pass = c.ctr.chunks_all_pass; out->rounds = c.ctr.rounds;
    out->expired = c.ctr.expired;
    return SF_OK;
}

}  // extern "C"
