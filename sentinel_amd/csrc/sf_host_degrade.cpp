// sf_host_degrade.cpp -- DegradeSlot circuit breakers of the host runtime
// (sf_degrade.hip): the rule loader, sf_degrade_submit, sf_read_breaker.
#include "sf_host.h"

extern "C" {

// the scratch size of the work set (sf_worksets.h) as rocPRIM states it
static int dg_temp_query(uint32_t n, uint32_t key_bits, size_t* bytes) { HIP_TRY(dg_sort_bytes(n, key_bits, bytes)); return SF_OK; }

// DegradeRule.equals (DegradeRule.java:153-164, AbstractRule.equals :76-93):
// resource, limitApp (always "default" here) and the six fields, doubles by
// Double.compare (bit pattern; every NaN equal).
static bool dg_same_double(double a, double b) {
    if (a != a && b != b) return true;
    int64_t x, y;
    std::memcpy(&x, &a, 8); std::memcpy(&y, &b, 8);
    return x == y;
}
static bool dg_rule_equal(const sf_degrade_rule& a, const sf_degrade_rule& b) {
    return a.resource == b.resource && a.grade == b.grade && dg_same_double(a.count, b.count) &&
           a.time_window_s == b.time_window_s && a.min_request_amount == b.min_request_amount &&
           dg_same_double(a.slow_ratio_threshold, b.slow_ratio_threshold) && a.stat_interval_ms == b.stat_interval_ms;
}

int sf_load_degrade_rules(sf_engine* e, const sf_degrade_rule* rules, uint32_t n, uint32_t* n_loaded) {
    if (!e || (n && !rules)) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(drain(e));
    // buildCircuitBreakers (DegradeRuleManager.java:236-265): valid rules, list order per resource.
    // Everything is built in locals first; the engine's tables are swapped only
    // after every check and allocation succeeded (a failed load keeps the old rules).
    std::vector<uint32_t> loc, valid;
    for (uint32_t i = 0; i < n; i++) {
        if (!dg_valid(rules[i])) continue;
        uint32_t l;
        if (!local_of(e, rules[i].resource, &l)) return fail(SF_ERR_INVALID, "degrade rule resource outside this shard");
        valid.push_back(i);
        loc.push_back(l);
    }
    const uint32_t nv = (uint32_t)valid.size();
    std::vector<uint32_t> order(nv);
    for (uint32_t i = 0; i < nv; i++) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return loc[a] < loc[b]; });
    std::vector<uint32_t> rr_of(e->R, 0), off;
    std::vector<DevBreakerRule> dr(nv);
    std::vector<sf_breaker_state> st(nv);
    std::vector<uint32_t> pos(nv, 0);
    uint32_t n_rres = 0;
    for (uint32_t p = 0; p < nv; p++) {
        const uint32_t v = order[p];
        if (p == 0 || loc[order[p - 1]] != loc[v]) {
            off.push_back(p);
            n_rres++;
        }
        if (p - off.back() >= SF_MAX_BREAKERS_PER_RESOURCE)
            return fail(SF_ERR_UNSUPPORTED, "more than SF_MAX_BREAKERS_PER_RESOURCE degrade rules on one resource");
        const sf_degrade_rule& r = rules[valid[v]];
        dr[p] = make_dev_breaker_rule(r);
        st[p] = sf_breaker_state{SF_CB_CLOSED, 0, 0, DG_WS_NONE, 0, 0};
        pos[v] = p;
    }
    off.push_back(nv);
    for (auto& x : rr_of) x = n_rres;
    for (uint32_t k = 0; k < n_rres; k++) rr_of[loc[order[off[k]]]] = k;
    // getExistingSameCbOrNew (DegradeRuleManager.java:151-163): a rule equal to
    // one of the resource's current breakers keeps that breaker and its state.
    // The reference hands the SAME breaker object to two equal new rules of one
    // resource; that aliasing is refused rather than approximated.
    if (nv && !e->dg.rules.empty()) {
        std::vector<sf_breaker_state> old(e->dg.rules.size());
        for (size_t k = 0; k < old.size(); k++)
            HIP_TRY(hipMemcpy(&old[k], e->dg.dev.state + e->dg.pos[k], sizeof(sf_breaker_state), hipMemcpyDeviceToHost));
        std::vector<uint8_t> taken(old.size(), 0);
        for (uint32_t v = 0; v < nv; v++) {
            const sf_degrade_rule& r = rules[valid[v]];
            for (size_t k = 0; k < old.size(); k++) {
                if (!dg_rule_equal(r, e->dg.rules[k])) continue;
                if (taken[k])
                    return fail(SF_ERR_UNSUPPORTED, "two equal degrade rules would share one existing breaker");
                taken[k] = 1;
                st[pos[v]] = old[k];
                break;
            }
        }
    }
    uint32_t *d_rr = nullptr, *d_off = nullptr;
    DevBreakerRule* d_rules = nullptr;
    sf_breaker_state* d_st = nullptr;
    DevPool fresh{HIP_MEM};                    // (the new tables, freed by an early return)
    SF_TRY(fresh.alloc(&d_rr, nz((size_t)e->R * 4)));
    SF_TRY(fresh.alloc(&d_off, nz(off.size() * 4)));
    SF_TRY(fresh.alloc(&d_rules, nz((size_t)nv * sizeof(DevBreakerRule))));
    SF_TRY(fresh.alloc(&d_st, nz((size_t)nv * sizeof(sf_breaker_state))));
    HIP_TRY(hipMemcpy(d_rr, rr_of.data(), (size_t)e->R * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_off, off.data(), off.size() * 4, hipMemcpyHostToDevice));
    if (nv) HIP_TRY(hipMemcpy(d_rules, dr.data(), (size_t)nv * sizeof(DevBreakerRule), hipMemcpyHostToDevice));
    if (nv) HIP_TRY(hipMemcpy(d_st, st.data(), (size_t)nv * sizeof(sf_breaker_state), hipMemcpyHostToDevice));
    e->pool.release_all(e->dg.dev.rr_of, e->dg.dev.off, e->dg.dev.rules, e->dg.dev.state);
    e->pool.adopt(fresh);
    e->dg.dev = DegradeDev{};
    e->dg.dev.rr_of = d_rr; e->dg.dev.off = d_off; e->dg.dev.rules = d_rules; e->dg.dev.state = d_st;
    e->dg.dev.n_rres = n_rres;
    // DegradeSlot inside sf_submit's chain (sf_decide.h decide_segment)
    e->st.dg_rr_of = n_rres ? d_rr : nullptr;
    e->st.dg_off = d_off; e->st.dg_rules = d_rules; e->st.dg_state = d_st; e->st.dg_n = n_rres;
    e->dg.pos = pos;
    e->dg.rules.clear();
    for (uint32_t v = 0; v < nv; v++) e->dg.rules.push_back(rules[valid[v]]);
    uint32_t kb = 1;
    while ((1ull << kb) <= n_rres) kb++;                        // keys 0..n_rres (n_rres = no breaker)
    e->dg.dev.key_bits = kb;
    dg_drop_sort_tmp(e->dg.ws);                                   // re-sized for the new key width
    {   // the routing summary reads dg_rr_of
        hipError_t re = launch_rdesc(e->st, e->stream);
        if (re == hipSuccess) re = hipStreamSynchronize(e->stream);
        if (re != hipSuccess) return fail(SF_ERR_DEVICE, std::string("rdesc: ") + hipGetErrorString(re));
    }
    if (n_loaded) *n_loaded = nv;
    return SF_OK;
}

int sf_degrade_submit(sf_engine* e, const sf_event_batch* in, sf_verdicts* out) {
    if (!e || !in || !out || !out->status) return fail(SF_ERR_INVALID, "null argument");
    if (in->n == 0) return SF_OK;
    if (!in->res_id || !in->ts_ms || !in->flags) return fail(SF_ERR_INVALID, "missing event array");
    if (in->n > e->cfg.max_batch) return fail(SF_ERR_CAPACITY, "batch larger than max_batch");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(drain(e));
    const uint32_t n = in->n;
    SF_TRY(dg_work_ensure(e->dg.ws, n, e->dg.dev.n_rres, e->dg.dev.key_bits, dg_temp_query));
    hipStream_t s = e->stream;
    DegradeBatch b{};
    b.n = n; b.shard_count = e->cfg.shard_count; b.shard_index = e->cfg.shard_index; b.R = e->R;
    b.last_ts = e->st.last_ts;
    // AuthoritySlot precedes DegradeSlot: entries the loaded rules block are marked first
    const bool auth = e->auth.of && in->origin;
    uint8_t* status = nullptr;
    uint16_t* rule = nullptr;
    int32_t* wait = nullptr;
    const uint32_t* origin = nullptr;
    StagePlan plan(in->mem == SF_MEM_HOST, out->mem == SF_MEM_HOST);
    plan.in(true, &b.res, in->res_id, (size_t)n * 4); plan.in(true, &b.ts, in->ts_ms, (size_t)n * 8);
    plan.in(true, &b.flags, in->flags, n);
    plan.in(in->entry_ref != nullptr, &b.eref, in->entry_ref, (size_t)n * 8);
    plan.in(in->create_ts != nullptr, &b.cts, in->create_ts, (size_t)n * 8);
    plan.out(true, &status, out->status, n);
    plan.out(out->rule_idx != nullptr, &rule, out->rule_idx, (size_t)n * 2);
    plan.out(out->wait_ms != nullptr, &wait, out->wait_ms, (size_t)n * 4);
    plan.in(auth, &origin, in->origin, (size_t)n * 4);
    SF_TRY(e->dg.stage.reserve(e->pool, plan.size()));
    plan.bind(e->dg.stage.p);
    SF_TRY(plan.upload(h2d_on(s)));
    if (auth) {                                  // (drained: the slot's array is free)
        Slot& sl = e->slot[e->cur];
        SF_TRY(slot_aflags(e, sl));
        HIP_TRY(launch_auth_mark(e->auth, b.res, origin, b.flags, n, (uint8_t)(SF_EV_BLOCKED | EVF_AUTH), sl.aflags, s));
        b.flags = sl.aflags;
        b.marked = 1;
    }
    HIP_TRY(hipMemsetAsync(e->dg.ws.w.err, 0, 4, s));
    HIP_TRY(dg_launch(e->dg.dev, e->dg.ws.w, b, status, rule, wait, s));
    int err = 0;
    HIP_TRY(hipMemcpyAsync(&err, e->dg.ws.w.err, 4, hipMemcpyDeviceToHost, s));
    SF_TRY(plan.download(d2h_on(s)));
    HIP_TRY(hipStreamSynchronize(s));
    if (err & 1) return fail(SF_ERR_INVALID, "event resource outside this shard");
    if (err & 2) return fail(SF_ERR_INVALID, "EXIT without a valid entry_ref or create_ts");
    if (err & 4) return fail(SF_ERR_INVALID, "event times must be non-decreasing (within and across batches)");
    return SF_OK;
}

int sf_read_breaker(sf_engine* e, uint32_t k, sf_breaker_state* out) {
    if (!e || !out) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    if (k >= e->dg.pos.size()) return fail(SF_ERR_INVALID, "breaker index");
    HIP_TRY(hipMemcpy(out, e->dg.dev.state + e->dg.pos[k], sizeof *out, hipMemcpyDeviceToHost));
    if (out->window_start == DG_WS_NONE) out->window_start = SF_WS_ABSENT;
    return SF_OK;
}

}  // extern "C"
