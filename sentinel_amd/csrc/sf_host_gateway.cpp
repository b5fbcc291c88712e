// sf_host_gateway.cpp -- API-gateway flow rules of the host runtime
// (sf_gateway.h, sf_gateway.hip): sf_load_gateway_rules keeps the converted
// rules as the gateway list of the ParamFlow stage and the parser's tables,
// sf_gateway_args parses a batch of requests into event columns.
#include "sf_host.h"

extern "C" {

uint64_t sf_gateway_string_bits(const uint8_t* bytes, uint32_t len) { return gw_hash(bytes, bytes ? len : 0); }

int sf_load_gateway_rules(sf_engine* e, const sf_gateway_rule* rules, uint32_t n, const uint32_t* str_off,
                          const uint8_t* bytes, uint32_t n_str) {
    if (!e || (n && !rules) || (n_str && (!str_off || (str_off[n_str] && !bytes))))
        return fail(SF_ERR_INVALID, "null argument");
    for (uint32_t s = 0; s < n_str; s++)
        if (str_off[s] > str_off[s + 1]) return fail(SF_ERR_INVALID, "pattern offsets decrease");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(drain(e));   // pending batches were sorted under the old rules
    for (uint32_t i = 0; i < n; i++) {
        uint32_t l;
        if (!local_of(e, rules[i].resource, &l)) return fail(SF_ERR_INVALID, "rule resource outside this shard");
    }
    std::vector<sf_param_rule> pr(n);
    std::vector<sf_hot_item> pi(n);
    std::vector<int32_t> slot(n);
    std::vector<sf_gateway_desc> desc(n);
    uint32_t n_pr = 0, n_pi = 0, n_d = 0;
    const int rc = sf_gateway_convert(rules, n, str_off, bytes, n_str, pr.data(), &n_pr, pi.data(), &n_pi, slot.data(),
                                      desc.data(), &n_d);
    if (rc == SF_ERR_UNSUPPORTED)
        return fail(rc, "gateway rules: a HashMap bin would be treeified (not modelled)");
    if (rc == SF_ERR_CAPACITY)
        return fail(rc, "gateway rules: a resource needs more than SF_MAX_ARGS slots or SF_MAX_RULES_PER_RESOURCE rules");
    if (rc != SF_OK) return fail(rc, "gateway rules: a pattern index outside the string table");
    pr.resize(n_pr); pi.resize(n_pi);
    // the parser's tables: the descriptor of each local resource, every pattern's bytes once per slot
    std::vector<uint32_t> of(e->R, GW_NONE);
    std::vector<GwDesc> gd(n_d);
    std::vector<uint8_t> pat;
    for (uint32_t k = 0; k < n_d; k++) {
        const sf_gateway_desc& d = desc[k];
        GwDesc& g = gd[k];
        g = GwDesc{};
        g.n_slots = d.n_slots; g.n_item = d.n_item_slots; g.gate = d.mode_gate;
        for (uint32_t a = 0; a < d.n_item_slots; a++) {
            const sf_gateway_slot& s = d.slot[a];
            GwSlot& o = g.slot[a];
            o.field_id = s.field_id; o.parse = s.parse_strategy; o.match = s.match_strategy;
            if (s.pattern != SF_GW_NONE && str_off[s.pattern + 1] != str_off[s.pattern]) {
                o.pat_off = (uint32_t)pat.size();
                o.pat_len = str_off[s.pattern + 1] - str_off[s.pattern];
                pat.insert(pat.end(), bytes + str_off[s.pattern], bytes + str_off[s.pattern + 1]);
            }
        }
        uint32_t l = 0;
        local_of(e, d.resource, &l);
        of[l] = k;
    }
    GwTables t{};
    DevPool fresh{HIP_MEM};                    // (the new tables, freed by an early return)
    if (n_d) {
        uint32_t* d_of = nullptr; GwDesc* d_desc = nullptr; uint8_t* d_pat = nullptr;
        SF_TRY(fresh.alloc(&d_of, nz(of.size() * 4)));
        SF_TRY(fresh.alloc(&d_desc, nz(gd.size() * sizeof(GwDesc))));
        SF_TRY(fresh.alloc(&d_pat, nz(pat.size())));
        HIP_TRY(hipMemcpy(d_of, of.data(), of.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_desc, gd.data(), gd.size() * sizeof(GwDesc), hipMemcpyHostToDevice));
        if (!pat.empty()) HIP_TRY(hipMemcpy(d_pat, pat.data(), pat.size(), hipMemcpyHostToDevice));
        t.of = d_of; t.desc = d_desc; t.pat = d_pat;
    }
    // both lists of the ParamFlow stage again: the new gateway list, the param list as loaded
    SF_TRY(install_param_rules(e, pr, pi, e->host_prules.data(), (uint32_t)e->host_prules.size(), e->host_pitems.data(),
                               (uint32_t)e->host_pitems.size()));
    e->gw.rules.swap(pr);
    e->gw.items.swap(pi);
    e->pool.release_all(e->gw.t.of, e->gw.t.desc, e->gw.t.pat);
    e->pool.adopt(fresh);
    e->gw.t = t;
    return SF_OK;
}

int sf_gateway_args(sf_engine* e, const sf_gateway_batch* in, sf_gateway_events* out) {
    if (!e || !in || !out) return fail(SF_ERR_INVALID, "null argument");
    if (in->mem != out->mem) return fail(SF_ERR_INVALID, "sf_gateway_args: the batch and the event columns must be in one memory form");
    const uint32_t n = in->n, n_total = out->n_total, n_exit = out->n_exit;
    if (n_exit && (!out->exit_pos || !out->entry_ref)) return fail(SF_ERR_INVALID, "missing exit_pos / entry_ref");
    if (n == 0) return n_exit ? fail(SF_ERR_INVALID, "exit_pos without a gateway entry in the batch") : SF_OK;
    if (!in->ts_ms || !in->count || !in->flags || !in->res_off || !in->val_off || !in->ev_index || (in->n_str && !in->str_off))
        return fail(SF_ERR_INVALID, "missing request array");
    if (!out->res_id || !out->ts_ms || !out->count || !out->flags || !out->n_args || !out->arg_tag || !out->arg_bits)
        return fail(SF_ERR_INVALID, "missing event column");
    const uint32_t cap = e->cfg.max_batch;
    if (n > cap || n_total > cap || n_exit > cap) return fail(SF_ERR_CAPACITY, "more requests, events or exits than max_batch");
    const bool host = in->mem == SF_MEM_HOST;
    std::lock_guard<std::mutex> lk(e->mu);
    hipStream_t s = e->stream;
    if (!e->gw.len) SF_TRY(e->pool.alloc(&e->gw.len, 32));
    // an error word of its own: batches in flight report through the engine's
    int32_t* d_err = (int32_t*)(e->gw.len + 4);
    GwBatch b{};
    b.n = n; b.n_str = in->n_str; b.n_exit = n_exit; b.n_total = n_total;
    uint32_t n_bytes = 0;
    // the lengths of the tables are their last offsets: read in place, or gathered on the device for one copy
    if (host) {
        b.n_ent = in->res_off[n]; b.n_val = in->val_off[n]; n_bytes = in->n_str ? in->str_off[in->n_str] : 0;
    } else {
        uint32_t zero = 0;                      // (a batch without strings has no str_off)
        b.res_off = in->res_off; b.val_off = in->val_off; b.str_off = in->n_str ? in->str_off : e->gw.len + 3;
        if (!in->n_str) HIP_TRY(hipMemcpyAsync(e->gw.len + 3, &zero, 4, hipMemcpyHostToDevice, s));
        uint32_t len[3] = {0, 0, 0};
        HIP_TRY(gw_lengths(b, e->gw.len, s));
        HIP_TRY(hipMemcpyAsync(len, e->gw.len, sizeof len, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        b.n_ent = len[0]; b.n_val = len[1]; n_bytes = len[2];
    }
    if (b.n_ent > cap) return fail(SF_ERR_CAPACITY, "more gateway entries than max_batch");
    if (n_bytes >= (1u << 31)) return fail(SF_ERR_CAPACITY, "gateway strings must be < 2^31 bytes");
    if ((b.n_ent && (!in->res_id || !in->res_mode)) || (b.n_val && (!in->val_field || !in->val_str)) || (n_bytes && !in->bytes))
        return fail(SF_ERR_INVALID, "missing request array");
    const size_t nt = n_total, ne = b.n_ent, nv = b.n_val, ns = b.n_str;
    GwOut o{};
    StagePlan plan(host, host);
    plan.in(true, &b.ts, in->ts_ms, (size_t)n * 8); plan.in(true, &b.count, in->count, (size_t)n * 4);
    plan.in(true, &b.flags, in->flags, n); plan.in(true, &b.res_off, in->res_off, ((size_t)n + 1) * 4);
    plan.in(true, &b.res_id, in->res_id, ne * 4); plan.in(true, &b.res_mode, in->res_mode, ne * 4);
    plan.in(true, &b.val_off, in->val_off, ((size_t)n + 1) * 4); plan.in(true, &b.val_field, in->val_field, nv * 4);
    plan.in(true, &b.val_str, in->val_str, nv * 4); plan.in(in->val_flags != nullptr, &b.val_flags, in->val_flags, nv);
    plan.in(ns != 0, &b.str_off, in->str_off, (ns + 1) * 4); plan.in(true, &b.bytes, in->bytes, n_bytes);
    plan.in(true, &b.ev_index, in->ev_index, (size_t)n * 4);
    plan.in(n_exit != 0, &b.entry_ref, out->entry_ref, nt * 8); plan.in(n_exit != 0, &b.exit_pos, out->exit_pos, (size_t)n_exit * 4);
    plan.inout(true, &o.res_id, out->res_id, nt * 4); plan.inout(true, &o.ts, out->ts_ms, nt * 8);
    plan.inout(true, &o.count, out->count, nt * 4); plan.inout(true, &o.flags, out->flags, nt);
    plan.inout(true, &o.n_args, out->n_args, nt); plan.inout(true, &o.arg_tag, out->arg_tag, nt * SF_MAX_ARGS);
    plan.inout(true, &o.arg_bits, out->arg_bits, nt * SF_MAX_ARGS * 8);
    SF_TRY(e->gw.stage.reserve(e->pool, std::max<size_t>(plan.size(), 16)));
    SF_TRY(e->gw.own.reserve(e->pool, std::max<size_t>(nt, 1) * 4));
    plan.bind(e->gw.stage.p);
    SF_TRY(plan.upload(h2d_on(s)));
    GwTables t = e->gw.t;
    t.R = e->R; t.shard_count = e->cfg.shard_count; t.shard_index = e->cfg.shard_index;
    HIP_TRY(hipMemsetAsync(d_err, 0, sizeof(int32_t), s));
    int32_t err = 0;
    const hipError_t le = gw_launch(t, b, o, (uint32_t*)e->gw.own.p, d_err, &err, s);
    if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("gateway launch: ") + hipGetErrorString(le));
    if (err)
        return fail(err, "malformed gateway batch (offsets start at 0 and must not decrease, string indices must be < n_str, "
                         "event ranges must not overlap or pass n_total, resources must be this shard's, an exit_pos must "
                         "refer to a gateway entry of the batch)");
    if (host) SF_TRY(plan.download(d2h_on(s)));
    HIP_TRY(hipStreamSynchronize(s));
    return SF_OK;
}

}  // extern "C"
