// embedded_check.cpp -- TEST ONLY: the engine's host-compilable embedded token
// server path (sentinel_amd/csrc/sf_token.h emb_request / flow_decide /
// lim_try_pass, sf_xflow.h xg_event with EMB) against case files the Python
// model wrote (tests/embedded_model.py), run under ASan + UBSan by
// tests/test_embedded_check.py.  Every table is a heap block of exactly its
// size, so an index past a table is an AddressSanitizer report.
//
// All events of a batch are replayed as ONE xflow group segment in submission
// order: what one lane of k_decide_x does for a group (how resources are
// grouped is the GPU suite's subject).  Compared: every verdict, wait_ms and
// rule_idx, every resource's ClusterNode and the seven ClusterMetric sums.
//
// Input (whitespace separated):
//   CFG S interval occupy_timeout max_rt cold_factor exceed_count max_occupy_ratio R
//   NS n   { id connected max_qps }
//   CR n   { flow_id count threshold_type ns_id S I }
//   FR n   { resource grade count behavior max_queue cluster limit_app fallback }
//   BIND n { rule_index flow_id }
//   BATCH n { res ts count flags entry_ref  status wait rule }      (any number of batches)
//   NODE res present threads { S x (ws pass block exc succ rt occ min_rt bor_ws bor_pass) } { 60 x (8 values) }
//   SUM flow_id now s0..s6
// Output: "ok <events> <nodes> <sums>" or one line per mismatch, exit 1.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#include "../sentinel_amd/csrc/sf_xflow.h"

using namespace sf;

template <class T> static std::unique_ptr<T[]> block(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]()); }

struct Check {
    DevState st{};
    EmbState emb{};
    uint32_t R = 0;
    int S = 2;
    std::unique_ptr<Bucket[]> second, minute;
    std::unique_ptr<Borrow[]> borrow;
    std::unique_ptr<int64_t[]> threads, bind;
    std::unique_ptr<uint32_t[]> rule_off, prule_off;
    std::unique_ptr<DevRule[]> rules;
    std::unique_ptr<DevRuleState[]> rstate;
    std::unique_ptr<DevParamRule[]> prules;
    std::unique_ptr<DevHotItem[]> items;
    std::unique_ptr<uint8_t[]> pm_init;
    std::unique_ptr<ParamSlot[]> ptab;
    std::unique_ptr<ClRule[]> crules;
    std::unique_ptr<ClFlowState[]> fstate;
    std::unique_ptr<IdSlot[]> idtab;
    std::unique_ptr<ClNs[]> ns;
    std::unique_ptr<LimState[]> lim;
    int32_t err = 0;
};

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: embedded_check case.txt\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string tag;
    Check c;
    long bad = 0, n_events = 0, n_nodes = 0, n_sums = 0;
    int cold = 3;
    std::vector<sf_namespace> nsv;
    std::vector<sf_cluster_flow_rule> crv;
    std::vector<sf_flow_rule> frv;
    bool built = false;
    auto build = [&]() {                                    // the tables of the engine, as its loads build them
        built = true;
        DevState& st = c.st;
        const size_t R = c.R, S = (size_t)c.S;
        c.second = block<Bucket>(R * S); c.borrow = block<Borrow>(R * S); c.minute = block<Bucket>(R * MINUTE);
        for (size_t i = 0; i < R * S; i++) { c.second[i] = fresh_bucket(WS_NONE, st.max_rt); c.borrow[i] = Borrow{WS_NONE, 0}; }
        for (size_t i = 0; i < R * MINUTE; i++) c.minute[i] = fresh_bucket(WS_NONE, st.max_rt);
        c.threads = block<int64_t>(R);
        c.rule_off = block<uint32_t>(R + 1); c.prule_off = block<uint32_t>(R + 1);
        std::vector<uint32_t> counts(R, 0);
        for (const sf_flow_rule& r : frv) counts[r.resource]++;
        for (size_t r = 0; r < R; r++) c.rule_off[r + 1] = c.rule_off[r] + counts[r];
        const size_t nr = frv.size();
        c.rules = block<DevRule>(nr); c.rstate = block<DevRuleState>(nr); c.bind = block<int64_t>(nr);
        std::vector<uint32_t> fill(c.rule_off.get(), c.rule_off.get() + R), pos(nr);
        for (size_t k = 0; k < nr; k++) {
            pos[k] = fill[frv[k].resource]++;
            c.rules[pos[k]] = make_dev_rule(frv[k], cold, (int)k, XNONE);
            c.rstate[pos[k]] = fresh_rule_state();
        }
        c.prules = block<DevParamRule>(1); c.items = block<DevHotItem>(1); c.pm_init = block<uint8_t>(R);
        c.ptab = block<ParamSlot>(16);
        st.R = (uint32_t)R; st.shard_count = 1;
        st.second = c.second.get(); st.borrow = c.borrow.get(); st.minute = c.minute.get(); st.threads = c.threads.get();
        st.rule_off = c.rule_off.get(); st.rules = c.rules.get(); st.rstate = c.rstate.get();
        st.prule_off = c.prule_off.get(); st.prules = c.prules.get(); st.items = c.items.get();
        st.pm_init = c.pm_init.get(); st.ptab = c.ptab.get(); st.pcap_mask = 15; st.err = &c.err;
        // the token server's tables (sf_host_cluster.cpp tok_rebuild)
        const size_t nf = crv.size(), nn = nsv.size();
        c.crules = block<ClRule>(nf); c.fstate = block<ClFlowState>(nf);
        c.ns = block<ClNs>(nn); c.lim = block<LimState>(nn);
        for (size_t i = 0; i < nn; i++) {
            c.ns[i] = ClNs{nsv[i].connected_count, nsv[i].max_allowed_qps >= 0, nsv[i].max_allowed_qps};
            for (int k = 0; k < LIM_S; k++) { c.lim[i].ws[k] = WS_NONE; c.lim[i].v[k] = 0; }
        }
        uint64_t cap = 16;
        while (cap < 2 * nf + 2) cap <<= 1;
        c.idtab = block<IdSlot>(cap);
        for (uint64_t i = 0; i < cap; i++) c.idtab[i] = IdSlot{0, -1, -1};
        for (size_t i = 0; i < nf; i++) {
            ClRule& r = c.crules[i];
            r = ClRule{};
            r.count = crv[i].count; r.flow_id = crv[i].flow_id; r.threshold_type = crv[i].threshold_type; r.ns = -1;
            for (size_t k = 0; k < nn; k++) if (nsv[k].namespace_id == crv[i].namespace_id) { r.ns = (int32_t)k; break; }
            r.S = crv[i].sample_count; r.interval = crv[i].window_interval_ms; r.wl = r.interval / r.S;
            for (int k = 0; k < CL_MAXS; k++) { c.fstate[i].b[k].ws = WS_NONE; }
            uint64_t h = id_hash(r.flow_id) & (cap - 1);
            while (c.idtab[h].id != 0 && c.idtab[h].id != r.flow_id) h = (h + 1) & (cap - 1);
            c.idtab[h].id = r.flow_id;
            if (c.idtab[h].flow < 0) c.idtab[h].flow = (int32_t)i;
        }
        TokState& ts = c.emb.ts;
        ts.n_flow = ts.n_rules = (uint32_t)nf; ts.n_ns = (uint32_t)nn;
        ts.rules = c.crules.get(); ts.fstate = c.fstate.get(); ts.idtab = c.idtab.get(); ts.id_mask = cap - 1;
        ts.ns = c.ns.get(); ts.lim = c.lim.get(); ts.err = &c.err; ts.shard_count = 1; ts.shard_index = 0;
        c.emb.bind = c.bind.get();
        st.emb = &c.emb;
        return pos;
    };
    std::vector<uint32_t> pos;
    while (in >> tag) {
        if (tag == "CFG") {
            DevState& st = c.st;
            in >> c.S >> st.interval >> st.occupy_timeout >> st.max_rt >> cold >> c.emb.ts.exceed_count >>
                c.emb.ts.max_occupy_ratio >> c.R;
            st.S = c.S; st.wl = st.interval / st.S;
            if (c.S < 1 || c.S > SF_MAX_SAMPLE_COUNT) { std::fprintf(stderr, "sample_count out of range\n"); return 2; }
        } else if (tag == "NS") {
            size_t n; in >> n; nsv.resize(n);
            for (auto& x : nsv) in >> x.namespace_id >> x.connected_count >> x.max_allowed_qps;
        } else if (tag == "CR") {
            size_t n; in >> n; crv.resize(n);
            for (auto& x : crv) in >> x.flow_id >> x.count >> x.threshold_type >> x.namespace_id >> x.sample_count >> x.window_interval_ms;
        } else if (tag == "FR") {
            size_t n; in >> n; frv.assign(n, sf_flow_rule{});
            for (auto& x : frv) {
                in >> x.resource >> x.grade >> x.count >> x.control_behavior >> x.max_queueing_time_ms >> x.cluster_mode >>
                    x.limit_app >> x.cluster_fallback;
                x.strategy = SF_STRATEGY_DIRECT; x.ref_resource = SF_REF_NONE; x.warm_up_period_sec = 10;
                if (x.resource >= c.R) { std::fprintf(stderr, "rule resource out of range\n"); return 2; }
            }
        } else if (tag == "BIND") {
            pos = build();
            size_t n; in >> n;
            for (size_t i = 0; i < n; i++) {
                uint32_t k; int64_t fid; in >> k >> fid;
                if (k >= frv.size()) { std::fprintf(stderr, "bind out of range\n"); return 2; }
                c.bind[pos[k]] = fid;
            }
        } else if (tag == "BATCH") {
            if (!built) { std::fprintf(stderr, "BATCH before BIND\n"); return 2; }
            uint32_t n; in >> n;
            auto res = block<uint32_t>(n), ident = block<uint32_t>(n);
            auto ts = block<int64_t>(n), eref = block<int64_t>(n), cts = block<int64_t>(n);
            auto cnt = block<int32_t>(n), vw = block<int32_t>(n), want_w = block<int32_t>(n);
            auto fl = block<uint8_t>(n), vs = block<uint8_t>(n), want_s = block<uint8_t>(n);
            auto vr = block<uint16_t>(n), want_r = block<uint16_t>(n);
            for (uint32_t i = 0; i < n; i++) {
                int f, s, r;
                in >> res[i] >> ts[i] >> cnt[i] >> f >> eref[i] >> s >> want_w[i] >> r;
                want_s[i] = (uint8_t)s; want_r[i] = (uint16_t)r;
                fl[i] = (uint8_t)(f & 0x0F);                                 // the sort's internal flags (k_keys)
                if ((f & (SF_EV_BLOCKED | SF_EV_EXIT)) == SF_EV_BLOCKED)
                    fl[i] |= EVF_SYSBLK | (uint8_t)(SYSR_OTHER << EVF_SYSREASON_SHIFT);
                ident[i] = i;
                if (res[i] >= c.R) { std::fprintf(stderr, "event resource out of range\n"); return 2; }
            }
            SegIO io{ts.get(), cnt.get(), fl.get(), eref.get(), cts.get(), 0, nullptr, nullptr, nullptr, n,
                     nullptr, nullptr, nullptr, vs.get(), vw.get(), vr.get()};
            io.perm = ident.get(); io.o_status = vs.get(); io.o_wait = vw.get(); io.o_rule = vr.get();
            io.ev_res = res.get(); io.ev_origin = nullptr; io.ev_ctx = nullptr; io.shard_count = 1;
            c.err = 0;
            if (c.S <= 2) decide_xgroup<2, true>(c.st, io, 0, n);           // the two instances of the device walks
            else decide_xgroup<SF_MAX_SAMPLE_COUNT, true>(c.st, io, 0, n);
            if (c.err) { std::printf("batch raised error %d\n", c.err); bad++; }
            for (uint32_t i = 0; i < n; i++, n_events++)
                if (vs[i] != want_s[i] || vw[i] != want_w[i] || vr[i] != want_r[i]) {
                    if (bad++ < 20)
                        std::printf("event %ld (res %u ts %lld): got (%u, %d, %u), the model (%u, %d, %u)\n", n_events, res[i],
                                    (long long)ts[i], vs[i], vw[i], vr[i], want_s[i], want_w[i], want_r[i]);
                }
        } else if (tag == "NODE") {
            uint32_t res; int present; int64_t thr;
            in >> res >> present >> thr;
            if (res >= c.R) { std::fprintf(stderr, "node out of range\n"); return 2; }
            auto abs = [](int64_t ws) { return ws == SF_WS_ABSENT ? WS_NONE : ws; };
            bool same = c.threads[res] == thr;
            auto bucket = [&](const Bucket& b) {
                int64_t v[8];
                for (auto& x : v) in >> x;
                if (abs(v[0]) != b.ws) { same = false; return; }
                if (b.ws == WS_NONE) return;
                same = same && v[1] == b.pass && v[2] == b.block && v[3] == b.exc && v[4] == b.succ && v[5] == b.rt &&
                       v[6] == b.occ && v[7] == b.min_rt;
            };
            for (int i = 0; i < c.S; i++) {
                bucket(c.second[(size_t)res * c.S + i]);
                int64_t bw, bp; in >> bw >> bp;
                const Borrow& b = c.borrow[(size_t)res * c.S + i];
                same = same && abs(bw) == b.ws && (b.ws == WS_NONE || bp == b.pass);
            }
            for (int i = 0; i < MINUTE; i++) bucket(c.minute[(size_t)res * MINUTE + i]);
            if (!same) { std::printf("node %u differs from the model\n", res); bad++; }
            n_nodes++;
        } else if (tag == "SUM") {
            int64_t fid, now, want[CE_COUNT];
            in >> fid >> now;
            for (auto& x : want) in >> x;
            const int32_t r = id_lookup(c.emb.ts, fid, false);
            for (int ev = 0; ev < CE_COUNT; ev++) {
                int64_t got = 0;
                if (r >= 0) {
                    const ClRule& rule = c.crules[r];
                    ClMetric m{&c.fstate[r], rule.S, rule.wl, rule.interval, rule.interval / 1000.0};
                    got = m.sum(ev, now);
                }
                if (got != want[ev]) {
                    std::printf("flowId %lld event %d: sum %lld, the model %lld\n", (long long)fid, ev, (long long)got, (long long)want[ev]);
                    bad++;
                }
            }
            n_sums++;
        } else {
            std::fprintf(stderr, "unknown record %s\n", tag.c_str());
            return 2;
        }
    }
    if (bad) return 1;
    std::printf("ok %ld %ld %ld\n", n_events, n_nodes, n_sums);
    return 0;
}
