// sf_engine.cpp — host runtime behind the C-ABI (include/sentinel_flow.h).
//
// Owns one GPU's shard of resource state in HBM, the rule tables and the
// batch pipeline: SF_SLOTS batches in flight (struct Slot) over the sort
// stream, the decide streams (`stream` and its fork / join streams 2-4), the
// ENTRY_NODE side stream of asynchronous batches and the packed path's two
// copy streams.  The entry points are serialised by a mutex (the Java shim
// batches from many threads into one flusher).  There is no
// CPU fallback: without a usable gfx950 device sf_create fails.
#include <functional>

#include "sf_host.h"

static thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

extern "C" {

int sf_abi_version(void) { return SF_ABI_VERSION; }
const char* sf_last_error(void) { return g_err.c_str(); }

void sf_config_default(sf_config* c) {
    std::memset(c, 0, sizeof *c);
    c->sample_count = 2; c->interval_ms = 1000; c->occupy_timeout_ms = 500; c->cold_factor = 3;
    c->statistic_max_rt = 5000; c->max_resources = 1024; c->max_batch = 1u << 20;
    c->param_capacity = 1u << 16; c->shard_count = 1; c->shard_index = 0; c->device = 0;
    c->cluster_sample_count = 10; c->cluster_interval_ms = 1000; c->exceed_count = 1.0;
    c->max_occupy_ratio = 1.0; c->max_flow_ids = 1024; c->aux_capacity = 65536;
}

// the events of a slot (the packed stage's are created with its copy streams, submit_packed)
static int slot_create(Slot& sl) {
    for (auto& x : sl.evs) HIP_TRY(hipEventCreate(&x));
    for (hipEvent_t* x : {&sl.sorted, &sl.done, &sl.end, &sl.core})
        HIP_TRY(hipEventCreateWithFlags(x, hipEventDisableTiming));
    return SF_OK;
}

// Teardown: the streams drain, the pools free their memory, then the
// communicator, the events and the streams go.  (A pool missing here would
// still be freed by its destructor, after the streams.)
void sf_destroy(sf_engine* e) {
    if (!e) return;
    for (hipStream_t x : {e->sstream, e->stream, e->h2d, e->d2h}) if (x) hipStreamSynchronize(x);
    for (Slot& sl : e->slot) { sl.wpool.clear(); sl.pkpool.clear(); }
    for (DevPool* p : {&e->pool, &e->user_dev, &e->user_host, &e->tok.tw.pool, &e->rls.ws.pool, &e->cc.ws.pool, &e->dg.ws.pool, &e->rep.ml_pool})
        p->clear();
    if (e->comm) ncclCommDestroy(e->comm);
    for (Slot& sl : e->slot) {
        const PkStage& p = sl.pk;
        for (hipEvent_t x : {p.h2d, p.d2h, p.consumed, sl.sorted, sl.done, sl.end, sl.core}) if (x) hipEventDestroy(x);
        for (hipEvent_t x : sl.evs) if (x) hipEventDestroy(x);
    }
    for (auto& x : e->rep.ml_ev) if (x) hipEventDestroy(x);
    if (e->ev_en) hipEventDestroy(e->ev_en);
    for (hipStream_t x : {e->h2d, e->d2h, e->stream, e->stream2, e->stream3, e->stream4, e->sstream}) if (x) hipStreamDestroy(x);
    if (e->enstream && e->en_own) hipStreamDestroy(e->enstream);
    delete e;
}

// One Work set: every sorted-order buffer of one batch (sf_internal.h).
static int work_fill(sf_engine* e, Work& w, DevPool& m) {
    const sf_config& c = e->cfg;
    const size_t N = c.max_batch, R = e->R;
    SF_TRY(m.alloc(&w.keys_in, nz(N * 4))); SF_TRY(m.alloc(&w.keys_out, nz(N * 4))); SF_TRY(m.alloc(&w.perm, nz(N * 4)));
    // (12-B payloads when the batch has origins)
    SF_TRY(m.alloc(&w.pv_in, nz(N * sizeof(PackedEvO)))); SF_TRY(m.alloc(&w.pv_out, nz(N * sizeof(PackedEvO))));
    SF_TRY(m.alloc(&w.err, nz(4)));
    SF_TRY(m.alloc(&w.head_scan, nz(N * 4)));
    SF_TRY(m.alloc(&w.seg_start, nz((N + 1) * 4))); SF_TRY(m.alloc(&w.seg_res, nz(N * 4))); SF_TRY(m.alloc(&w.n_seg, nz(4)));
    SF_TRY(m.alloc(&w.s_meta, nz(N * 4)));
    SF_TRY(m.alloc(&w.s_eref, nz(N * 8))); SF_TRY(m.alloc(&w.s_cts, nz(N * 8)));
    SF_TRY(m.alloc(&w.s_nargs, nz(N))); SF_TRY(m.alloc(&w.s_atag, nz(N * SF_MAX_ARGS))); SF_TRY(m.alloc(&w.s_abits, nz(N * SF_MAX_ARGS * 8)));
    SF_TRY(m.alloc(&w.v_status, nz(N))); SF_TRY(m.alloc(&w.v_wait, nz(N * 4))); SF_TRY(m.alloc(&w.v_rule, nz(N * 2)));
    if (query_temp_bytes((uint32_t)N, &w.sort_tmp_bytes) != hipSuccess) return fail(SF_ERR_DEVICE, "sort temp size query");
    SF_TRY(m.alloc(&w.sort_tmp, nz(w.sort_tmp_bytes)));
    // heavy / light split
    w.heavy_min = c.heavy_min_events ? c.heavy_min_events : 512;
    {
        int dev = 0, ncu = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) ncu = 256;
        w.stream_grid = 2u * (uint32_t)(ncu > 0 ? ncu : 256);
        w.fill_grid = 8u * (uint32_t)(ncu > 0 ? ncu : 256);
    }
    const size_t SC = std::min<size_t>(N, R) + 1;
    w.seg_cap = (uint32_t)SC;
    SF_TRY(m.alloc(&w.segflag, nz(SC * 4))); SF_TRY(m.alloc(&w.seg_mode, nz(SC))); SF_TRY(m.alloc(&w.lcounts, nz(2 * LCLS * 4)));
    {   // light_list regions per length class: class c holds segments of >= lo_len(c) events
        size_t off = 0;
        for (int k = 0; k < LCLS; k++) {
            const size_t lo_len = k == 0 ? 1 : (k == 1 ? 2 : ((size_t)1 << (k - 1)) + 1);
            const size_t cap = lo_len > w.heavy_min ? 0 : std::min<size_t>(SC, N / lo_len + 1);
            w.loff[k] = (uint32_t)off;
            w.lcap[k] = (uint32_t)cap;
            off += cap;
        }
        SF_TRY(m.alloc(&w.light_list, nz(off * 4)));
    }
    SF_TRY(m.alloc(&w.heavy_list, nz(SC * 4)));
    SF_TRY(m.alloc(&w.counters, nz(WC_COUNT * 4))); SF_TRY(m.alloc(&w.pcg, nz(N * 8))); SF_TRY(m.alloc(&w.segs_lb, nz(segs_lb_bytes((uint32_t)N))));
    // <= len/TILE + 2 tiles per heavy segment; a ParamFlow-only segment of more
    // than 32 events is heavy too (SM_PARAM, k_classify), whatever heavy_min
    w.fill_tile_cap = (uint32_t)(N / FILL_TILE + 2 * (N / (std::min<uint32_t>(w.heavy_min, 32u) + 1)) + 2);
    SF_TRY(m.alloc(&w.fill_tiles, nz((size_t)2 * w.fill_tile_cap * sizeof(uint2)))); SF_TRY(m.alloc(&w.fill_ntiles, nz(2 * 4)));
    w.acc_cap = (uint32_t)std::min<size_t>(std::max<size_t>(N / w.heavy_min * 64, 1 << 16), 1u << 24);
    SF_TRY(m.alloc(&w.acc_hw, nz((size_t)w.acc_cap * ACC_BYTES))); SF_TRY(m.alloc(&w.acc_sec, nz((size_t)w.acc_cap * ACC_BYTES)));
    SF_TRY(m.alloc(&w.acc_hw_base, nz(SC * 4))); SF_TRY(m.alloc(&w.acc_sec_base, nz(SC * 4))); SF_TRY(m.alloc(&w.seg_hw0, nz(SC * 8)));
    SF_TRY(m.alloc(&w.seg_sec0, nz(SC * 8))); SF_TRY(m.alloc(&w.seg_nhw, nz(SC * 4))); SF_TRY(m.alloc(&w.seg_nsec, nz(SC * 4)));
    SF_TRY(m.alloc(&w.hticks, nz((N / (w.heavy_min + 1) + 2) * 8)));
    SF_TRY(m.alloc(&w.sticks, nz((N / (w.heavy_min + 1) + 2) * 8)));
    SF_TRY(m.alloc(&w.stream_list, nz(SC * 4)));
    SF_TRY(m.alloc(&w.xw_list, nz((N / XW_MIN + 1) * 4)));
    SF_TRY(m.alloc(&w.xcl_list, nz((N / XW_MIN + 1) * 4)));
    SF_TRY(m.alloc(&w.passbits, nz((N / 64 + 2) * 8)));
    SF_TRY(m.alloc(&w.exit_of, nz(N * 4)));
    SF_TRY(m.alloc(&w.lxfar, nz((N / 64 + 2) * 8)));
    SF_TRY(m.alloc(&w.thr_rec, nz(N * 8)));
    SF_TRY(m.alloc(&w.tile_rc, nz((size_t)w.fill_tile_cap * 4))); SF_TRY(m.alloc(&w.seg_rb, nz(SC * 4))); SF_TRY(m.alloc(&w.seg_re, nz(SC * 4)));
    SF_TRY(m.alloc(&w.vs_cursor, nz(VS_CURSORS(N) * 4)));
    SF_TRY(m.alloc(&w.s_origin, nz(N * 4))); SF_TRY(m.alloc(&w.s_oslot, nz(N * 4))); SF_TRY(m.alloc(&w.ox_cnt, nz(8 * 4)));
    SF_TRY(m.alloc(&w.ox_bflags, nz((N / OX_TILE + 1) * 4))); SF_TRY(m.alloc(&w.ox_bseg, nz((N / OX_TILE + 1) * 8)));
    return SF_OK;
}

// (the slot is ready only with every buffer of its set; a failure leaves none)
static int alloc_work(sf_engine* e, Slot& sl) {
    const int rc = work_fill(e, sl.w, sl.wpool);
    if (rc) { sl.wpool.clear(); sl.w = Work{}; sl.aflags = nullptr; return rc; }
    sl.ready = true;
    return SF_OK;
}

static int create(sf_engine* e);
int sf_create(const sf_config* cfg, sf_engine** out) {
    if (!cfg || !out) return fail(SF_ERR_INVALID, "null argument");
    *out = nullptr;
    const sf_config& c = *cfg;
    if (c.sample_count <= 0 || c.sample_count > SF_MAX_SAMPLE_COUNT || c.interval_ms <= 0 ||
        c.interval_ms % c.sample_count != 0)
        return fail(SF_ERR_INVALID, "sample_count/interval_ms invalid (LeapArray.java:70-87)");
    if (c.max_resources == 0 || c.max_batch == 0) return fail(SF_ERR_INVALID, "max_resources/max_batch must be > 0");
    if (c.shard_count == 0 || c.shard_index >= c.shard_count) return fail(SF_ERR_INVALID, "bad shard");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(SF_ERR_DEVICE, "no HIP device visible: the engine has no CPU fallback");
    if (c.device < 0 || c.device >= ndev) return fail(SF_ERR_DEVICE, "device ordinal out of range");
    HIP_TRY(hipSetDevice(c.device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, c.device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SF_ERR_DEVICE, std::string("engine is built for gfx950, device is ") + prop.gcnArchName);

    sf_engine* e = new sf_engine();
    e->cfg = c;
    const int rc = create(e);              // (every failure past this point takes the engine with it)
    if (rc) { sf_destroy(e); return rc; }
    *out = e;
    return SF_OK;
}

static int create(sf_engine* e) {
    const sf_config& c = e->cfg;
    e->R = c.max_resources;
    while ((1ull << e->key_bits) < e->R) e->key_bits++;
    {   // stream priorities of the decide phase (SF_STREAM_PRIO, diagnostics):
        // 0 = the light lanes' stream C first, 1 = stream A (THREAD / RL chains) first
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        const char* pv = getenv("SF_STREAM_PRIO");
        const bool a_first = pv && pv[0] == '1';
        HIP_TRY(hipStreamCreateWithPriority(&e->stream, hipStreamNonBlocking, a_first ? greatest : least));
        HIP_TRY(hipStreamCreateWithFlags(&e->stream2, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithPriority(&e->stream3, hipStreamNonBlocking, a_first ? least : greatest));
        // the sort stream (batch k+1's sort phase runs beside batch k's decide phase)
        const char* ps = getenv("SF_SORT_PRIO");
        if (ps && ps[0] == '1') HIP_TRY(hipStreamCreateWithPriority(&e->sstream, hipStreamNonBlocking, greatest));
        else if (ps && ps[0] == '0') HIP_TRY(hipStreamCreateWithPriority(&e->sstream, hipStreamNonBlocking, least));
        else HIP_TRY(hipStreamCreateWithFlags(&e->sstream, hipStreamNonBlocking));
    }
    if (const char* v = getenv("SF_SERIAL_STREAMS")) e->serial = v[0] == '1';
    if (const char* v = getenv("SF_XCL_MIN")) e->xcl_min = std::max<uint32_t>(XW_MIN, (uint32_t)strtoul(v, nullptr, 10));
    if (const char* v = getenv("SF_RLS_WAVE")) if (v[0] == '0') e->rls.wave_min = UINT32_MAX;
    {   // the side stream of asynchronous batches: stream C, whose light lanes end
        // first (diagnostics SF_SIDE: 0 none -- on `stream` as before round 6 --,
        // 1 a stream of its own, 2 stream B, 3 stream C).  Same-box means of the
        // driver's step (tools/gpu_var.sh, 3-4 runs each): 13.32 / 13.65 / 13.24 /
        // 13.15 ms; a stream of its own is slower even with GPU_MAX_HW_QUEUES=8.
        const char* v = getenv("SF_SIDE");
        e->side_mode = v ? v[0] - '0' : 3;
        if (e->side_mode == 1) {
            HIP_TRY(hipStreamCreateWithFlags(&e->enstream, hipStreamNonBlocking));
            e->en_own = true;
        } else if (e->side_mode == 2) e->enstream = e->stream2;
        else if (e->side_mode == 3) e->enstream = e->stream3;
        else e->side_mode = 0;
    }
    HIP_TRY(hipEventCreateWithFlags(&e->ev_en, hipEventDisableTiming));
    for (Slot& sl : e->slot) SF_TRY(slot_create(sl));

    DevState& st = e->st;
    st.S = c.sample_count; st.wl = c.interval_ms / c.sample_count; st.interval = c.interval_ms;
    st.occupy_timeout = c.occupy_timeout_ms; st.max_rt = c.statistic_max_rt; st.R = e->R;
    st.shard_count = c.shard_count;
    const size_t R = e->R, S = c.sample_count;
    SF_TRY(e->pool.alloc(&st.second, nz(R * S * sizeof(Bucket))));
    SF_TRY(e->pool.alloc(&st.borrow, nz(R * S * sizeof(Borrow))));
    SF_TRY(e->pool.alloc(&st.minute, nz(R * MINUTE * sizeof(Bucket))));
    SF_TRY(e->pool.alloc(&st.threads, nz(R * sizeof(int64_t))));
    SF_TRY(e->pool.alloc(&st.rule_off, nz((R + 1) * sizeof(uint32_t))));
    SF_TRY(e->pool.alloc(&st.prule_off, nz((R + 1) * sizeof(uint32_t))));
    SF_TRY(e->pool.alloc(&st.pm_init, nz(R)));
    SF_TRY(e->pool.alloc(&st.rdesc, nz(R * sizeof(RDesc))));
    SF_TRY(e->pool.alloc(&st.prio_seen, nz(sizeof(int32_t))));
    SF_TRY(e->pool.alloc(&st.err, nz(sizeof(int32_t))));
    uint64_t pcap = 16;
    while (pcap < (uint64_t)c.param_capacity) pcap <<= 1;
    SF_TRY(e->pool.alloc(&st.ptab, nz(pcap * sizeof(ParamSlot))));
    st.pcap_mask = pcap - 1;
    HIP_TRY(hipMemsetAsync((void*)st.rule_off, 0, (R + 1) * sizeof(uint32_t), e->stream));
    HIP_TRY(hipMemsetAsync((void*)st.prule_off, 0, (R + 1) * sizeof(uint32_t), e->stream));
    HIP_TRY(hipMemsetAsync(st.pm_init, 0, R, e->stream));
    HIP_TRY(hipMemsetAsync((void*)st.rdesc, 0, R * sizeof(RDesc), e->stream));   // (= no rules)
    HIP_TRY(hipMemsetAsync(st.prio_seen, 0, sizeof(int32_t), e->stream));
    HIP_TRY(hipMemsetAsync(st.ptab, 0, pcap * sizeof(ParamSlot), e->stream));
    SF_TRY(e->pool.alloc(&st.pins, nz(256 * 16 * sizeof(unsigned int))));
    SF_TRY(e->pool.alloc(&st.xw_stats, nz(4 * sizeof(unsigned long long))));
    HIP_TRY(hipMemset(e->st.xw_stats, 0, 4 * sizeof(unsigned long long)));
    HIP_TRY(hipMemsetAsync(st.pins, 0, 256 * 16 * sizeof(unsigned int), e->stream));
    HIP_TRY(hipMemsetAsync(st.err, 0, sizeof(int32_t), e->stream));
    HIP_TRY(launch_init_state(st, e->stream));
    e->tok.ts.err = st.err;
    e->tok.ts.exceed_count = c.exceed_count;
    e->tok.ts.shard_count = c.shard_count; e->tok.ts.shard_index = c.shard_index;
    e->tok.ts.max_occupy_ratio = c.max_occupy_ratio;
    SF_TRY(e->pool.alloc(&e->tok.d_sum, nz(sizeof(int64_t))));
    SF_TRY(e->pool.alloc(&st.last_fetch, nz(R * sizeof(int64_t))));
    SF_TRY(e->pool.alloc(&st.last_ts, nz(sizeof(int64_t))));
    {
        const int64_t t_min = INT64_MIN;
        HIP_TRY(hipMemcpyAsync(st.last_ts, &t_min, 8, hipMemcpyHostToDevice, e->stream));
    }
    HIP_TRY(hipMemsetAsync(st.last_fetch, 0xff, R * sizeof(int64_t), e->stream));   // lastFetchTime = -1
    SF_TRY(e->pool.alloc(&e->en, nz(sizeof(EntryNode))));
    SF_TRY(e->pool.alloc(&e->en_acc, nz(sizeof(EntryAcc))));
    HIP_TRY(launch_entry_init(e->en, st.max_rt, e->stream));

    SF_TRY(alloc_work(e, e->slot[0]));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SF_OK;
}

extern "C++" int local_of(const sf_engine* e, uint32_t res, uint32_t* l) {
    if (res % e->cfg.shard_count != e->cfg.shard_index) return 0;
    *l = res / e->cfg.shard_count;
    return *l < e->R;
}

// Per-kernel device times of the batch last run in the slot (its events),
// added to the stats once, after that batch has completed.
static void acc_timing(sf_engine* e, Slot& sl) {
    if (!sl.timed) return;
    sl.timed = false;
    hipEvent_t* ev = sl.evs;
    float a = 0, b2 = 0, c = 0, d = 0;
    hipEventElapsedTime(&a, ev[EV_SORT_START], ev[EV_SORTED]);
    hipEventElapsedTime(&b2, ev[EV_SORTED], ev[EV_CLASSIFIED]);
    hipEventElapsedTime(&c, ev[EV_CLASSIFIED], ev[EV_JOINED]);
    hipEventElapsedTime(&d, ev[EV_JOINED], ev[EV_SCATTERED]);
    float cl = 0, li = 0, hd = 0, hf = 0, hs = 0;
    hipEventElapsedTime(&cl, ev[EV_CLASSIFY_START], ev[EV_CLASSIFIED]);
    hipEventElapsedTime(&li, ev[EV_FORK], ev[EV_LIGHT_DONE]);
    if (e->st.n_window_rules) {                    // the lean walks end on stream B
        float lq = 0;
        hipEventElapsedTime(&lq, ev[EV_FORK], ev[EV_LEAN_DONE]);
        li = std::max(li, lq);
    }
    hipEventElapsedTime(&hd, ev[EV_FORK], ev[EV_HEAVY_DECIDED]);
    hipEventElapsedTime(&hf, ev[EV_HEAVY_DECIDED], ev[EV_HEAVY_FILLED]);
    hipEventElapsedTime(&hs, ev[EV_STREAM_START], ev[EV_STREAM_DONE]);
    e->stats.classify_ms += cl; e->stats.light_ms += li;
    e->stats.heavy_decide_ms += hd; e->stats.heavy_fill_ms += hf; e->stats.stream_ms += hs;
    e->stats.sort_ms += a + b2;
    e->stats.decide_ms += c;
    e->stats.scatter_ms += d;
    e->stats.total_ms += a + b2 + c + d;
}

// a batch's error flag (Work::err, read back after the batch) as the call's result
static int batch_error(int err) {
    if (!err) return SF_OK;
    return fail(err, err == SF_ERR_CAPACITY ? "capacity exceeded (param table, or the origin / context node pool: aux_capacity)"
                                            : "invalid batch (resource outside shard or bad entry_ref)");
}

// order `stream` after the last asynchronous ENTRY_NODE update (every host
// call that reads or writes ENTRY_NODE on `stream` does this first)
extern "C++" int en_fence(sf_engine* e) {
    if (!e->en_async) return SF_OK;
    HIP_TRY(hipStreamWaitEvent(e->stream, e->ev_en, 0));
    e->en_async = false;
    return SF_OK;
}

static int sparse_complete(PkStage& pk);
// Drain asynchronously submitted batches: wait for both streams, then report
// the first error flag raised by any of them.  An async packed batch whose
// verdicts the caller has not collected keeps its error for its own
// sf_sync_packed, unless `all` (sf_sync: every batch collected here).
extern "C++" int drain(sf_engine* e, bool all) {
    if (e->en_async) { HIP_TRY(hipStreamSynchronize(e->enstream)); e->en_async = false; }
    if (!e->pending) return SF_OK;
    HIP_TRY(hipStreamSynchronize(e->sstream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->d2h) HIP_TRY(hipStreamSynchronize(e->d2h));
    for (Slot& sl : e->slot) sl.pk.d2h_pending = false;
    int first = 0;
    unsigned keep = 0;
    for (int k = 0; k < SF_SLOTS; k++) {
        if (!(e->pending & (1u << k))) continue;
        PkStage& pk = e->slot[k].pk;
        // an async packed batch whose verdicts the caller has not collected: its
        // error came back with them and is reported by its own sf_sync_packed
        if (pk.out_status && !all) { keep |= 1u << k; continue; }
        if (pk.out_status) {
            pk.out_status = nullptr;
            if (pk.sparse) SF_TRY(sparse_complete(pk));
        }
        int32_t err = 0;
        HIP_TRY(hipMemcpy(&err, e->slot[k].w.err, 4, hipMemcpyDeviceToHost));
        if (err && !first) first = err;
    }
    e->pending = keep;
    for (Slot& sl : e->slot) acc_timing(e, sl);
    uint32_t nseg = 0;
    HIP_TRY(hipMemcpy(&nseg, e->slot[e->last].w.n_seg, 4, hipMemcpyDeviceToHost));
    e->stats.n_segments = nseg;
    return batch_error(first);
}

// The origin / context node pool and its index table (sf_xflow.h,
// sf_origin.hip), allocated with the first batch with origins or the first
// rule that reads such nodes; the nodes live as long as the engine
// (ClusterNode.originCountMap / NodeSelectorSlot maps are never pruned).  The
// pool grows by chunks of AX_CHUNK nodes (no node moves) and the index table
// by rehashing into a larger one, both between batches, so that a batch never
// fails on their capacity.
static int chunk_init(sf_engine* e, const AuxChunk& c) {
    DevState pool = e->st;                     // fresh nodes: the resource-row initialiser on the chunk
    pool.second = c.sec; pool.borrow = c.bor; pool.minute = c.min; pool.threads = c.thr; pool.R = AX_CHUNK;
    const hipError_t le = launch_init_state(pool, e->stream);
    if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("aux init: ") + hipGetErrorString(le));
    HIP_TRY(hipMemcpyAsync(e->ax_dir + e->ax_host.size(), &c, sizeof c, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SF_OK;
}
static int pool_grow(sf_engine* e, uint64_t need) {
    DevState& st = e->st;
    const size_t S = st.S;
    if ((uint64_t)st.ax_cap >= need) return SF_OK;
    while ((uint64_t)st.ax_cap < need) {
        if (e->ax_host.size() >= AX_MAX_CHUNKS) return fail(SF_ERR_CAPACITY, "origin / context node pool at its limit");
        const size_t sec_b = (size_t)AX_CHUNK * S * sizeof(Bucket), bor_b = (size_t)AX_CHUNK * S * sizeof(Borrow);
        const size_t min_b = (size_t)AX_CHUNK * MINUTE * sizeof(Bucket), thr_b = (size_t)AX_CHUNK * sizeof(int64_t);
        char* m = nullptr;                     // (one allocation per chunk)
        SF_TRY(e->pool.alloc(&m, sec_b + bor_b + min_b + thr_b));
        const AuxChunk c{(Bucket*)m, (Borrow*)(m + sec_b), (Bucket*)(m + sec_b + bor_b), (int64_t*)(m + sec_b + bor_b + min_b)};
        const int rc = chunk_init(e, c);
        if (rc) { e->pool.release(m); return rc; }   // (not yet in the directory)
        e->ax_host.push_back(c);
        st.ax_cap += AX_CHUNK;
    }
    return SF_OK;
}

// Rebuild an open-addressed table (origin index or ParamFlow table) into a new
// one of at least `ncap` slots; a key that would land farther than
// PT_MAX_PROBE from its home slot makes k_ox_rehash raise its flag, and the
// rebuild is retried at twice the size (nothing in flight).
static int rehash_table(sf_engine* e, const ParamSlot* old, uint64_t old_n, uint64_t ncap,
                        ParamSlot** out, uint64_t* out_cap, const char* what) {
    if (!e->rh_err) SF_TRY(e->pool.alloc(&e->rh_err, sizeof(int32_t)));
    for (;; ncap *= 2) {
        DevPool fresh{HIP_MEM};                // (frees the new table on every path but the good one)
        ParamSlot* nt = nullptr;
        SF_TRY(fresh.alloc(&nt, ncap * sizeof(ParamSlot)));
        HIP_TRY(hipMemsetAsync(nt, 0, ncap * sizeof(ParamSlot), e->stream));
        HIP_TRY(hipMemsetAsync(e->rh_err, 0, sizeof(int32_t), e->stream));
        const hipError_t le = launch_ox_rehash(old, old_n, nt, ncap - 1, e->rh_err, e->stream);
        if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(le));
        int32_t flag = 0;
        HIP_TRY(hipMemcpyAsync(&flag, e->rh_err, sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (flag) continue;
        e->pool.adopt(fresh);
        *out = nt; *out_cap = ncap;
        return SF_OK;
    }
}

static int ensure_aux(sf_engine* e) {
    DevState& st = e->st;
    if (st.xtab) return SF_OK;
    const uint32_t cap = e->cfg.aux_capacity ? e->cfg.aux_capacity : 65536;
    uint64_t tcap = 16;
    while (tcap < 2ull * cap) tcap <<= 1;
    // (st.xtab says that the three exist: they reach the engine together or not at all)
    DevPool fresh{HIP_MEM};
    AuxChunk* dir = nullptr; uint32_t* count = nullptr; ParamSlot* tab = nullptr;
    SF_TRY(fresh.alloc(&dir, AX_MAX_CHUNKS * sizeof(AuxChunk)));
    SF_TRY(fresh.alloc(&count, sizeof(uint32_t)));
    SF_TRY(fresh.alloc(&tab, tcap * sizeof(ParamSlot)));
    HIP_TRY(hipMemsetAsync(count, 0, sizeof(uint32_t), e->stream));
    HIP_TRY(hipMemsetAsync(tab, 0, tcap * sizeof(ParamSlot), e->stream));
    e->pool.adopt(fresh);
    e->ax_dir = dir; st.ax_count = count; st.xtab = tab;
    st.xcap_mask = tcap - 1;
    st.ax_chunks = e->ax_dir;
    st.ax_cap = 0;
    return pool_grow(e, cap);
}

// the index table rebuilt with room for `need` keys at half load (nothing in flight)
static int index_grow(sf_engine* e, uint64_t need) {
    DevState& st = e->st;
    uint64_t tcap = (st.xcap_mask + 1) * 4;
    while (tcap < 2 * need) tcap <<= 1;
    ParamSlot* nt = nullptr;
    HIP_TRY(hipDeviceSynchronize());
    SF_TRY(rehash_table(e, st.xtab, st.xcap_mask + 1, tcap, &nt, &tcap, "index rehash"));
    e->pool.release(st.xtab);
    st.xtab = nt;
    st.xcap_mask = tcap - 1;
    e->aux_grows++;
    return SF_OK;
}

// The origin pass's three maps of a Work set (pool slot -> heavy id, heavy id
// -> slot, thread deltas): built in a scratch pool, installed together.
struct OxMaps { uint32_t* hmap = nullptr; uint32_t* hslot = nullptr; int64_t* thr = nullptr; };
static int ox_map_alloc(DevPool& fresh, size_t need, OxMaps& m) {
    SF_TRY(fresh.alloc(&m.hmap, need * 4));
    SF_TRY(fresh.alloc(&m.hslot, need * 4));
    return fresh.alloc(&m.thr, need * 8);
}
static void ox_map_install(Slot& sl, DevPool& fresh, const OxMaps& m, size_t n) {
    Work& w = sl.w;
    sl.wpool.release_all(w.ox_hmap, w.ox_hslot, w.ox_thr);
    sl.wpool.adopt(fresh);
    w.ox_hmap = m.hmap; w.ox_hslot = m.hslot; w.ox_thr = m.thr; w.ox_hmap_n = w.ox_hslot_n = n;
}
// the maps sized for the index table (every pool slot is below its
// capacity), the slot -> heavy id map reset to XNONE
static int ox_maps(sf_engine* e, Slot& sl, bool reset, hipStream_t ss) {
    Work& w = sl.w;
    const size_t need = (size_t)e->st.xcap_mask + 1;
    if (w.ox_hmap_n < need) {
        sl.wpool.release_all(w.ox_hmap, w.ox_hslot, w.ox_thr);      // (nothing to keep: freed first)
        w.ox_hmap_n = w.ox_hslot_n = 0;
        DevPool fresh{HIP_MEM};
        OxMaps m;
        SF_TRY(ox_map_alloc(fresh, need, m));
        ox_map_install(sl, fresh, m, need);
        reset = true;
    }
    if (reset) HIP_TRY(hipMemsetAsync(w.ox_hmap, 0xff, w.ox_hmap_n * 4, ss));
    return SF_OK;
}

// After the sort phase of a batch with origins (or with rules that read origin
// / context nodes): the index pass inserts every key the batch needs (growing
// the table and running again when it fills), then the pool grows to cover
// the new slots -- all before the decide phase, so nothing is ever dropped.
// The host waits for the sort stream here (the previous batch's decide phase
// keeps running).  Fills `plan` for the origin-node pass of the decide phase.
static int ox_prologue(sf_engine* e, Slot& sl, const DevBatch& b, hipStream_t ss) {
    Work& w = sl.w;
    SF_TRY(ensure_aux(e));
    // a batch that stopped between its index pass and its origin apply (an
    // early error return) left its heavy ids in ox_hmap: reset them
    SF_TRY(ox_maps(e, sl, w.ox_dirty, ss));
    if (b.origin && !w.ox_pairs_cap) {             // (at most one pair per event)
        SF_TRY(sl.wpool.alloc(&w.ox_pairs, (size_t)e->cfg.max_batch * sizeof(uint4)));
        const int rc = sl.wpool.alloc(&w.ox_plist, (size_t)e->cfg.max_batch * sizeof(uint32_t));
        if (rc) { sl.wpool.release(w.ox_pairs); return rc; }
        w.ox_pairs_cap = e->cfg.max_batch;
    }
    return SF_OK;
}
static int ox_launch_index(sf_engine* e, Work& w, const DevBatch& b, hipStream_t ss) {
    DevState stl = e->st;
    stl.err = w.err;
    const uint64_t xcap = e->st.xcap_mask + 1;
    const uint32_t lim = (uint32_t)std::min<uint64_t>(xcap * 7 / 10, 0xffffff00u);
    DevBatch bi = b;
    if (!w.s_origin || !b.origin) bi.origin = nullptr;
    w.ox_dirty = true;
    const hipError_t le = launch_ox_index(stl, w, bi, lim, ss);
    if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("origin index: ") + hipGetErrorString(le));
    return SF_OK;
}
// after the index passes (counts read): the pool covers every slot, the index
// stays at most half full, the plan of the origin-node pass
static int ox_plan(sf_engine* e, Slot& sl, const uint32_t* cnt, uint32_t ax, const int64_t* t01, OxPlan* plan) {
    Work& w = sl.w;
    SF_TRY(pool_grow(e, ax));
    // keep the index at most half full for the next batches
    if ((uint64_t)ax * 2 > e->st.xcap_mask + 1) {
        HIP_TRY(hipDeviceSynchronize());
        // (the Work set's hmap entries of this batch are slot-indexed: still valid after a rehash)
        const size_t old_n = w.ox_hmap_n;
        SF_TRY(index_grow(e, (uint64_t)ax * 2));
        if (w.ox_hmap_n < (size_t)e->st.xcap_mask + 1) {
            // regrow the maps keeping this batch's heavy ids
            const size_t need = (size_t)e->st.xcap_mask + 1;
            DevPool fresh{HIP_MEM};            // (the new maps, freed by an early return)
            OxMaps m;
            SF_TRY(ox_map_alloc(fresh, need, m));
            HIP_TRY(hipMemsetAsync(m.hmap, 0xff, need * 4, e->stream));
            HIP_TRY(hipMemcpyAsync(m.hmap, w.ox_hmap, old_n * 4, hipMemcpyDeviceToDevice, e->stream));
            HIP_TRY(hipMemcpyAsync(m.hslot, w.ox_hslot, old_n * 4, hipMemcpyDeviceToDevice, e->stream));
            HIP_TRY(hipStreamSynchronize(e->stream));
            ox_map_install(sl, fresh, m, need);
        }
    }
    plan->n_heavy = cnt[OXC_HEAVY];
    plan->n_pairs = cnt[OXC_PAIRS];
    const int64_t wl = e->st.wl;
    plan->win.w0s = t01[0] / wl; plan->win.w0m = t01[0] / 1000;
    plan->win.ws = (uint32_t)(t01[1] / wl - plan->win.w0s + 1);
    plan->win.wm = (uint32_t)(t01[1] / 1000 - plan->win.w0m + 1);
    const size_t acc_n = (size_t)plan->n_heavy * ((size_t)plan->win.ws + plan->win.wm);
    if (w.ox_acc_n < acc_n) {
        sl.wpool.release(w.ox_acc);
        w.ox_acc_n = 0;
        const size_t n2 = acc_n + acc_n / 4;
        SF_TRY(sl.wpool.alloc(&w.ox_acc, n2 * sizeof(OxAcc)));
        w.ox_acc_n = n2;
    }
    return SF_OK;
}
static int prepare_origins(sf_engine* e, Slot& sl, const DevBatch& b, hipStream_t ss, OxPlan* plan) {
    Work& w = sl.w;
    SF_TRY(ox_prologue(e, sl, b, ss));
    uint32_t cnt[8] = {0};
    uint32_t ax = 0;
    for (int round = 0;; round++) {
        SF_TRY(ox_launch_index(e, w, b, ss));
        HIP_TRY(hipMemcpyAsync(cnt, w.ox_cnt, sizeof cnt, hipMemcpyDeviceToHost, ss));
        HIP_TRY(hipMemcpyAsync(&ax, e->st.ax_count, 4, hipMemcpyDeviceToHost, ss));
        HIP_TRY(hipStreamSynchronize(ss));
        if (!cnt[OXC_OVERFLOW]) break;
        if (round > 12) return fail(SF_ERR_CAPACITY, "origin / context node index cannot grow");
        // no room for the keys: everything drains, the table grows to the keys
        // reserved (every absent key counted, by each workgroup that missed it),
        // the pass runs again
        HIP_TRY(hipDeviceSynchronize());
        SF_TRY(index_grow(e, std::max<uint64_t>((uint64_t)cnt[OXC_RESERVED], ax) * 3 / 2));
        SF_TRY(ox_maps(e, sl, true, ss));
    }
    int64_t t01[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&t01[0], b.ts, 8, hipMemcpyDeviceToHost, ss));
    HIP_TRY(hipMemcpyAsync(&t01[1], b.ts + (b.n - 1), 8, hipMemcpyDeviceToHost, ss));
    HIP_TRY(hipStreamSynchronize(ss));
    return ox_plan(e, sl, cnt, ax, t01, plan);
}


// The xflow groups (sf_xflow.h build_xmap / build_xw) and the embedded token
// server's tables (sf_token.h EmbState) from the host copies of the four loads
// they depend on: flow rules, binds, cluster rules, namespaces.  Whichever of
// those loads comes last calls this, so the groups do not depend on the order
// of the loads.  The caller holds e->mu and has drained.
extern "C++" int xgroups_rebuild(sf_engine* e) {
    const std::vector<DevRule>& dr = e->host_rules;
    const std::vector<uint32_t>& off = e->host_rule_off;
    if (off.empty()) return SF_OK;                                  // no flow rule load yet: nothing to group
    const bool emb = !e->binds.empty();
    std::vector<int64_t> bind;
    std::vector<int32_t> bind_ns;
    std::vector<uint8_t> bind_wave;              // the flowId is loaded and no limiter gates it (k_decide_xcl)
    // until the tables below are complete no walk may follow the old ones: a failure leaves the
    // engine without an embedded token server (unbound behaviour), never with stale pointers
    e->st.emb = nullptr;
    if (emb) {
        SF_TRY(tok_ready(e));
        bind.assign(std::max<size_t>(1, dr.size()), 0);
        bind_ns.assign(bind.size(), -1);
        bind_wave.assign(bind.size(), 0);
        for (const sf_cluster_bind& b : e->binds) {
            const int32_t pos = e->flow_csr_of[b.rule_index];
            bind[pos] = b.flow_id;
            // the first cluster flow rule of an id is the one looked up, the first namespace of an id
            // the one it counts in (tok_rebuild)
            for (const sf_cluster_flow_rule& f : e->tok.host_cflow) {
                if (f.flow_id != b.flow_id) continue;
                bind_wave[pos] = 1;
                for (size_t i = 0; i < e->tok.host_ns.size(); i++) {
                    if (e->tok.host_ns[i].namespace_id != f.namespace_id) continue;
                    if (e->tok.host_ns[i].max_allowed_qps >= 0) { bind_ns[pos] = (int32_t)i; bind_wave[pos] = 0; }
                    break;
                }
                break;
            }
        }
    }
    std::vector<uint32_t> xmap;
    const bool xflow = build_xmap(dr.data(), off.data(), e->R, xmap, emb ? bind.data() : nullptr,
                                  emb ? bind_ns.data() : nullptr);
    if (xflow) {
        SF_TRY(ensure_aux(e));
        if (!e->xmap_buf) SF_TRY(e->pool.alloc(&e->xmap_buf, (size_t)e->R * sizeof(uint32_t)));
        HIP_TRY(hipMemcpyAsync(e->xmap_buf, xmap.data(), (size_t)e->R * sizeof(uint32_t), hipMemcpyHostToDevice,
                               e->stream));
        std::vector<uint8_t> xw;
        build_xw(dr.data(), off.data(), e->R, xmap, xw, emb ? bind.data() : nullptr, emb ? bind_wave.data() : nullptr);
        if (!e->xw_buf) SF_TRY(e->pool.alloc(&e->xw_buf, (size_t)e->R));
        HIP_TRY(hipMemcpyAsync(e->xw_buf, xw.data(), (size_t)e->R, hipMemcpyHostToDevice, e->stream));
    }
    if (emb) {
        e->pool.release(e->emb_bind);
        SF_TRY(e->pool.alloc(&e->emb_bind, bind.size() * sizeof(int64_t)));
        HIP_TRY(hipMemcpyAsync(e->emb_bind, bind.data(), bind.size() * sizeof(int64_t), hipMemcpyHostToDevice, e->stream));
        if (!e->emb_dev) SF_TRY(e->pool.alloc(&e->emb_dev, sizeof(EmbState)));
        if (!e->emb_stats) SF_TRY(e->pool.alloc(&e->emb_stats, 2 * sizeof(unsigned long long)));
        HIP_TRY(hipMemsetAsync(e->emb_stats, 0, 2 * sizeof(unsigned long long), e->stream));
        const EmbState h{e->tok.ts, e->emb_bind, e->emb_stats, e->xcl_min, 0};
        HIP_TRY(hipMemcpyAsync(e->emb_dev, &h, sizeof h, hipMemcpyHostToDevice, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->st.xmap = xflow ? e->xmap_buf : nullptr;
    e->st.xw = xflow ? e->xw_buf : nullptr;
    e->st.emb = emb ? e->emb_dev : nullptr;
    // the wave walk's stream, created at the first table that routes to it and
    // after the pipeline's four (a stream created earlier changes which hardware
    // queue each of those gets: config 3 lost 2.3 ms/step to a shared queue)
    if (e->st.xw && !e->stream4) HIP_TRY(hipStreamCreateWithFlags(&e->stream4, hipStreamNonBlocking));
    return SF_OK;
}

int sf_load_flow_rules(sf_engine* e, const sf_flow_rule* rules, uint32_t n) {
    if (!e || (n && !rules)) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(drain(e));   // pending batches were sorted under the old rules
    std::vector<uint32_t> counts(e->R + 1, 0);
    std::vector<const sf_flow_rule*> valid;
    std::vector<uint32_t> valid_local, valid_ref;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t l;
        if (!local_of(e, rules[i].resource, &l)) return fail(SF_ERR_INVALID, "rule resource outside this shard");
        if (!valid_flow_rule(rules[i])) continue;
        uint32_t ref = XNONE;
        if (rules[i].strategy == SF_STRATEGY_RELATE && rules[i].ref_resource != SF_REF_NONE) {
            // RELATE reads refResource's ClusterNode: it must be decided by the same
            // engine (co-locate the pair); an id beyond this shard's
            // resources never gets a node (the rule passes)
            if (rules[i].ref_resource % e->cfg.shard_count != e->cfg.shard_index)
                return fail(SF_ERR_UNSUPPORTED, "RELATE refResource on another shard: co-locate it with the resource");
            const uint32_t rl = rules[i].ref_resource / e->cfg.shard_count;
            if (rl < e->R) ref = rl;
        }
        if (rules[i].control_behavior != SF_BEHAVIOR_DEFAULT && rules[i].grade == SF_GRADE_QPS &&
            e->cfg.cold_factor <= 1 &&
            (rules[i].control_behavior == SF_BEHAVIOR_WARM_UP || rules[i].control_behavior == SF_BEHAVIOR_WARM_UP_RATE_LIMITER))
            return fail(SF_ERR_INVALID, "Cold factor should be larger than 1 (WarmUpController.java:114-116)");
        if (++counts[l] > SF_MAX_RULES_PER_RESOURCE)
            return fail(SF_ERR_UNSUPPORTED, "more than SF_MAX_RULES_PER_RESOURCE rules on one resource");
        valid.push_back(&rules[i]);
        valid_local.push_back(l);
        valid_ref.push_back(ref);
    }
    std::vector<uint32_t> off(e->R + 1, 0);
    for (uint32_t r = 0; r < e->R; r++) off[r + 1] = off[r] + counts[r];
    std::vector<uint32_t> fill(off.begin(), off.end() - 1);
    std::vector<DevRule> dr(valid.size());
    std::vector<DevRuleState> ds(valid.size());
    // every check has passed: from here the tables move.  The binds name positions of the old rule
    // table, so they go first: a failure below leaves every cluster rule decided as unbound
    e->st.emb = nullptr;
    e->binds.clear();
    e->flow_pos.assign(valid.size(), 0);
    for (size_t k = 0; k < valid.size(); k++) {
        const sf_flow_rule& r = *valid[k];
        uint32_t pos = fill[valid_local[k]]++;
        e->flow_pos[k] = pos;
        DevRule d = make_dev_rule(r, e->cfg.cold_factor, (int32_t)k, valid_ref[k]);
        dr[pos] = d;
        ds[pos] = fresh_rule_state();
    }
    e->n_flow = (uint32_t)valid.size();
    {   // which segment classes the rules allow (launches of absent classes are skipped)
        uint32_t ns = 0, nw = 0;
        for (const DevRule& r : dr) {
            if (r.kind == CT_RATE_LIMITER || (r.kind == CT_DEFAULT && r.grade == SF_GRADE_THREAD)) ns++;
            if ((r.kind == CT_DEFAULT && r.grade == SF_GRADE_QPS) || r.kind == CT_WARM_UP) nw++;
        }
        e->st.n_stream_rules = ns; e->st.n_window_rules = nw;
    }
    e->pool.release_all(e->st.rules, e->st.rstate);
    SF_TRY(e->pool.alloc(&e->st.rules, std::max<size_t>(1, dr.size()) * sizeof(DevRule)));
    SF_TRY(e->pool.alloc(&e->st.rstate, std::max<size_t>(1, ds.size()) * sizeof(DevRuleState)));
    if (!dr.empty()) {
        HIP_TRY(hipMemcpyAsync((void*)e->st.rules, dr.data(), dr.size() * sizeof(DevRule), hipMemcpyHostToDevice, e->stream));
        HIP_TRY(hipMemcpyAsync(e->st.rstate, ds.data(), ds.size() * sizeof(DevRuleState), hipMemcpyHostToDevice, e->stream));
    }
    HIP_TRY(hipMemcpyAsync((void*)e->st.rule_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, e->stream));
    HIP_TRY(launch_rdesc(e->st, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    // the xflow groups; rule indices changed, so the binds of the embedded token server are gone
    e->host_rules = std::move(dr); e->host_rule_off = std::move(off);      // (uploaded and synchronised above)
    e->flow_csr_of.assign(n, -1); e->flow_cluster.assign(n, 0);
    for (size_t k = 0; k < valid.size(); k++) e->flow_csr_of[(size_t)(valid[k] - rules)] = (int32_t)e->flow_pos[k];
    for (uint32_t i = 0; i < n; i++) e->flow_cluster[i] = rules[i].cluster_mode != 0;
    e->binds.clear();
    return xgroups_rebuild(e);
}

// ParamFlowRule.equals of two loaded rules of one resource (their item lists as loaded)
static bool same_param_rule(const sf_param_rule& a, const sf_hot_item* ia, const sf_param_rule& b, const sf_hot_item* ib) {
    auto same_double = [](double x, double y) { return (x != x && y != y) || std::memcmp(&x, &y, 8) == 0; };
    if (!(a.resource == b.resource && a.grade == b.grade && a.param_idx == b.param_idx && same_double(a.count, b.count) &&
          a.control_behavior == b.control_behavior && a.max_queueing_time_ms == b.max_queueing_time_ms &&
          a.burst_count == b.burst_count && a.duration_in_sec == b.duration_in_sec && a.item_count == b.item_count))
        return false;
    for (uint32_t t = 0; t < a.item_count; t++) {
        const sf_hot_item &x = ia[a.item_offset + t], &y = ib[b.item_offset + t];
        if (x.tag != y.tag || x.bits != y.bits || x.count != y.count) return false;
    }
    return true;
}

// The ParamFlow tables of the device from the two lists a resource's ParamFlow
// stage walks: the gateway list (sf_load_gateway_rules; GatewayFlowSlot, order
// -4000) first, then the list of sf_load_param_rules (ParamFlowSlot, -3000).
// Nothing is changed before both lists are checked; the caller holds e->mu
// and has drained, and keeps the host copies of the lists.
extern "C++" int install_param_rules(sf_engine* e, const std::vector<sf_param_rule>& gw, const std::vector<sf_hot_item>& gwi,
                                     const sf_param_rule* rules, uint32_t n, const sf_hot_item* items, uint32_t n_items) {
    const uint32_t ng = (uint32_t)gw.size(), ngi = (uint32_t)gwi.size(), nt = ng + n;
    std::vector<uint32_t> counts(e->R + 1, 0), loc(nt);
    for (uint32_t i = 0; i < nt; i++) {
        const sf_param_rule& r = i < ng ? gw[i] : rules[i - ng];
        if (!local_of(e, r.resource, &loc[i])) return fail(SF_ERR_INVALID, "rule resource outside this shard");
        if (i >= ng && (uint64_t)r.item_offset + r.item_count > n_items) return fail(SF_ERR_INVALID, "hot item range");
        if (++counts[loc[i]] > SF_MAX_RULES_PER_RESOURCE)
            return ng ? fail(SF_ERR_CAPACITY, "more than SF_MAX_RULES_PER_RESOURCE gateway and param rules on one resource")
                      : fail(SF_ERR_UNSUPPORTED, "more than SF_MAX_RULES_PER_RESOURCE param rules on one resource");
    }
    for (uint32_t i = 0; i < ng; i++)
        for (uint32_t j = 0; j < n; j++)
            if (same_param_rule(gw[i], gwi.data(), rules[j], items))
                return fail(SF_ERR_UNSUPPORTED, "a converted gateway rule equals a param rule of its resource: "
                                                "they would share one ParameterMetric counter");
    std::vector<uint32_t> off(e->R + 1, 0);
    for (uint32_t r = 0; r < e->R; r++) off[r + 1] = off[r] + counts[r];
    std::vector<uint32_t> fill(off.begin(), off.end() - 1);
    std::vector<DevParamRule> dp(nt);
    for (uint32_t i = 0; i < nt; i++) {                        // (the gateway rules of a resource come first)
        DevParamRule d = i < ng ? make_dev_param_rule(gw[i], -1 - (int32_t)i) : make_dev_param_rule(rules[i - ng], (int32_t)(i - ng));
        if (i >= ng) d.item_off += (int32_t)ngi;
        dp[fill[loc[i]]++] = d;
    }
    std::vector<DevHotItem> di(ngi + n_items);
    for (uint32_t i = 0; i < ngi + n_items; i++) {
        const sf_hot_item& it = i < ngi ? gwi[i] : items[i - ngi];
        di[i].bits = it.bits; di[i].count = it.count; di[i].tag = it.tag;
    }
    e->n_prule = nt;
    e->st.n_prule = nt;
    e->pool.release_all(e->st.prules, e->st.items);
    SF_TRY(e->pool.alloc(&e->st.prules, std::max<size_t>(1, dp.size()) * sizeof(DevParamRule)));
    SF_TRY(e->pool.alloc(&e->st.items, std::max<size_t>(1, di.size()) * sizeof(DevHotItem)));
    if (nt) HIP_TRY(hipMemcpyAsync(e->st.prules, dp.data(), dp.size() * sizeof(DevParamRule), hipMemcpyHostToDevice, e->stream));
    if (!di.empty()) HIP_TRY(hipMemcpyAsync((void*)e->st.items, di.data(), di.size() * sizeof(DevHotItem), hipMemcpyHostToDevice, e->stream));
    HIP_TRY(hipMemcpyAsync((void*)e->st.prule_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, e->stream));
    // a rule reload drops all ParameterMetric state (new ParameterMetric per resource)
    HIP_TRY(hipMemsetAsync(e->st.pm_init, 0, e->R, e->stream));
    HIP_TRY(hipMemsetAsync(e->st.ptab, 0, (e->st.pcap_mask + 1) * sizeof(ParamSlot), e->stream));
    HIP_TRY(hipMemsetAsync(e->st.pins, 0, 256 * 16 * sizeof(unsigned int), e->stream));
    e->p_used = e->p_pending = 0;
    // keys one event (or one collection element) can insert: a rule key per rule
    // (ParameterMetric token / time maps) and a thread-count key per rule's index
    uint32_t kmax = 0;
    for (uint32_t r = 0; r < e->R; r++) kmax = std::max(kmax, counts[r]);
    e->p_kmax = 2ull * kmax;
    HIP_TRY(launch_rdesc(e->st, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SF_OK;
}

int sf_load_param_rules(sf_engine* e, const sf_param_rule* rules, uint32_t n, const sf_hot_item* items,
                        uint32_t n_items) {
    if (!e || (n && !rules) || (n_items && !items)) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(drain(e));   // pending batches were sorted under the old rules
    SF_TRY(install_param_rules(e, e->gw.rules, e->gw.items, rules, n, items, n_items));
    e->host_prules.assign(rules, rules + n);
    e->host_pitems.assign(items, items + n_items);
    return SF_OK;
}

// SystemRuleManager.loadSystemConf (SystemRuleManager.java:267-289) through
// SystemPropertyListener.configUpdate (:173-196): the minimum of every set
// threshold; checkSystemStatus follows the last rule, as in the reference.
int sf_load_system_rules(sf_engine* e, const sf_system_rule* rules, uint32_t n) {
    if (!e || (n && !rules)) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(drain(e));
    SysRule r{};
    r.qps = r.highest_load = r.highest_cpu = 1.7976931348623157e308;
    r.max_rt = r.max_thread = INT64_MAX;
    r.cur_load = e->sys.cur_load; r.cur_cpu = e->sys.cur_cpu;
    for (uint32_t i = 0; i < n; i++) {
        const sf_system_rule& x = rules[i];
        int check = 0;
        if (x.highest_system_load >= 0) { r.highest_load = std::fmin(r.highest_load, x.highest_system_load); r.load_set = 1; check = 1; }
        if (x.highest_cpu_usage >= 0 && x.highest_cpu_usage <= 1) {
            r.highest_cpu = std::fmin(r.highest_cpu, x.highest_cpu_usage); r.cpu_set = 1; check = 1;
        }
        if (x.avg_rt >= 0) { if (x.avg_rt < r.max_rt) r.max_rt = x.avg_rt; check = 1; }
        if (x.max_thread >= 0) { if (x.max_thread < r.max_thread) r.max_thread = x.max_thread; check = 1; }
        if (x.qps >= 0) { r.qps = std::fmin(r.qps, x.qps); check = 1; }
        r.check = check;
    }
    e->sys = r;
    return SF_OK;
}
// SystemStatusListener readings (system load average, cpu usage): fixed inputs of a replay
int sf_set_system_status(sf_engine* e, double avg_load, double cpu_usage) {
    if (!e) return fail(SF_ERR_INVALID, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    e->sys.cur_load = avg_load; e->sys.cur_cpu = cpu_usage;
    return SF_OK;
}

// ---------------------------------------------------------------- AuthorityRule (sf_authority.h)
// the slot's effective-flags array, with its Work set's pool
extern "C++" int slot_aflags(sf_engine* e, Slot& sl) {
    if (sl.aflags) return SF_OK;
    return sl.wpool.alloc(&sl.aflags, nz(e->cfg.max_batch));
}

// AuthorityRuleManager.loadAuthorityConf: the new tables are built on the host
// and in a scratch pool and adopted only when complete; until then the old map
// stays in force.
int sf_load_authority_rules(sf_engine* e, const sf_authority_rule* rules, uint32_t n, const uint32_t* apps,
                            uint32_t n_apps, uint32_t* n_loaded) {
    if (!e || (n && !rules)) return fail(SF_ERR_INVALID, "null argument");
    for (uint32_t i = 0; i < n; i++)
        if (rules[i].app_cnt && !apps) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(drain(e));   // pending batches were marked under the old rules
    AuthHost h;
    if (auth_build(rules, n, apps, n_apps, e->R, e->cfg.shard_count, e->cfg.shard_index, h) != SF_OK)
        return fail(SF_ERR_INVALID, "authority rule: app range outside apps[], or a resource beyond max_resources");
    AuthTables t{};
    t.R = e->R; t.shard_count = e->cfg.shard_count; t.shard_index = e->cfg.shard_index;
    DevPool fresh{HIP_MEM};                    // (the new tables, freed by an early return)
    if (!h.rule.empty()) {
        uint32_t *d_of = nullptr, *d_apps = nullptr;
        AuthRule* d_rule = nullptr;
        SF_TRY(fresh.alloc(&d_of, nz(h.of.size() * 4)));
        SF_TRY(fresh.alloc(&d_rule, nz(h.rule.size() * sizeof(AuthRule))));
        SF_TRY(fresh.alloc(&d_apps, nz(h.apps.size() * 4)));
        HIP_TRY(hipMemcpy(d_of, h.of.data(), h.of.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_rule, h.rule.data(), h.rule.size() * sizeof(AuthRule), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_apps, h.apps.data(), h.apps.size() * 4, hipMemcpyHostToDevice));
        for (Slot& sl : e->slot) SF_TRY(slot_aflags(e, sl));
        t.of = d_of; t.rule = d_rule; t.apps = d_apps;
    }
    e->pool.release_all(e->auth.of, e->auth.rule, e->auth.apps);
    e->pool.adopt(fresh);
    e->auth = t;
    if (n_loaded) *n_loaded = (uint32_t)h.rule.size();
    return SF_OK;
}

// The mark pass of one batch on stream s, after its staging or expansion: with
// rules loaded and origins in the batch, the slot's effective-flags array takes
// the place of the batch's flags (whole batch, indexed like it, so planner
// views, the degrade chain and the ENTRY_NODE update read it unchanged).  The
// caller has ordered s after the `end` of the slot's previous batch.
static int auth_apply(sf_engine* e, Slot& sl, DevBatch& b, hipStream_t s) {
    if (!e->auth.of || !b.origin || !b.n) return SF_OK;
    SF_TRY(slot_aflags(e, sl));
    HIP_TRY(launch_auth_mark(e->auth, b.res, b.origin, b.flags, b.n, (uint8_t)(SF_EV_BLOCKED | EVF_AUTH), sl.aflags, s));
    b.flags = sl.aflags;
    b.marked = 1;
    return SF_OK;
}

int sf_authority_mark(sf_engine* e, const uint32_t* res_id, const uint32_t* origin, const uint8_t* flags, uint32_t n,
                      int mem, uint8_t* out_flags) {
    if (!e || (n && (!res_id || !flags || !out_flags))) return fail(SF_ERR_INVALID, "null argument");
    if (!n) return SF_OK;
    std::lock_guard<std::mutex> lk(e->mu);
    hipStream_t s = e->stream;
    AuthTables t = e->auth;
    if (!origin) { t.of = nullptr; origin = res_id; }          // nothing blocks: the ids are not compared
    if (mem != SF_MEM_HOST) {
        HIP_TRY(launch_auth_mark(t, res_id, origin, flags, n, (uint8_t)SF_EV_BLOCKED, out_flags, s));
        HIP_TRY(hipStreamSynchronize(s));
        return SF_OK;
    }
    DevPool tmp{HIP_MEM};
    GrowBuf buf;
    const uint32_t *d_res = nullptr, *d_og = nullptr;
    const uint8_t* d_fl = nullptr;
    uint8_t* d_out = nullptr;
    StagePlan plan(true, true);
    plan.in(true, &d_res, res_id, (size_t)n * 4); plan.in(true, &d_og, origin, (size_t)n * 4);
    plan.in(true, &d_fl, flags, n); plan.out(true, &d_out, out_flags, n);
    SF_TRY(buf.reserve(tmp, plan.size()));
    plan.bind(buf.p);
    SF_TRY(plan.upload(h2d_on(s)));
    HIP_TRY(launch_auth_mark(t, d_res, d_og, d_fl, n, (uint8_t)SF_EV_BLOCKED, d_out, s));
    SF_TRY(plan.download(d2h_on(s)));
    HIP_TRY(hipStreamSynchronize(s));
    return SF_OK;
}

// The exact ParamFlow table never fills during a batch: before a batch with
// ParamFlow rules, the keys it can insert at most ((events + collection
// elements) x the most keys per event) must fit in the table's free half,
// counting the inserts of the batches still in flight the same way.  When
// they may not, everything drains, the device's insert counters give the
// exact fill, and the table is rebuilt larger if it is still too small
// (ParameterMetric's maps have no capacity in the reference apart from the
// LRU, ParameterMetric.java:99-118, whose eviction the exact table replaces).
static int param_reserve(sf_engine* e, uint64_t bound) {
    if (!e->n_prule || !bound) return SF_OK;
    const uint64_t cap = e->st.pcap_mask + 1;
    if ((e->p_used + e->p_pending + bound) * 2 <= cap) { e->p_pending += bound; return SF_OK; }
    auto read_used = [&](uint64_t* used) -> int {
        std::vector<unsigned int> c(256 * 16);
        HIP_TRY(hipMemcpy(c.data(), e->st.pins, c.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
        uint64_t u = 0;
        for (int k = 0; k < 256; k++) u += c[k * 16];
        *used = u;
        return SF_OK;
    };
    // The batches counted in p_pending may have finished already: when every
    // enqueued decide phase is done (a non-blocking event query), the device
    // counters give the exact fill without a drain, and the pending worst-case
    // bounds are released (they only ever grew before).
    bool idle = true;
    for (const Slot& sl : e->slot)
        if (idle && sl.used && hipEventQuery(sl.done) != hipSuccess) idle = false;
    if (idle) {
        uint64_t used = 0;
        SF_TRY(read_used(&used));
        e->p_used = used;
        e->p_pending = 0;
        if ((used + bound) * 2 <= cap) { e->p_pending = bound; return SF_OK; }
    }
    SF_TRY(drain(e));
    HIP_TRY(hipStreamSynchronize(e->stream));
    uint64_t used = 0;
    SF_TRY(read_used(&used));
    e->p_used = used;
    e->p_pending = 0;
    if ((used + bound) * 2 > cap) {
        uint64_t ncap = cap * 2;
        while ((used + bound) * 2 > ncap) ncap <<= 1;
        ParamSlot* nt = nullptr;
        HIP_TRY(hipDeviceSynchronize());
        SF_TRY(rehash_table(e, e->st.ptab, cap, ncap, &nt, &ncap, "param rehash"));
        e->pool.release(e->st.ptab);
        e->st.ptab = nt;
        e->st.pcap_mask = ncap - 1;
        e->p_grows++;
    }
    e->p_pending = bound;
    return SF_OK;
}

// the caller's batch and verdict arrays as device pointers: host arrays are
// copied to the engine's staging buffers on stream ss (verdicts come back
// from stage_out after the decision: vout.download, finish_sync)
static int stage_batch(sf_engine* e, const sf_event_batch* in, const sf_verdicts* out, hipStream_t ss,
                       DevBatch& b, DevVerdicts& dv, StagePlan& vout) {
    const uint32_t n = in->n;
    b.n = n; b.arg_slots = in->arg_slots; b.arg_stride = n;
    const bool host = in->mem == SF_MEM_HOST, coll = in->arg_elem_off != nullptr;
    const size_t na = (size_t)n * in->arg_slots;
    StagePlan p(host, false);
    // a host array that is absent or empty gives a null pointer; a device array is passed on as it is
    const auto arr = [&](bool on, auto** dev, const void* src, size_t bytes) {
        p.in(on && (!host || (src && bytes)), dev, src, bytes);
    };
    arr(true, &b.res, in->res_id, (size_t)n * 4); arr(true, &b.ts, in->ts_ms, (size_t)n * 8);
    arr(true, &b.cnt, in->count, (size_t)n * 4); arr(true, &b.flags, in->flags, n);
    arr(true, &b.eref, in->entry_ref, (size_t)n * 8);
    arr(in->entry_ref != nullptr, &b.cts, in->create_ts, (size_t)n * 8);
    arr(true, &b.nargs, in->n_args, n);
    arr(true, &b.atag, in->arg_tag, na); arr(true, &b.abits, in->arg_bits, na * 8);
    // (a host batch without arg_elem_off has no element arrays)
    arr(!host || coll, &b.aoff, in->arg_elem_off, (na + 1) * 4);
    arr(!host || coll, &b.etag, in->elem_tag, in->n_elems);
    arr(!host || coll, &b.ebits, in->elem_bits, (size_t)in->n_elems * 8);
    arr(true, &b.origin, in->origin, (size_t)n * 4); arr(true, &b.ctx, in->context, (size_t)n * 4);
    SF_TRY(e->stage_in.reserve(e->pool, p.size()));
    p.bind(e->stage_in.p);
    SF_TRY(p.upload(h2d_on(ss)));
    vout.out(true, &dv.status, out->status, n);
    vout.out(out->wait_ms != nullptr, &dv.wait, out->wait_ms, (size_t)n * 4);
    vout.out(out->rule_idx != nullptr, &dv.rule, out->rule_idx, (size_t)n * 2);
    SF_TRY(e->stage_out.reserve(e->pool, vout.size()));
    vout.bind(e->stage_out.p);
    return SF_OK;
}

// ---------------------------------------------------------------- stages of a submit (submit_core, sf_submit_node)
static int check_event_batch(const sf_engine* e, const sf_event_batch* in) {
    if (in->n && (!in->res_id || !in->ts_ms || !in->count || !in->flags)) return fail(SF_ERR_INVALID, "missing event array");
    if (in->n > e->cfg.max_batch) return fail(SF_ERR_CAPACITY, "batch larger than max_batch");
    if (in->arg_slots > SF_MAX_ARGS || (in->arg_slots && (!in->arg_tag || !in->arg_bits)))
        return fail(SF_ERR_INVALID, "bad arg arrays");
    if (in->arg_elem_off && in->n_elems && (!in->elem_tag || !in->elem_bits))
        return fail(SF_ERR_INVALID, "collection arguments without element arrays");
    return SF_OK;
}

// The origin-node pool on its first use (every entry with an origin has a node,
// ClusterBuilderSlot.java:107-110; the caller has drained) and room in the
// ParamFlow table for every key the batch can insert.
static int reserve_for_batch(sf_engine* e, const sf_event_batch* in, bool with_ox, uint32_t n_arg_events) {
    if (with_ox && !e->st.xtab) {
        SF_TRY(ensure_aux(e));
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    const uint64_t elems = in->arg_elem_off ? in->n_elems : 0;
    // (an event without arguments reaches no parameter map)
    return param_reserve(e, ((uint64_t)n_arg_events + elems) * e->p_kmax);
}

// the batch that last used the next batch's slot (two submits ago) must be done:
// its events and buffers are reused (sort(k) still overlaps decide(k-1))
static int take_slot(sf_engine* e, Slot& sl) {
    if (!sl.used) return SF_OK;
    HIP_TRY(hipEventSynchronize(sl.done));
    acc_timing(e, sl);
    return SF_OK;
}

// the SystemRule planner's buffers and its verdicts (sf_system.h), on first use
static int sys_buffers_ensure(sf_engine* e) {
    // (each on its own: one that is missing after a failure is allocated by the next call)
    if (!e->sys_plan) SF_TRY(e->pool.alloc(&e->sys_plan, sizeof(SysPlanDev)));
    if (!e->sys_pa) SF_TRY(e->pool.alloc(&e->sys_pa, SYS_PLAN_BLOCKS * sizeof(SysExitQ)));
    if (!e->sys_pb) SF_TRY(e->pool.alloc(&e->sys_pb, SYS_PLAN_BLOCKS * sizeof(SysEntQ)));
    if (!e->sys_mask) SF_TRY(e->pool.alloc(&e->sys_mask, e->cfg.max_batch));
    return SF_OK;
}

// the slot's batch is enqueued up to its last event record
static void slot_enqueued(sf_engine* e, Slot& sl, uint32_t n) {
    sl.used = true;
    e->last = (int)(&sl - e->slot);
    e->stats.n_events = n;
    e->stats.n_launches++;
}

// The end of a synchronous batch on `stream`: its events, the verdicts back to
// host arrays (vout: stage_batch's), its error flag, one stream sync.  plain:
// not the SystemRule rounds (the segment count and kernel times of the batch
// go to the stats).
static int finish_sync(sf_engine* e, Slot& sl, const StagePlan& vout, uint32_t n, bool plain) {
    hipStream_t s = e->stream;
    HIP_TRY(hipEventRecord(sl.core, s));
    HIP_TRY(hipEventRecord(sl.done, s));
    HIP_TRY(hipEventRecord(sl.end, s));
    slot_enqueued(e, sl, n);
    sl.timed = plain && e->timing;
    SF_TRY(vout.download(d2h_on(s)));
    int32_t err = 0;
    uint32_t nseg = 0;
    HIP_TRY(hipMemcpyAsync(&err, sl.w.err, 4, hipMemcpyDeviceToHost, s));
    if (plain) HIP_TRY(hipMemcpyAsync(&nseg, sl.w.n_seg, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (plain) {
        e->stats.n_segments = nseg;
        acc_timing(e, sl);
    }
    return batch_error(err);
}

// Sort and decide the view [p, q) of a staged batch (a SystemRule sub-batch):
// its IN entries' system verdicts are in e->sys_mask, the verdicts of the
// events before it in dv; stream e->stream (the caller fenced the batch's
// staging).  v / dvv: the view, for the caller's ENTRY_NODE step.
static int decide_view(sf_engine* e, Slot& sl, DevState& stl, const DevBatch& b, const DevVerdicts& dv,
                       uint32_t p, uint32_t q, bool with_ox, DevBatch& v, DevVerdicts& dvv) {
    hipStream_t s = e->stream;
    Work& w = sl.w;
    v = b;
    v.n = q - p; v.base = p;
    v.res = b.res + p; v.ts = b.ts + p; v.cnt = b.cnt + p; v.flags = b.flags + p;
    v.eref = b.eref ? b.eref + p : nullptr; v.cts = b.cts ? b.cts + p : nullptr;
    v.nargs = b.nargs ? b.nargs + p : nullptr;
    v.atag = b.atag ? b.atag + p : nullptr; v.abits = b.abits ? b.abits + p : nullptr;
    v.origin = b.origin ? b.origin + p : nullptr; v.ctx = b.ctx ? b.ctx + p : nullptr;
    v.sys = e->sys_mask + p; v.vprev = dv.status + p;
    dvv = DevVerdicts{dv.status + p, dv.wait ? dv.wait + p : nullptr, dv.rule ? dv.rule + p : nullptr};
    hipError_t le = launch_sort(stl, w, v, e->cfg.shard_count, e->cfg.shard_index, e->key_bits, s, sl.evs, false);
    OxPlan plan{};
    if (le == hipSuccess && with_ox) {
        SF_TRY(prepare_origins(e, sl, v, s, &plan));
        stl.xtab = e->st.xtab; stl.xcap_mask = e->st.xcap_mask; stl.ax_cap = e->st.ax_cap;
    }
    if (le == hipSuccess)
        le = launch_decide(stl, w, v, dvv, s, e->serial ? s : e->stream2, e->serial ? s : e->stream3,
                           e->serial ? s : e->stream4, sl.evs, false, with_ox ? &plan : nullptr);
    if (le == hipSuccess && with_ox) w.ox_dirty = false;     // k_ox_reset enqueued
    if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("launch: ") + hipGetErrorString(le));
    return SF_OK;
}

// pre: launched on the sort stream after the batch's error flag is cleared and
// before its sort (sf_submit_packed's expansion of the packed words)
using PreSort = std::function<hipError_t(hipStream_t, int32_t*)>;
// what sf_submit_packed adds to the batch it hands to submit_core: the
// expansion, whether a collection's abits is its CSR index already
// (DevBatch::acsr), and the events that can reach a parameter map
struct PackedHook { PreSort pre; bool acsr; uint32_t n_arg_events; };

// A staged batch under SystemRules on an unsharded engine.  They couple every
// IN entry to the global ENTRY_NODE: the batch is decided as a sequence of
// safe sub-batches (sf_system.h), each planned on the exact ENTRY_NODE, then
// sorted / decided / reduced by the ordinary pipeline.  One host round trip
// per sub-batch (its end q).
static int submit_sys_rounds(sf_engine* e, Slot& sl, const DevBatch& staged, const DevVerdicts& dv, const StagePlan& vout,
                             bool with_ox, const PreSort* pre) {
    DevBatch b = staged;                                // (the mark pass below redirects its flags)
    const uint32_t n = b.n;
    hipStream_t s = e->stream, ss = e->serial ? e->stream : e->sstream;
    Work& w = sl.w;
    SF_TRY(sys_buffers_ensure(e));
    if (!e->sys_ibuf && e->st.n_prule) SF_TRY(e->pool.alloc(&e->sys_ibuf, SYS_PLAN_CAP));
    HIP_TRY(hipMemsetAsync(w.err, 0, sizeof(int32_t), ss));
    if (pre) {
        const hipError_t pe = (*pre)(ss, w.err);
        if (pe != hipSuccess) return fail(SF_ERR_DEVICE, std::string("pre-sort: ") + hipGetErrorString(pe));
    }
    SF_TRY(auth_apply(e, sl, b, ss));                   // before the planner: it skips marked IN entries
    HIP_TRY(hipEventRecord(sl.sorted, ss));
    HIP_TRY(hipStreamWaitEvent(s, sl.sorted, 0));
    SF_TRY(en_fence(e));
    DevState stl = e->st;
    stl.err = w.err;
    uint32_t p = 0, rounds = 0;
    while (p < n) {
        hipError_t le = sys_plan(stl, b, dv.status, e->sys_mask, e->sys, e->en, p, e->sys_plan, e->sys_pa,
                                 e->sys_pb, s, e->sys_ibuf);
        if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("system plan: ") + hipGetErrorString(le));
        uint32_t qi[2] = {0, 0};                        // q, inert entries planned
        static_assert(offsetof(SysPlanDev, n_inert) == offsetof(SysPlanDev, q) + 4, "q, n_inert adjacent");
        HIP_TRY(hipMemcpyAsync(qi, &e->sys_plan->q, 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        const uint32_t q = qi[0];
        if (q <= p || q > n) return fail(SF_ERR_DEVICE, "system planner made no progress");
        DevBatch v;
        DevVerdicts dvv;
        SF_TRY(decide_view(e, sl, stl, b, dv, p, q, with_ox, v, dvv));
        // the system verdicts of the inert entries (ENTRY_NODE is still at p)
        if (qi[1]) le = sys_plan_fix(stl, b, dv, e->sys_mask, e->sys, p, q, e->sys_plan, e->sys_pa, e->sys_pb, s);
        if (le == hipSuccess) le = launch_entry_node(stl, v, dvv.status, e->en, e->en_acc, s);
        if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("launch: ") + hipGetErrorString(le));
        p = q;
        rounds++;
    }
    e->stats.sys_rounds += rounds;
    return finish_sync(e, sl, vout, n, false);
}

static int submit_core(sf_engine* e, const sf_event_batch* in, sf_verdicts* out, bool async,
                       const uint8_t* forced = nullptr, const PackedHook* hook = nullptr) {
    if (!e || !in || !out || !out->status) return fail(SF_ERR_INVALID, "null argument");
    if (in->n == 0) return SF_OK;
    SF_TRY(check_event_batch(e, in));
    // SystemRules read the node-wide ENTRY_NODE: a sharded engine decides them
    // only through the round protocol (sf_system_plan / sf_submit_forced)
    if (e->sys.check && e->cfg.shard_count > 1 && !forced)
        return fail(SF_ERR_UNSUPPORTED, "SystemRules on a sharded engine: use sf_system_plan + sf_submit_forced "
                                        "+ sf_entry_node_add (the node-wide round protocol)");
    const uint32_t n = in->n;
    hipStream_t s = e->stream, ss = e->serial ? e->stream : e->sstream;
    // the origin-node pass (sf_origin.hip) runs for batches with origins and
    // whenever rules read origin / context nodes (the xflow walk's node keys)
    const bool with_ox = in->origin || e->st.xmap;
    // asynchronous only for HBM-resident batches and verdicts, without SystemRules
    async = async && in->mem != SF_MEM_HOST && out->mem != SF_MEM_HOST && !e->sys.check && !forced;
    // (the first batch with origins builds the origin-node pool with nothing in flight)
    if (!async || (with_ox && !e->st.xtab)) SF_TRY(drain(e));
    SF_TRY(reserve_for_batch(e, in, with_ox, hook ? hook->n_arg_events : in->n));
    const PreSort* pre = hook ? &hook->pre : nullptr;
    for (Slot& x : e->slot) {                      // the other Work sets on first asynchronous use
        if (!async || x.ready) continue;
        HIP_TRY(hipStreamSynchronize(s));
        SF_TRY(alloc_work(e, x));
    }
    Slot& sl = e->slot[e->cur];
    SF_TRY(take_slot(e, sl));
    Work& w = sl.w;
    DevBatch b{};
    DevVerdicts dv{};
    StagePlan vout(false, out->mem == SF_MEM_HOST);
    SF_TRY(stage_batch(e, in, out, ss, b, dv, vout));
    b.acsr = hook && hook->acsr;
    if (forced) {
        // the forced SystemRule verdicts of this (sub-)batch, planned node-wide
        SF_TRY(sys_buffers_ensure(e));
        HIP_TRY(hipMemcpyAsync(e->sys_mask, forced, n, hipMemcpyHostToDevice, ss));
        b.sys = e->sys_mask;
    }
    if (e->sys.check && !forced) return submit_sys_rounds(e, sl, b, dv, vout, with_ox, pre);
    // sort phase on the sort stream, into this batch's Work set (after the
    // decide phase of the batch that used it last; the mark pass rewrites the
    // flags that batch's ENTRY_NODE update reads)
    if (sl.used) HIP_TRY(hipStreamWaitEvent(ss, e->auth.of && b.origin ? sl.end : sl.done, 0));
    HIP_TRY(hipMemsetAsync(w.err, 0, sizeof(int32_t), ss));
    if (pre) {
        const hipError_t pe = (*pre)(ss, w.err);
        if (pe != hipSuccess) return fail(SF_ERR_DEVICE, std::string("pre-sort: ") + hipGetErrorString(pe));
    }
    SF_TRY(auth_apply(e, sl, b, ss));
    DevState stl = e->st;
    stl.err = w.err;
    hipError_t le = launch_sort(stl, w, b, e->cfg.shard_count, e->cfg.shard_index, e->key_bits, ss, sl.evs, e->timing);
    if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("launch: ") + hipGetErrorString(le));
    OxPlan plan{};
    if (with_ox) {
        SF_TRY(prepare_origins(e, sl, b, ss, &plan));
        stl.xtab = e->st.xtab; stl.xcap_mask = e->st.xcap_mask; stl.ax_cap = e->st.ax_cap;
    }
    HIP_TRY(hipEventRecord(sl.sorted, ss));
    // decide phase in batch order on the main streams
    HIP_TRY(hipStreamWaitEvent(s, sl.sorted, 0));
    // an asynchronous batch's verdict scatter and ENTRY_NODE update run on the
    // ENTRY_NODE stream, beside the next batch's decide phase
    const bool side = async && !e->serial && e->side_mode != 0;
    le = launch_decide(stl, w, b, dv, s, e->serial ? s : e->stream2, e->serial ? s : e->stream3,
                       e->serial ? s : e->stream4, sl.evs, e->timing,
                       with_ox ? &plan : nullptr, false, side ? e->enstream : nullptr);
    if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("launch: ") + hipGetErrorString(le));
    if (with_ox) w.ox_dirty = false;                                  // k_ox_reset enqueued
    // ENTRY_NODE: every IN event's StatisticSlot updates (after the verdicts, stream
    // order); under the round protocol the node-wide stream updates it (sf_entry_node_add)
    if (!side && !forced) {
        SF_TRY(en_fence(e));
        le = launch_entry_node(stl, b, dv.status, e->en, e->en_acc, s);
        if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("entry node: ") + hipGetErrorString(le));
    }
    if (!async) return finish_sync(e, sl, vout, n, true);
    // side: on the side stream after the scatter.  The Work set is free after
    // the scatter (done: the sort of the batch after next waits for it), the
    // batch k_entry_acc reads after the update (end)
    hipStream_t es = side ? e->enstream : s;
    HIP_TRY(hipEventRecord(sl.core, es));
    HIP_TRY(hipEventRecord(sl.done, es));
    if (side) {
        le = launch_entry_node(stl, b, dv.status, e->en, e->en_acc, es);
        if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("entry node: ") + hipGetErrorString(le));
    }
    HIP_TRY(hipEventRecord(sl.end, es));
    if (side) { HIP_TRY(hipEventRecord(e->ev_en, es)); e->en_async = true; }
    slot_enqueued(e, sl, n);
    sl.timed = e->timing;
    e->pending |= 1u << e->cur;
    e->cur = (e->cur + 1) % SF_SLOTS;
    return SF_OK;
}

int sf_submit(sf_engine* e, const sf_event_batch* in, sf_verdicts* out) {
    if (!e) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    return submit_core(e, in, out, false);
}

int sf_submit_async(sf_engine* e, const sf_event_batch* in, sf_verdicts* out) {
    if (!e) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    return submit_core(e, in, out, true);
}

// ---------------------------------------------------------------- compact batches
// sf_packed_batch: the packed words (and the sparse exit / count arrays) go to
// the Work set's device stage on the H2D stream, are expanded to the SoA batch
// on the sort stream, decided by submit_core (asynchronously when asked), and
// the verdicts come back on the D2H stream once the batch is decided.
// the rest of a sparse batch's lists (beyond the prefetch) and their lengths, once its copies are done
static int sparse_complete(PkStage& pk) {
    const uint32_t nw = pk.sp_counts[0], nr = pk.sp_counts[1], pre = pk.sp.prefetch;
    if (nw > pre) HIP_TRY(hipMemcpy(pk.sp.waits + pre, pk.sp_wl + pre, (size_t)(nw - pre) * 8, hipMemcpyDeviceToHost));
    if (nr > pre) HIP_TRY(hipMemcpy(pk.sp.rules + pre, pk.sp_rl + pre, (size_t)(nr - pre) * 8, hipMemcpyDeviceToHost));
    pk.sp.counts[0] = nw; pk.sp.counts[1] = nr;
    pk.sparse = false;
    return SF_OK;
}

// Before a buffer of the slot's packed stage is reallocated -- the only time
// the host blocks for it -- every batch that may still read or write it is
// done: the slot's last batch, its expansion, the copy of its verdicts.
static int pk_quiesce(Slot& sl) {
    PkStage& pk = sl.pk;
    if (sl.used) HIP_TRY(hipEventSynchronize(sl.end));
    if (pk.consumed_pending) { HIP_TRY(hipEventSynchronize(pk.consumed)); pk.consumed_pending = false; }
    if (pk.d2h_pending) { HIP_TRY(hipEventSynchronize(pk.d2h)); pk.d2h_pending = false; }
    return SF_OK;
}

static int submit_packed(sf_engine* e, const sf_packed_batch* in, sf_verdicts* out, bool async,
                         const sf_sparse_verdicts* sp = nullptr) {
    if (!e || !in || !out || !out->status) return fail(SF_ERR_INVALID, "null argument");
    if (sp && (!sp->waits || !sp->rules || !sp->counts)) return fail(SF_ERR_INVALID, "null sparse list");
    if (in->n == 0) return SF_OK;
    const bool narrow = !in->ev && in->ev4;
    if ((!in->ev && !narrow) || (in->n_exit && !in->exit_ref) || (in->n_count_ext && !in->count_ext) ||
        (narrow && (!in->ms_end || in->n_ms == 0)))
        return fail(SF_ERR_INVALID, "missing packed arrays");
    if (narrow && in->n_ms > SF_PK4_MAX_MS) return fail(SF_ERR_INVALID, "narrow packed batch spans more than 2^20 ms");
    if (in->n > e->cfg.max_batch) return fail(SF_ERR_CAPACITY, "batch larger than max_batch");
    // ParamFlow arguments, collection elements, contexts (sf_pkargs.h): what the
    // scalars tell is refused here, what the tables hold by the expansion
    PkArgIn ai{in->n, in->n_arg_events, in->n_values, in->arg_slots, in->n_elems, in->arg_event, in->arg_off,
               in->arg_tag, in->arg_bits, in->elem_off};
    if (!pk_args_header_ok(ai)) return fail(SF_ERR_INVALID, "bad packed argument tables");
    if (!ai.n_values) ai.elem_off = nullptr;                   // (no value: no collection)
    if (!ai.elem_off) ai.n_elems = 0;
    if (ai.n_elems && (!in->elem_tag || !in->elem_bits))
        return fail(SF_ERR_INVALID, "collection arguments without element arrays");
    std::lock_guard<std::mutex> lk(e->mu);
    const uint32_t n = in->n;
    const bool host_in = in->mem == SF_MEM_HOST, host_out = sp || out->mem == SF_MEM_HOST;
    if (!e->h2d) {
        HIP_TRY(hipStreamCreateWithFlags(&e->h2d, hipStreamNonBlocking));
        HIP_TRY(hipStreamCreateWithFlags(&e->d2h, hipStreamNonBlocking));
        for (Slot& x : e->slot) {
            PkStage& p = x.pk;
            HIP_TRY(hipEventCreateWithFlags(&p.h2d, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&p.d2h, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&p.consumed, hipEventDisableTiming));
            SF_TRY(x.pkpool.alloc_host(&p.err_host, 4));
            *p.err_host = 0;
            SF_TRY(x.pkpool.alloc_host(&p.sp_counts, 8));
        }
    }
    // (submit_core decides asynchronously only without SystemRules; the slot it takes is e->cur)
    const bool core_async = async && !e->sys.check;
    if (!core_async) SF_TRY(drain(e));
    Slot& sl = e->slot[e->cur];
    PkStage& pk = sl.pk;
    // The slot's staging buffer: its packed inputs are free once the batch
    // before in this slot has expanded them (early in its sort phase), its
    // expanded arrays once that batch is decided (submit_core waits for it
    // before the expansion), its staged verdicts once their D2H copy is done.
    // All are waited for on the device, so the H2D of batch k+1 follows the
    // H2D of batch k back to back and overlaps the decision of k and the D2H
    // of k-1; the host blocks only to reallocate.
    const size_t N = e->cfg.max_batch;
    Layout L;
    const size_t o_ev = L.take(N * 8), o_xr = L.take(N * 8), o_xc = L.take(N * 8), o_ce = L.take(N * 4), o_og = L.take(N * 4);
    const size_t o_res = L.take(N * 4), o_ts = L.take(N * 8), o_cnt = L.take(N * 4), o_fl = L.take(N), o_er = L.take(N * 8);
    const size_t o_ct = L.take(N * 8), o_tc = L.take((N / 4096 + 2) * 8);
    const size_t o_st = L.take(N), o_wt = L.take(N * 4), o_ru = L.take(N * 2);
    const size_t o_wl = L.take_if(sp, N * 8), o_rl = L.take_if(sp, N * 8), o_sc = L.take_if(sp, 16);
    const size_t o_ms = L.take_if(narrow, (size_t)SF_PK4_MAX_MS * 4);   // (the narrow words use o_ev's room)
    if (pk.buf.bytes < L.size()) {
        SF_TRY(pk_quiesce(sl));
        SF_TRY(pk.buf.reserve(sl.pkpool, L.size()));
    }
    char* B = pk.buf.at(0);
    // The arguments, elements and contexts are sized by the batch, not by
    // max_batch, so they have a buffer of their own (pk.buf's offsets are fixed
    // and batches in flight point into it).  Two lifetimes: the staged sparse
    // inputs are free once expanded (`consumed`), the dense arrays, the copied
    // elements and contexts are read by the decide phase and live until the
    // slot's `end`, like the expanded SoA arrays -- which is why the expansion
    // copies elements and contexts instead of handing on the staged ones.
    // The staged origins follow the same rule: the xflow walk reads them in
    // submission order during the decide phase, and the next H2D copy into
    // this slot waits only for `consumed`.
    const bool args = ai.n_arg_events != 0, ctx = in->context != nullptr, og_copy = host_in && in->origin;
    const uint32_t nae = ai.n_arg_events, nv = ai.n_values, ne = ai.n_elems, slots = args ? ai.arg_slots : 0;
    // staged inputs (device batches are read in place: the sources of the
    // expansion are the caller's device arrays, or the staged ones); a host
    // array that is absent or empty gives a null pointer
    StagePlan pi(host_in, false), px(false, false);
    const auto arr = [&](auto** dev, size_t bytes) {     // (staged in place of the caller's pointer)
        pi.in(!host_in || (*dev && bytes), dev, *dev, bytes);
    };
    PkCopy cp{};
    if (args) {
        arr(&ai.arg_event, (size_t)nae * 4); arr(&ai.arg_off, ((size_t)nae + 1) * 4);
        arr(&ai.arg_tag, nv); arr(&ai.arg_bits, (size_t)nv * 8);
        arr(&ai.elem_off, ((size_t)nv + 1) * 4);
    }
    pi.in(ne != 0, &cp.etag, in->elem_tag, ne); pi.in(ne != 0, &cp.ebits, in->elem_bits, (size_t)ne * 8);
    pi.in(ctx, &cp.ctx, in->context, (size_t)n * 4);
    // what the expansion writes
    PkArgOut ao{};
    px.scratch(args, &ao.nargs, n); px.scratch(args, &ao.atag, (size_t)n * slots);
    px.scratch(args, &ao.abits, (size_t)n * slots * 8);
    px.scratch(args && ai.elem_off, &ao.eoff, ((size_t)nv + 1) * 4);
    px.scratch(ne != 0, &cp.etag_out, ne); px.scratch(ne != 0, &cp.ebits_out, (size_t)ne * 8);
    px.scratch(ctx, &cp.ctx_out, (size_t)n * 4); px.scratch(og_copy, &cp.origin_out, (size_t)n * 4);
    if (pi.size() > pk.a_in || px.size() > pk.a_x) {
        SF_TRY(pk_quiesce(sl));
        // (both regions grow to the largest seen: the boundary moves only here)
        const size_t c_in = std::max(pi.size(), pk.a_in), c_x = std::max(px.size(), pk.a_x);
        pk.a_in = pk.a_x = 0;
        SF_TRY(pk.abuf.reserve(sl.pkpool, c_in + c_x));
        pk.a_in = c_in; pk.a_x = c_x;
    }
    pi.bind(pk.abuf.p);
    px.bind(pk.abuf.at(pk.a_in));
    hipStream_t ss = e->serial ? e->stream : e->sstream;
    const uint64_t* ev = in->ev; const int64_t* xr = in->exit_ref; const int64_t* xc = in->exit_cts;
    const uint32_t* ev4 = narrow ? in->ev4 : nullptr; const uint32_t* mse = narrow ? in->ms_end : nullptr;
    const uint32_t n_ms = narrow ? in->n_ms : 0;
    const int32_t* ce = in->count_ext; const uint32_t* og = in->origin;
    if (host_in) {
        hipStream_t h = e->serial ? e->stream : e->h2d;
        if (pk.consumed_pending) HIP_TRY(hipStreamWaitEvent(h, pk.consumed, 0));
        if (narrow) {
            HIP_TRY(hipMemcpyAsync(B + o_ev, in->ev4, (size_t)n * 4, hipMemcpyHostToDevice, h));
            HIP_TRY(hipMemcpyAsync(B + o_ms, in->ms_end, (size_t)n_ms * 4, hipMemcpyHostToDevice, h));
            ev4 = (const uint32_t*)(B + o_ev);
            mse = (const uint32_t*)(B + o_ms);
        } else {
            HIP_TRY(hipMemcpyAsync(B + o_ev, in->ev, (size_t)n * 8, hipMemcpyHostToDevice, h));
            ev = (const uint64_t*)(B + o_ev);
        }
        if (in->n_exit) {
            HIP_TRY(hipMemcpyAsync(B + o_xr, in->exit_ref, (size_t)in->n_exit * 8, hipMemcpyHostToDevice, h));
            xr = (const int64_t*)(B + o_xr);
            if (in->exit_cts) {
                HIP_TRY(hipMemcpyAsync(B + o_xc, in->exit_cts, (size_t)in->n_exit * 8, hipMemcpyHostToDevice, h));
                xc = (const int64_t*)(B + o_xc);
            }
        }
        if (in->n_count_ext) {
            HIP_TRY(hipMemcpyAsync(B + o_ce, in->count_ext, (size_t)in->n_count_ext * 4, hipMemcpyHostToDevice, h));
            ce = (const int32_t*)(B + o_ce);
        }
        if (in->origin) {
            HIP_TRY(hipMemcpyAsync(B + o_og, in->origin, (size_t)n * 4, hipMemcpyHostToDevice, h));
            og = (const uint32_t*)(B + o_og);
        }
        SF_TRY(pi.upload(h2d_on(h)));
        if (og_copy) cp.origin = og;
        HIP_TRY(hipEventRecord(pk.h2d, h));
        HIP_TRY(hipStreamWaitEvent(ss, pk.h2d, 0));
    }
    const bool exits = in->n_exit != 0;
    const int64_t base = in->ts_base;
    const uint32_t n_exit = in->n_exit, n_cext = in->n_count_ext;
    const hipEvent_t consumed = pk.consumed;
    if (!args) { ai.n_arg_events = ai.n_values = 0; ai.arg_event = ai.arg_off = nullptr; ai.elem_off = nullptr; }
    const PreSort expand = [=](hipStream_t st_, int32_t* err) {
        const hipError_t le = launch_pk_expand(ev, ev4, mse, n_ms, xr, xc, ce, base, n, n_exit, n_cext, (uint2*)(B + o_tc),
                                               (uint32_t*)(B + o_res), (int64_t*)(B + o_ts), (int32_t*)(B + o_cnt),
                                               (uint8_t*)(B + o_fl), (int64_t*)(B + o_er),
                                               exits ? (int64_t*)(B + o_ct) : nullptr, err, st_);
        if (le != hipSuccess) return le;
        if (args || cp.etag || cp.ctx || cp.origin) {
            const hipError_t ae = launch_pk_args(ai, ao, cp, err, st_);
            if (ae != hipSuccess) return ae;
        }
        return hipEventRecord(consumed, st_);
    };
    if (pk.d2h_pending) { HIP_TRY(hipStreamWaitEvent(ss, pk.d2h, 0)); pk.d2h_pending = false; }
    sf_event_batch eb{};
    eb.n = n; eb.mem = SF_MEM_DEVICE;
    eb.res_id = (const uint32_t*)(B + o_res); eb.ts_ms = (const int64_t*)(B + o_ts);
    eb.count = (const int32_t*)(B + o_cnt); eb.flags = (const uint8_t*)(B + o_fl);
    eb.entry_ref = exits ? (const int64_t*)(B + o_er) : nullptr;
    eb.create_ts = exits ? (const int64_t*)(B + o_ct) : nullptr;
    eb.origin = cp.origin ? cp.origin_out : og;
    if (args) {
        eb.arg_slots = slots; eb.n_args = ao.nargs; eb.arg_tag = ao.atag; eb.arg_bits = ao.abits;
        if (ai.elem_off) {
            eb.arg_elem_off = ao.eoff; eb.n_elems = ne;
            eb.elem_tag = cp.etag_out; eb.elem_bits = cp.ebits_out;
        }
    }
    if (ctx) eb.context = cp.ctx_out;
    sf_verdicts dv{};
    dv.mem = SF_MEM_DEVICE;
    dv.status = host_out ? (uint8_t*)(B + o_st) : out->status;
    dv.wait_ms = (sp || out->wait_ms) ? (host_out ? (int32_t*)(B + o_wt) : out->wait_ms) : nullptr;
    dv.rule_idx = (sp || out->rule_idx) ? (host_out ? (uint16_t*)(B + o_ru) : out->rule_idx) : nullptr;
    // (the expansion rewrites the arrays the ENTRY_NODE update of this slot's
    // previous batch reads)
    if (sl.used) HIP_TRY(hipStreamWaitEvent(ss, sl.end, 0));
    const PackedHook hook{expand, ai.elem_off != nullptr, nae};
    SF_TRY(submit_core(e, &eb, &dv, core_async, nullptr, &hook));
    pk.consumed_pending = true;
    if (host_out) {
        hipStream_t d = e->serial ? e->stream : e->d2h;
        HIP_TRY(hipStreamWaitEvent(d, sl.core, 0));
        HIP_TRY(hipMemcpyAsync(out->status, dv.status, n, hipMemcpyDeviceToHost, d));
        pk.sparse = sp != nullptr;
        if (sp) {
            // 1 byte per event plus the exceptions: the nonzero waits / rule indices
            // compacted on the device, their first `prefetch` back with the statuses
            unsigned long long* wl = (unsigned long long*)(B + o_wl);
            unsigned long long* rl = (unsigned long long*)(B + o_rl);
            uint32_t* sc = (uint32_t*)(B + o_sc);
            HIP_TRY(launch_sparse_verdicts(dv.wait_ms, dv.rule_idx, n, wl, rl, sc, d));
            HIP_TRY(hipMemcpyAsync(pk.sp_counts, sc, 8, hipMemcpyDeviceToHost, d));
            const size_t pre = std::min<size_t>(sp->prefetch, n) * 8;
            if (pre) {
                HIP_TRY(hipMemcpyAsync(sp->waits, wl, pre, hipMemcpyDeviceToHost, d));
                HIP_TRY(hipMemcpyAsync(sp->rules, rl, pre, hipMemcpyDeviceToHost, d));
            }
            pk.sp = *sp; pk.sp_wl = wl; pk.sp_rl = rl;
        } else {
            if (out->wait_ms) HIP_TRY(hipMemcpyAsync(out->wait_ms, dv.wait_ms, (size_t)n * 4, hipMemcpyDeviceToHost, d));
            if (out->rule_idx) HIP_TRY(hipMemcpyAsync(out->rule_idx, dv.rule_idx, (size_t)n * 2, hipMemcpyDeviceToHost, d));
        }
        if (core_async) HIP_TRY(hipMemcpyAsync(pk.err_host, sl.w.err, 4, hipMemcpyDeviceToHost, d));
        HIP_TRY(hipEventRecord(pk.d2h, d));
        pk.d2h_pending = true;
        pk.out_status = core_async ? out->status : nullptr;
        if (!core_async) {
            HIP_TRY(hipEventSynchronize(pk.d2h));
            pk.d2h_pending = false;
            if (sp) SF_TRY(sparse_complete(pk));
        }
    }
    return SF_OK;
}

int sf_submit_packed(sf_engine* e, const sf_packed_batch* in, sf_verdicts* out) {
    return submit_packed(e, in, out, false);
}
int sf_submit_packed_async(sf_engine* e, const sf_packed_batch* in, sf_verdicts* out) {
    return submit_packed(e, in, out, true);
}

// Wait for ONE asynchronous packed batch: the one whose host verdicts go to
// out->status (its D2H copy, which follows its decision on the device); the
// batch submitted after it stays in flight.  Its error flag came back with the
// verdicts.  A batch already collected (by sf_sync, a rule reload's drain, or
// an earlier call) has nothing left to wait for: SF_OK.
static int sync_packed(sf_engine* e, const uint8_t* status) {
    for (int k = 0; k < SF_SLOTS; k++) {
        PkStage& pk = e->slot[k].pk;
        if (!status || pk.out_status != status) continue;
        // (a drain may have waited for its copies already; its error stays this batch's)
        if (pk.d2h_pending) HIP_TRY(hipEventSynchronize(pk.d2h));
        pk.d2h_pending = false;
        pk.out_status = nullptr;
        e->pending &= ~(1u << k);          // checked here, not again by sf_sync
        if (pk.sparse) SF_TRY(sparse_complete(pk));
        return batch_error(*pk.err_host);
    }
    return SF_OK;
}

int sf_sync_packed(sf_engine* e, const sf_verdicts* out) {
    if (!e || !out || !out->status) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    return sync_packed(e, out->status);
}

int sf_submit_packed_sparse_async(sf_engine* e, const sf_packed_batch* in, sf_sparse_verdicts* out) {
    if (!e || !in || !out || !out->status) return fail(SF_ERR_INVALID, "null argument");
    sf_verdicts v{};
    v.mem = SF_MEM_HOST; v.status = out->status;
    return submit_packed(e, in, &v, true, out);
}

int sf_sync_packed_sparse(sf_engine* e, const sf_sparse_verdicts* out) {
    if (!e || !out || !out->status) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    return sync_packed(e, out->status);
}

// ---------------------------------------------------------------- node-wide SystemRule rounds
// (sentinel_flow.h: sf_system_plan / sf_submit_forced / sf_entry_node_add)
int sf_submit_forced(sf_engine* e, const sf_event_batch* in, sf_verdicts* out, const uint8_t* sys_mask) {
    if (!e || !in || !out || !sys_mask) return fail(SF_ERR_INVALID, "null argument");
    if (in->mem != SF_MEM_HOST) return fail(SF_ERR_INVALID, "sf_submit_forced takes host arrays");
    std::lock_guard<std::mutex> lk(e->mu);
    return submit_core(e, in, out, false, sys_mask);
}

// stage host IN-event arrays (ts, count, flags, entry_ref, create_ts) + optional
// verdicts at a device scratch (StageBuf); DevBatch over them.  keep: the
// scratch already holds these event arrays (a later round of the same merged
// stream): only the verdicts are copied.
static int stage_in_events(sf_engine* e, StageBuf& sb, const sf_event_batch* in, const uint8_t* status,
                           uint32_t n_status, DevBatch& b, uint8_t** dstatus, bool keep = false) {
    const uint32_t n = in->n;
    b = DevBatch{};
    b.n = n;
    StagePlan p(true, false);
    p.in(true, &b.ts, in->ts_ms, (size_t)n * 8); p.in(true, &b.cnt, in->count, (size_t)n * 4);
    p.in(true, &b.flags, in->flags, n);
    p.in(in->entry_ref != nullptr, &b.eref, in->entry_ref, (size_t)n * 8);
    p.in(in->create_ts != nullptr, &b.cts, in->create_ts, (size_t)n * 8);
    p.scratch(dstatus, (size_t)n + 1);
    const void* key[5] = {in->ts_ms, in->count, in->flags, in->entry_ref, in->create_ts};
    // the same host arrays as the round before: a cheap fingerprint of their
    // contents must match too (the contract is that the caller only appends
    // verdicts between rounds; an edited event array is restaged, not trusted)
    const int64_t fp[3] = {n ? in->ts_ms[0] : 0, n ? in->ts_ms[n - 1] : 0, n ? (int64_t)in->flags[0] : 0};
    keep = keep && sb.buf.p && sb.n == n && std::equal(key, key + 5, sb.key) && std::equal(fp, fp + 3, sb.fp) &&
           p.size() <= sb.buf.bytes;
    if (p.size() > sb.buf.bytes) sb.n = 0;         // (nothing is staged in a new buffer)
    SF_TRY(sb.buf.reserve(e->pool, p.size()));
    p.bind(sb.buf.p);
    hipStream_t s = e->stream;
    if (!keep) {
        SF_TRY(p.upload(h2d_on(s)));
        std::copy(key, key + 5, sb.key);
        std::copy(fp, fp + 3, sb.fp);
        sb.n = n;
    }
    if (status && n_status) {
        // a continued stream: the verdicts staged for the round before are
        // final (the caller only appends), only the new ones are copied
        const uint32_t from = (keep && sb.st_src == status && sb.st_n <= n_status) ? sb.st_n : 0;
        if (n_status > from)
            HIP_TRY(hipMemcpyAsync(*dstatus + from, status + from, n_status - from, hipMemcpyHostToDevice, s));
        sb.st_src = status; sb.st_n = n_status;
    } else {
        sb.st_src = nullptr; sb.st_n = 0;
    }
    return SF_OK;
}

// ---------------------------------------------------------------- sharded SystemRules: the per-window exchange
// (sf_sysx.h; sentinel_flow.h sf_submit_node).  All ranks run the same number
// of all-gathers in the same order: every decision that shapes the loop is
// made from exchanged data (plan windows, the plan's levels and q).  RCCL:
// device buffers into d_recv; a callback: host buffers, the result in sx_hrecv.
static int sx_exchange(sf_engine* e, sf_allgather_fn fn, void* ctx, const int64_t* d_send, int64_t* d_recv,
                       size_t words) {
    const size_t bytes = words * 8, N = e->cfg.shard_count;
    hipStream_t s = e->stream;
    if (!fn) {
        const ncclResult_t r = ncclAllGather(d_send, d_recv, bytes, ncclInt8, e->comm, s);
        if (r != ncclSuccess) return fail(SF_ERR_DEVICE, std::string("ncclAllGather: ") + ncclGetErrorString(r));
        return SF_OK;
    }
    e->sx.hsend.resize(words);
    e->sx.hrecv.resize(words * N);
    HIP_TRY(hipMemcpyAsync(e->sx.hsend.data(), d_send, bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (fn(ctx, e->sx.hsend.data(), e->sx.hrecv.data(), bytes) != 0) return fail(SF_ERR_DEVICE, "all-gather callback failed");
    return SF_OK;                               // (every rank's message in sx_hrecv; the plan step reads it there)
}

static int sx_recv_reserve(sf_engine* e, size_t words) {
    if (e->sx.recv.bytes >= words * 8) return SF_OK;
    HIP_TRY(hipStreamSynchronize(e->stream));
    return e->sx.recv.reserve(e->pool, words * 8);
}

int sf_submit_node(sf_engine* e, const sf_event_batch* in, const int64_t* seq, sf_verdicts* out,
                   sf_allgather_fn allgather, void* ctx) {
    if (!e || !in || !out) return fail(SF_ERR_INVALID, "null argument");
    if (in->n && (!seq || !out->status)) return fail(SF_ERR_INVALID, "missing event array");
    SF_TRY(check_event_batch(e, in));
    std::lock_guard<std::mutex> lk(e->mu);
    if (!e->sys.check) return in->n ? submit_core(e, in, out, false) : SF_OK;   // nothing node-wide to decide
    // thread / average-RT / BBR checks: the wide message format and plan step (sf_sysx.h)
    const bool wide = !sx_rule_ok(e->sys);
    if (!allgather && !e->comm) return fail(SF_ERR_INVALID, "no exchange: sf_comm_init or an all-gather callback");
    SF_TRY(drain(e));
    const uint32_t n = in->n, N = e->cfg.shard_count;
    hipStream_t s = e->stream;
    if (!e->sx.msg) SF_TRY(e->pool.alloc(&e->sx.msg, SX_WORDS * 8));
    if (wide && !e->sx.wmsg) SF_TRY(e->pool.alloc(&e->sx.wmsg, SXW_WORDS * 8));
    if (wide && !e->sx.wsegs) SF_TRY(e->pool.alloc(&e->sx.wsegs, (size_t)SXW_MAX_SEGS * sizeof(SxwSeg)));
    if (wide) e->sx.whsegs.resize(SXW_MAX_SEGS);
    const size_t mwords = wide ? SXW_WORDS : SX_WORDS;
    int64_t* const msg = wide ? e->sx.wmsg : e->sx.msg;    // the level messages (the header uses sx_msg)
    if (!e->sx.ibuf) SF_TRY(e->pool.alloc(&e->sx.ibuf, e->cfg.max_batch));
    SF_TRY(sys_buffers_ensure(e));
    SF_TRY(sx_recv_reserve(e, (size_t)N * mwords));
    const bool with_ox = in->origin || e->st.xmap;
    SF_TRY(reserve_for_batch(e, in, with_ox, in->n));
    Slot& sl = e->slot[e->cur];
    SF_TRY(take_slot(e, sl));
    Work& w = sl.w;
    DevBatch b{};
    DevVerdicts dv{};
    StagePlan vout(false, out->mem == SF_MEM_HOST);
    SF_TRY(stage_batch(e, in, out, s, b, dv, vout));
    SF_TRY(auth_apply(e, sl, b, s));             // this rank's own events, before the exchange sees them
    const int64_t* dseq = seq;
    if (in->mem == SF_MEM_HOST && n) {
        if (!e->sx.seq) SF_TRY(e->pool.alloc(&e->sx.seq, (size_t)e->cfg.max_batch * 8));
        HIP_TRY(hipMemcpyAsync(e->sx.seq, seq, (size_t)n * 8, hipMemcpyHostToDevice, s));
        dseq = e->sx.seq;
    }
    HIP_TRY(hipMemsetAsync(w.err, 0, sizeof(int32_t), s));
    DevState stl = e->st;
    stl.err = w.err;
    SxArgs a{};
    a.b = b; a.seq = dseq; a.msg = e->sx.msg; a.vstatus = dv.status;
    a.r = e->sys; a.S = stl.S; a.wl = stl.wl; a.interval = stl.interval; a.max_rt = stl.max_rt;
    a.interval_sec = stl.interval / 1000.0; a.st = stl;
    a.ibuf = e->st.n_prule ? e->sx.ibuf : nullptr;
    a.g = std::__gcd((int64_t)stl.wl, (int64_t)1000);
    // every rank's message on the host: the plan step runs there (one sync per level)
    auto gather = [&](const int64_t* d_send, size_t words, std::vector<int64_t>& h) -> int {
        SF_TRY(sx_exchange(e, allgather, ctx, d_send, (int64_t*)e->sx.recv.p, words));
        if (allgather) { h.assign(e->sx.hrecv.begin(), e->sx.hrecv.begin() + words * N); return SF_OK; }
        h.resize(words * N);
        HIP_TRY(hipMemcpyAsync(h.data(), e->sx.recv.p, words * N * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        return SF_OK;
    };
    // ---- per batch: the node's plan windows (cells of g ms) and where each starts
    int64_t C0 = INT64_MAX, C1 = INT64_MIN, seq_end = INT64_MIN;
    bool neg = false;
    std::vector<int64_t> h;
    {
        HIP_TRY(sx_header(a, e->sx.msg, s));
        SF_TRY(gather(e->sx.msg, 5, h));
        for (uint32_t k = 0; k < N; k++) {
            const int64_t* x = &h[(size_t)k * 5];
            if (!x[4]) continue;
            C0 = std::min(C0, x[0]); C1 = std::max(C1, x[1]); seq_end = std::max(seq_end, x[2]);
            neg |= x[3] != 0;
        }
    }
    if (neg) return fail(SF_ERR_UNSUPPORTED, "an IN entry with acquireCount < 0: the event all-gather protocol");
    std::vector<int64_t> wseq;                  // start sequence number of each non-empty plan window
    std::vector<int64_t> wkey;                  // its index (cell - C0)
    if (seq_end != INT64_MIN) {
        const uint64_t nw = (uint64_t)(C1 - C0) + 1;
        if (nw > (1u << 22)) return fail(SF_ERR_CAPACITY, "batch spans too many plan windows");
        SF_TRY(sx_recv_reserve(e, (size_t)N * nw));
        DevPool tmp{HIP_MEM};
        int64_t* wbuf = nullptr;
        SF_TRY(tmp.alloc(&wbuf, nw * 8));
        a.c0 = C0;
        const hipError_t le = sx_winfirst(a, wbuf, (uint32_t)nw, s);
        if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("plan windows: ") + hipGetErrorString(le));
        SF_TRY(gather(wbuf, nw, h));
        tmp.release(wbuf);
        for (uint64_t k = 0; k < nw; k++) {
            int64_t m = INT64_MAX;
            for (uint32_t r = 0; r < N; r++) m = std::min(m, h[(size_t)r * nw + k]);
            if (m != INT64_MAX) { wseq.push_back(m); wkey.push_back((int64_t)k); }
        }
    }
    a.c0 = C0;
    // ENTRY_NODE, identical on every rank, advanced on the host by the node's deltas (no
    // kernel reads it while the batch is decided: the system verdicts are forced)
    EntryNode enh;
    HIP_TRY(hipMemcpyAsync(&enh, e->en, sizeof enh, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    uint32_t* d_lq = (uint32_t*)e->sx.recv.p;     // (sx_locate's result: the recv buffer is free then)
    // ---- rounds
    a.msg = msg;
    HIP_TRY(wide ? sxw_nodelta(msg, s) : sx_nodelta(msg, s));
    int64_t sp = wseq.empty() ? INT64_MAX : wseq[0];
    uint32_t lp = 0, rounds = 0;
    size_t j = 0;
    uint64_t levels = 0;
    // The wide kinds: how many sequence numbers past s_p a round plans.  Where a
    // thread or RT rule hovers at its threshold a round ends at an unknown entry
    // a few thousand events on, and binning the whole rest of the window first
    // costs a level per round; a range of 64^k numbers needs k levels.  Set from
    // the plan's own results (q), so it is the same on every rank: twice the
    // last round's length, rounded up to 64^k (k >= 2); 64 times wider after a
    // round that settled its whole range; no limit after a window's end.
    int64_t wcap = INT64_MAX;
    for (;;) {
        const bool fin = wseq.empty() || sp >= seq_end;
        while (!fin && j + 1 < wseq.size() && wseq[j + 1] <= sp) j++;
        const int64_t lo = fin ? 0 : sp, hi_w = fin ? 0 : (j + 1 < wseq.size() ? wseq[j + 1] : seq_end);
        const int64_t hi = (wide && !fin && hi_w - lo > wcap) ? lo + wcap : hi_w;
        const int64_t wstart = fin ? 0 : (C0 + wkey[j]) * a.g;
        SxPlan hp;
        SxwPlan hw;
        sx_begin(&hp, lo, hi);
        sxw_begin(&hw, lo, hi);
        for (int level = 0;; level++) {
            const hipError_t le = wide ? sxw_stats(a, hw, lp, level == 0, s) : sx_stats(a, hp, lp, level == 0, s);
            if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("exchange stats: ") + hipGetErrorString(le));
            SF_TRY(gather(msg, mwords, h));
            levels++;
            if (level == 0) {
                // the node's ENTRY_NODE contribution of the last sub-batch (its plan window is the key)
                int64_t key = -1;
                for (uint32_t k = 0; k < N; k++) key = std::max(key, h[(size_t)k * mwords + SXD_KEY]);
                if (key >= 0) {
                    const int64_t W = (C0 + key) * a.g;
                    sx_apply_delta(h.data(), (int)N, &enh, W - W % a.wl, a.S, a.wl, W - W % 1000, a.max_rt, mwords);
                }
                hw.base = sys_base(enh.second, a.S, a.wl, a.interval, a.max_rt, enh.threads, wstart);
                hp.P = hw.base.P;
            }
            if (wide) {
                sxw_reduce(h.data(), (int)N, &hw, e->sx.whsegs.data(), a.r, a.S, a.interval_sec);
                hp.q = hw.q; hp.done = hw.done;
            } else {
                sx_reduce(h.data(), (int)N, &hp, a.r, a.interval_sec);
            }
            if (hp.done) break;
            if (level > SXW_MAX_LEVELS) return fail(SF_ERR_DEVICE, "exchange plan did not converge");
        }
        if (fin) break;
        // (the plan is the same on every rank, so these fail on all of them together)
        if (hp.q <= sp || hp.q > hi) return fail(SF_ERR_DEVICE, "exchange plan made no progress");
        if (wide && hw.overflow) return fail(SF_ERR_DEVICE, "exchange plan: too many settled runs");
        uint32_t lq;
        if (in->mem == SF_MEM_HOST) {
            lq = (uint32_t)(std::lower_bound(seq + lp, seq + n, hp.q) - seq);
        } else {
            HIP_TRY(sx_locate(a, lp, hp.q, d_lq, s));
            HIP_TRY(hipMemcpyAsync(&lq, d_lq, 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        if (lq < lp || lq > n) return fail(SF_ERR_DEVICE, "exchange plan: bad local range");
        if (lq > lp) {
            if (wide && hw.nseg)
                HIP_TRY(hipMemcpyAsync(e->sx.wsegs, e->sx.whsegs.data(), (size_t)hw.nseg * sizeof(SxwSeg),
                                       hipMemcpyHostToDevice, s));
            hipError_t le = wide ? sxw_mask(a, e->sys_mask, lp, lq, e->sx.wsegs, hw.nseg, s)
                                 : sx_mask(a, e->sys_mask, lp, lq, hp.P, s);
            if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("exchange mask: ") + hipGetErrorString(le));
            DevBatch v;
            DevVerdicts dvv;
            SF_TRY(decide_view(e, sl, stl, b, dv, lp, lq, with_ox, v, dvv));
            le = launch_entry_delta(stl, v, dvv.status, e->en_acc, msg, wkey[j], s);
            if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("exchange delta: ") + hipGetErrorString(le));
        } else {
            HIP_TRY(wide ? sxw_nodelta(msg, s) : sx_nodelta(msg, s));
        }
        if (wide) {
            if (hp.q < hi) {
                const int64_t len = hp.q - sp;
                wcap = (int64_t)SXW_B * SXW_B;
                while (wcap < 2 * len && wcap < ((int64_t)1 << 48)) wcap *= SXW_B;
            } else if (hi < hi_w) {
                wcap = wcap < ((int64_t)1 << 48) ? wcap * SXW_B : INT64_MAX;
            } else {
                wcap = INT64_MAX;
            }
        }
        lp = lq;
        sp = hp.q;
        rounds++;
    }
    if (lp != n) return fail(SF_ERR_DEVICE, "exchange rounds left events undecided");
    // (enh lives in this frame: the copy is complete before any return)
    HIP_TRY(hipMemcpyAsync(e->en, &enh, sizeof enh, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    e->stats.sys_rounds += rounds;
    e->stats.sys_exchanges += levels;
    return finish_sync(e, sl, vout, n, false);
}

int sf_system_plan(sf_engine* e, const sf_event_batch* in, const uint8_t* status, uint32_t p, uint32_t* q,
                   uint8_t* sys_mask) {
    if (!e || !in || !q || !sys_mask || (p && !status)) return fail(SF_ERR_INVALID, "null argument");
    if (in->mem != SF_MEM_HOST || !in->ts_ms || !in->count || !in->flags)
        return fail(SF_ERR_INVALID, "sf_system_plan takes the node's IN events in host arrays");
    if (in->n > e->cfg.max_batch) return fail(SF_ERR_CAPACITY, "batch larger than max_batch");
    if (p >= in->n) return fail(SF_ERR_INVALID, "plan position past the batch");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(drain(e));
    const uint32_t n = in->n;
    if (!e->sys.check) {                                   // no SystemRule: nothing is forced
        std::memset(sys_mask + p, SYS_NONE, n - p);
        *q = n;
        return SF_OK;
    }
    SF_TRY(sys_buffers_ensure(e));
    DevBatch b;
    uint8_t* dstatus = nullptr;
    // a later round of the same merged stream (p > 0, same arrays): the events
    // staged for the round before are reused, only the verdicts are copied
    SF_TRY(stage_in_events(e, e->plan_sb, in, status, p, b, &dstatus, p > 0));
    hipStream_t s = e->stream;
    DevState stl = e->st;
    hipError_t le = sys_plan(stl, b, dstatus, e->sys_mask, e->sys, e->en, p, e->sys_plan, e->sys_pa, e->sys_pb, s);
    if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("system plan: ") + hipGetErrorString(le));
    uint32_t qq = 0;
    HIP_TRY(hipMemcpyAsync(&qq, &e->sys_plan->q, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (qq <= p || qq > n) return fail(SF_ERR_DEVICE, "system planner made no progress");
    HIP_TRY(hipMemcpy(sys_mask + p, e->sys_mask + p, qq - p, hipMemcpyDeviceToHost));
    *q = qq;
    return SF_OK;
}

int sf_entry_node_add(sf_engine* e, const sf_event_batch* in, const uint8_t* status) {
    if (!e || !in || !status) return fail(SF_ERR_INVALID, "null argument");
    if (in->mem != SF_MEM_HOST || !in->ts_ms || !in->count || !in->flags)
        return fail(SF_ERR_INVALID, "sf_entry_node_add takes host arrays");
    if (in->n > e->cfg.max_batch) return fail(SF_ERR_CAPACITY, "batch larger than max_batch");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(drain(e));
    if (!in->n) return SF_OK;
    DevBatch b;
    uint8_t* dstatus = nullptr;
    SF_TRY(stage_in_events(e, e->en_sb, in, status, in->n, b, &dstatus));
    hipError_t le = launch_entry_node(e->st, b, dstatus, e->en, e->en_acc, e->stream);
    if (le != hipSuccess) return fail(SF_ERR_DEVICE, std::string("entry node: ") + hipGetErrorString(le));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SF_OK;
}

// A kernel's small result: `bytes` of scratch, launch(scratch) on `stream`, the
// copy back and one sync; the scratch is freed on every path.
static int read_back(sf_engine* e, void* host, size_t bytes, const char* what,
                     const std::function<hipError_t(void*)>& launch) {
    DevPool tmp{HIP_MEM};
    void* d = nullptr;
    SF_TRY(tmp.alloc(&d, bytes));
    hipError_t he = launch(d);
    if (he == hipSuccess) he = hipMemcpyAsync(host, d, bytes, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
    if (he != hipSuccess) return fail(SF_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(he));
    return SF_OK;
}

static Bucket from_abi_bucket(const sf_bucket& o, int64_t max_rt) {
    Bucket d{};
    if (o.window_start == SF_WS_ABSENT) { d = Bucket{WS_NONE, 0, 0, 0, 0, 0, 0, max_rt}; return d; }
    d.ws = o.window_start; d.pass = o.pass; d.block = o.block; d.exc = o.exception; d.succ = o.success; d.rt = o.rt;
    d.occ = o.occupied_pass; d.min_rt = o.min_rt;
    return d;
}
static void to_abi_bucket(const Bucket& d, sf_bucket* o) {
    o->window_start = d.ws == WS_NONE ? SF_WS_ABSENT : d.ws;
    o->pass = d.pass; o->block = d.block; o->exception = d.exc; o->success = d.succ; o->rt = d.rt;
    o->occupied_pass = d.occ; o->min_rt = d.min_rt;
    if (d.ws == WS_NONE) { o->pass = o->block = o->exception = o->success = o->rt = o->occupied_pass = o->min_rt = 0; }
}

// one node's rows (a resource row or an origin / context pool slot) -> sf_node_state
static int read_rows(sf_engine* e, const Bucket* gsec, const Borrow* gbor, const Bucket* gmin, const int64_t* gthr,
                     sf_node_state* out) {
    const int S = e->cfg.sample_count;
    std::vector<Bucket> sec(S), mins(MINUTE);
    std::vector<Borrow> bor(S);
    int64_t th = 0;
    HIP_TRY(hipMemcpyAsync(sec.data(), gsec, S * sizeof(Bucket), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(bor.data(), gbor, S * sizeof(Borrow), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(mins.data(), gmin, MINUTE * sizeof(Bucket), hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipMemcpyAsync(&th, gthr, 8, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    std::memset(out, 0, sizeof *out);
    for (int i = 0; i < SF_MAX_SAMPLE_COUNT; i++) { out->second[i].window_start = SF_WS_ABSENT; out->borrow_ws[i] = SF_WS_ABSENT; }
    for (int i = 0; i < S; i++) {
        to_abi_bucket(sec[i], &out->second[i]);
        out->borrow_ws[i] = bor[i].ws == WS_NONE ? SF_WS_ABSENT : bor[i].ws;
        out->borrow_pass[i] = bor[i].ws == WS_NONE ? 0 : bor[i].pass;
    }
    for (int i = 0; i < MINUTE; i++) to_abi_bucket(mins[i], &out->minute[i]);
    out->cur_thread_num = th;
    return SF_OK;
}

int sf_read_node(sf_engine* e, uint32_t resource, sf_node_state* out) {
    if (!e || !out) return fail(SF_ERR_INVALID, "null argument");
    uint32_t l;
    if (!local_of(e, resource, &l)) return fail(SF_ERR_INVALID, "resource outside this shard");
    std::lock_guard<std::mutex> lk(e->mu);
    const NodeRows r = cluster_rows(e->st, l);
    return read_rows(e, r.sec, r.bor, r.min, r.thr, out);
}

// origin / context node of local resource l (sf_xflow.h aux_get): its pool
// slot found on the device, its rows read through the host's chunk directory
static int read_aux(sf_engine* e, uint32_t resource, uint32_t kind, uint32_t id, sf_node_state* out) {
    if (!e || !out) return fail(SF_ERR_INVALID, "null argument");
    uint32_t l;
    if (!local_of(e, resource, &l)) return fail(SF_ERR_INVALID, "resource outside this shard");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(drain(e));
    if (!e->st.xtab) return fail(SF_ERR_INVALID, "no origin / context node is kept");
    uint32_t k = XNONE;
    SF_TRY(read_back(e, &k, 4, "aux find", [&](void* d) {
        return launch_aux_find(e->st, pkey_hi(l, PK_AUX, kind, 0), id, (uint32_t*)d, e->stream);
    }));
    if (k == XNONE || k >= e->st.ax_cap) return fail(SF_ERR_INVALID, "that origin / context node is not kept");
    DevState hs = e->st;
    hs.ax_chunks = e->ax_host.data();            // host mirror of the chunk directory
    const NodeRows r = aux_rows(hs, k);
    return read_rows(e, r.sec, r.bor, r.min, r.thr, out);
}
int sf_read_origin_node(sf_engine* e, uint32_t resource, uint32_t origin, sf_node_state* out) {
    return read_aux(e, resource, AX_ORIGIN, origin, out);
}
int sf_read_context_node(sf_engine* e, uint32_t context, uint32_t resource, sf_node_state* out) {
    return read_aux(e, resource, AX_CTX, context, out);
}

int sf_read_entry_node(sf_engine* e, sf_node_state* out) {
    if (!e || !out) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(en_fence(e));
    EntryNode en;
    HIP_TRY(hipMemcpyAsync(&en, e->en, sizeof en, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    std::memset(out, 0, sizeof *out);
    for (int i = 0; i < SF_MAX_SAMPLE_COUNT; i++) { out->second[i].window_start = SF_WS_ABSENT; out->borrow_ws[i] = SF_WS_ABSENT; }
    for (int i = 0; i < e->cfg.sample_count; i++) to_abi_bucket(en.second[i], &out->second[i]);
    for (int i = 0; i < MINUTE; i++) to_abi_bucket(en.minute[i], &out->minute[i]);
    out->cur_thread_num = en.threads;
    return SF_OK;
}

int sf_read_rule_state(sf_engine* e, uint32_t idx, sf_rule_state* out) {
    if (!e || !out) return fail(SF_ERR_INVALID, "null argument");
    if (idx >= e->n_flow) return fail(SF_ERR_INVALID, "rule index");
    std::lock_guard<std::mutex> lk(e->mu);
    DevRuleState s{};
    HIP_TRY(hipMemcpy(&s, e->st.rstate + e->flow_pos[idx], sizeof s, hipMemcpyDeviceToHost));
    out->stored_tokens = s.stored_tokens; out->last_filled_time = s.last_filled; out->latest_passed_time = s.latest_passed;
    return SF_OK;
}

int sf_node_digests(sf_engine* e, uint64_t* out, uint32_t n_rows) {
    if (!e || (n_rows && !out)) return fail(SF_ERR_INVALID, "null argument");
    if (n_rows > e->R) return fail(SF_ERR_INVALID, "n_rows above max_resources");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(drain(e));
    if (!n_rows) return SF_OK;
    return read_back(e, out, (size_t)n_rows * 8, "node digests", [&](void* d) {
        return launch_node_digests(e->st, n_rows, (unsigned long long*)d, e->stream);
    });
}

int sf_read_rule_states(sf_engine* e, uint32_t first, uint32_t n, sf_rule_state* out) {
    if (!e || (n && !out)) return fail(SF_ERR_INVALID, "null argument");
    if ((uint64_t)first + n > e->n_flow) return fail(SF_ERR_INVALID, "rule index");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(drain(e));
    if (!n) return SF_OK;
    std::vector<DevRuleState> all(e->n_flow);      // CSR order: the positions of a range are not contiguous
    HIP_TRY(hipMemcpyAsync(all.data(), e->st.rstate, all.size() * sizeof(DevRuleState), hipMemcpyDeviceToHost,
                           e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (uint32_t i = 0; i < n; i++) {
        const DevRuleState& s = all[e->flow_pos[first + i]];
        out[i].stored_tokens = s.stored_tokens; out[i].last_filled_time = s.last_filled;
        out[i].latest_passed_time = s.latest_passed;
    }
    return SF_OK;
}


// ---------------------------------------------------------------- node-wide aggregate (RCCL)
int sf_comm_unique_id(uint8_t* out, size_t len) {
    if (!out || len < NCCL_UNIQUE_ID_BYTES) return fail(SF_ERR_INVALID, "unique id buffer");
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(SF_ERR_DEVICE, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
    std::memcpy(out, id.internal, NCCL_UNIQUE_ID_BYTES);
    return SF_OK;
}

int sf_comm_init(sf_engine* e, int nranks, int rank, const uint8_t* id, size_t len) {
    if (!e || !id || len < NCCL_UNIQUE_ID_BYTES || nranks <= 0 || rank < 0 || rank >= nranks)
        return fail(SF_ERR_INVALID, "sf_comm_init arguments");
    std::lock_guard<std::mutex> lk(e->mu);
    if (e->comm) { ncclCommDestroy(e->comm); e->comm = nullptr; }
    HIP_TRY(hipSetDevice(e->cfg.device));
    ncclUniqueId uid;
    std::memcpy(uid.internal, id, NCCL_UNIQUE_ID_BYTES);
    ncclResult_t r = ncclCommInitRank(&e->comm, nranks, uid, rank);
    if (r != ncclSuccess) { e->comm = nullptr; return fail(SF_ERR_DEVICE, std::string("ncclCommInitRank: ") + ncclGetErrorString(r)); }
    if (!e->sx.agg) SF_TRY(e->pool.alloc(&e->sx.agg, 4096 * sizeof(int64_t)));
    return SF_OK;
}

int sf_set_report_entry_node(sf_engine* e, const sf_node_state* node) {
    if (!e) return fail(SF_ERR_INVALID, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(en_fence(e));
    if (!node) { e->rep.report_set = false; return SF_OK; }
    EntryNode& r = e->rep.report;
    r = EntryNode{};
    const int64_t mrt = e->cfg.statistic_max_rt;
    for (int i = 0; i < SF_MAX_SAMPLE_COUNT; i++)
        r.second[i] = i < e->cfg.sample_count ? from_abi_bucket(node->second[i], mrt) : Bucket{WS_NONE, 0, 0, 0, 0, 0, 0, mrt};
    for (int i = 0; i < MINUTE; i++) r.minute[i] = from_abi_bucket(node->minute[i], mrt);
    r.threads = node->cur_thread_num;
    e->rep.report_set = true;
    return SF_OK;
}

int sf_entry_node_allreduce(sf_engine* e, sf_node_state* out) {
    if (!e || !out) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(en_fence(e));
    if (!e->comm) return fail(SF_ERR_INVALID, "sf_comm_init first");
    const int S = e->cfg.sample_count, nb = S + MINUTE;
    hipStream_t s = e->stream;
    int64_t *ws = e->sx.agg, *gws = ws + nb, *vals = gws + nb, *minrt = vals + nb * 6 + 1;
    HIP_TRY(launch_en_pack_ws(e->en, S, ws, s));
    auto nc = [&](ncclResult_t r, const char* what) -> int {
        return r == ncclSuccess ? SF_OK : fail(SF_ERR_DEVICE, std::string(what) + ": " + ncclGetErrorString(r));
    };
    SF_TRY(nc(ncclAllReduce(ws, gws, nb, ncclInt64, ncclMax, e->comm, s), "allreduce max"));
    HIP_TRY(launch_en_pack_vals(e->en, S, gws, vals, minrt, s));
    SF_TRY(nc(ncclAllReduce(vals, vals, (size_t)nb * 6 + 1, ncclInt64, ncclSum, e->comm, s), "allreduce sum"));
    SF_TRY(nc(ncclAllReduce(minrt, minrt, nb, ncclInt64, ncclMin, e->comm, s), "allreduce min"));
    std::vector<int64_t> h_ws(nb), h_vals((size_t)nb * 6 + 1), h_min(nb);
    HIP_TRY(hipMemcpyAsync(h_ws.data(), gws, nb * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_vals.data(), vals, h_vals.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_min.data(), minrt, nb * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::memset(out, 0, sizeof *out);
    for (int i = 0; i < SF_MAX_SAMPLE_COUNT; i++) { out->second[i].window_start = SF_WS_ABSENT; out->borrow_ws[i] = SF_WS_ABSENT; }
    for (int i = 0; i < MINUTE; i++) out->minute[i].window_start = SF_WS_ABSENT;
    for (int i = 0; i < nb; i++) {
        sf_bucket& b = i < S ? out->second[i] : out->minute[i - S];
        if (h_ws[i] == INT64_MIN) continue;
        b.window_start = h_ws[i];
        const int64_t* v = &h_vals[(size_t)i * 6];
        b.pass = v[0]; b.block = v[1]; b.exception = v[2]; b.success = v[3]; b.rt = v[4]; b.occupied_pass = v[5];
        b.min_rt = h_min[i] == INT64_MAX ? e->cfg.statistic_max_rt : h_min[i];
    }
    out->cur_thread_num = h_vals[(size_t)nb * 6];
    return SF_OK;
}

int sf_device_alloc(sf_engine* e, size_t bytes, void** ptr) {
    if (!e || !ptr) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    return e->user_dev.alloc(ptr, nz(bytes));
}
int sf_device_free(sf_engine* e, void* ptr) {
    if (!e) return fail(SF_ERR_INVALID, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    if (!ptr || !e->user_dev.release(ptr)) return fail(SF_ERR_INVALID, "pointer not from sf_device_alloc");
    return SF_OK;
}
int sf_host_alloc(sf_engine* e, size_t bytes, void** ptr) {
    if (!e || !ptr) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    return e->user_host.alloc_host(ptr, nz(bytes));
}
int sf_host_free(sf_engine* e, void* ptr) {
    if (!e) return fail(SF_ERR_INVALID, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    if (!ptr || !e->user_host.release(ptr)) return fail(SF_ERR_INVALID, "pointer not from sf_host_alloc");
    return SF_OK;
}
int sf_memcpy(sf_engine* e, void* dst, const void* src, size_t bytes, int kind) {
    if (!e) return fail(SF_ERR_INVALID, "null engine");
    hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, k, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return SF_OK;
}
int sf_sync(sf_engine* e) {
    if (!e) return fail(SF_ERR_INVALID, "null engine");
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_TRY(hipStreamSynchronize(e->sstream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return drain(e, true);
}
int sf_get_stats(sf_engine* e, sf_stats* out) {
    if (!e || !out) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    *out = e->stats;
    if (e->st.ax_count) {
        uint32_t ax = 0;
        HIP_TRY(hipMemcpy(&ax, e->st.ax_count, 4, hipMemcpyDeviceToHost));
        out->aux_nodes = ax;
    }
    out->aux_capacity = e->st.ax_cap;
    out->aux_index_grows = e->aux_grows;
    out->param_table_grows = e->p_grows;
    if (e->st.xw_stats) {
        unsigned long long x[4];
        HIP_TRY(hipMemcpy(x, e->st.xw_stats, sizeof x, hipMemcpyDeviceToHost));
        out->xw_chunks_exact = x[0]; out->xw_chunks_serial = x[1]; out->xw_rounds = x[2]; out->xw_serial_events = x[3];
    }
    if (e->emb_stats) {
        unsigned long long x[2];
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipMemcpy(x, e->emb_stats, sizeof x, hipMemcpyDeviceToHost));
        out->xcl_chunks_wave = x[0]; out->xcl_chunks_serial = x[1];
    }
    return SF_OK;
}
int sf_set_timing(sf_engine* e, int enabled) {
    if (!e) return fail(SF_ERR_INVALID, "null engine");
    e->timing = enabled != 0;
    std::memset(&e->stats, 0, sizeof e->stats);
    return SF_OK;
}

int sf_read_param_thread(sf_engine* e, uint32_t resource, int param_idx, uint8_t tag, uint64_t bits, int64_t* out) {
    if (!e || !out) return fail(SF_ERR_INVALID, "null argument");
    uint32_t l = 0;
    if (!local_of(e, resource, &l)) return fail(SF_ERR_INVALID, "resource outside this shard");
    std::lock_guard<std::mutex> g(e->mu);
    SF_TRY(drain(e));
    long long h = 0;
    SF_TRY(read_back(e, &h, 8, "param thread read", [&](void* d) {
        return launch_param_thread_read(e->st, l, param_idx, tag, bits, (long long*)d, e->stream);
    }));
    *out = h;
    return SF_OK;
}

int sf_param_table_stats(sf_engine* e, uint64_t* used, uint64_t* capacity, uint32_t* max_probe) {
    if (!e || !used || !capacity || !max_probe) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> g(e->mu);
    SF_TRY(drain(e));
    unsigned long long h[2] = {0, 0};
    SF_TRY(read_back(e, h, 16, "param stats", [&](void* d) {
        return launch_param_stats(e->st, (unsigned long long*)d, e->stream);
    }));
    *used = h[0]; *capacity = e->st.pcap_mask + 1; *max_probe = (uint32_t)h[1];
    return SF_OK;
}

int sf_heavy_profile_read(sf_engine* e, sf_heavy_profile* out, uint32_t cap, uint32_t* n_out) {
    if (!e || !n_out || (cap && !out)) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> g(e->mu);
    uint32_t cnt[WC_STREAM_BACK + 1] = {}, nseg = 0;       // the list lengths of Work::counters
    SF_TRY(drain(e));
    const Work& lw = e->slot[e->last].w;
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream2));
    HIP_TRY(hipStreamSynchronize(e->stream3));
    if (e->stream4) HIP_TRY(hipStreamSynchronize(e->stream4));
    HIP_TRY(hipMemcpy(cnt, lw.counters, sizeof cnt, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(&nseg, lw.n_seg, 4, hipMemcpyDeviceToHost));
    const uint32_t hf = cnt[WC_HEAVY_FRONT], sf = cnt[WC_STREAM_FRONT];
    const uint32_t n1 = hf + cnt[WC_HEAVY_BACK], n2 = sf + cnt[WC_STREAM_BACK];
    const uint32_t nh = std::min(n1 + n2, cap);
    std::vector<uint32_t> full(lw.seg_cap), full2(lw.seg_cap), list(nh), start(nseg + 1), res(nseg);
    std::vector<uint8_t> mode(nseg);
    std::vector<uint64_t> ticks(n1 + 1), ticks2(n2 + 1), tk(nh);
    if (nh) {
        HIP_TRY(hipMemcpy(full.data(), lw.heavy_list, (size_t)lw.seg_cap * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(full2.data(), lw.stream_list, (size_t)lw.seg_cap * 4, hipMemcpyDeviceToHost));
        // per-block clocks exist for the first grid-size entries only (grid-stride beyond)
        const size_t hcap = (size_t)e->cfg.max_batch / (lw.heavy_min + 1) + 2;
        HIP_TRY(hipMemcpy(ticks.data(), lw.hticks, std::min<size_t>(n1, hcap) * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(ticks2.data(), lw.sticks, n2 * 8, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < nh; i++) {
            if (i < n1) {
                list[i] = i < hf ? full[i] : full[lw.seg_cap - 1 - (i - hf)];
                tk[i] = ticks[i];
            } else {
                const uint32_t k = i - n1;
                list[i] = k < sf ? full2[k] : full2[lw.seg_cap - 1 - (k - sf)];
                tk[i] = ticks2[k];
            }
        }
        HIP_TRY(hipMemcpy(start.data(), lw.seg_start, (nseg + 1) * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(res.data(), lw.seg_res, nseg * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(mode.data(), lw.seg_mode, nseg, hipMemcpyDeviceToHost));
    }
    uint64_t t0 = ~0ull;
    for (uint32_t i = n1; i < nh; i++) t0 = std::min(t0, tk[i] >> 24);
    for (uint32_t i = 0; i < nh; i++) {
        const uint32_t sg = list[i];
        out[i].resource = res[sg]; out[i].events = start[sg + 1] - start[sg];
        out[i].mode = mode[sg]; out[i].start = 0; out[i].ticks = e->timing ? tk[i] : 0;
        if (i >= n1 && e->timing) {          // stream segments: (start & 2^40-1) << 24 | duration
            out[i].ticks = tk[i] & 0xffffffull;
            out[i].start = (uint32_t)((tk[i] >> 24) - t0);
        }
    }
    *n_out = nh;
    return SF_OK;
}



}  // extern "C"
