// sf_host_report.cpp -- the metric snapshot and metrics.log of the host runtime
// (sf_entry.hip, sf_metric.hip): sf_snapshot, the resource names,
// sf_metric_log and sf_format_metric_rows.
#include "sf_host.h"

extern "C" {

int sf_snapshot(sf_engine* e, int64_t now_ms, sf_metric_row* out, uint32_t cap, uint32_t* n_out) {
    if (!e || !n_out || (cap && !out)) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(en_fence(e));
    *n_out = 0;
    hipStream_t s = e->stream;
    if (!e->rep.snap_ready) {
        const int rc = [&]() -> int {
            SF_TRY(e->pool.alloc(&e->rep.snap_counts, (size_t)e->R * 4));
            SF_TRY(e->pool.alloc(&e->rep.snap_offsets, (size_t)e->R * 4));
            SF_TRY(e->pool.alloc(&e->rep.snap_total, 4));
            HIP_TRY(rocprim_scan_bytes(e->R, &e->rep.snap_scan_bytes));
            return e->pool.alloc(&e->rep.snap_scan, min16(e->rep.snap_scan_bytes));
        }();
        if (rc) { e->pool.release_all(e->rep.snap_counts, e->rep.snap_offsets, e->rep.snap_total, e->rep.snap_scan); return rc; }
        e->rep.snap_ready = true;
    }
    SF_TRY(e->rep.snap_rows.reserve(e->pool, (size_t)cap * sizeof(sf_metric_row)));
    sf_metric_row* rows = (sf_metric_row*)e->rep.snap_rows.p;
    HIP_TRY(launch_snapshot(e->st, now_ms, e->cfg.shard_count, e->cfg.shard_index, e->rep.snap_counts, e->rep.snap_offsets,
                            rows, cap, e->rep.snap_total, e->rep.snap_scan, e->rep.snap_scan_bytes, s));
    uint32_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, e->rep.snap_total, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t k = std::min(total, cap);
    if (k) HIP_TRY(hipMemcpy(out, rows, (size_t)k * sizeof(sf_metric_row), hipMemcpyDeviceToHost));
    *n_out = total;
    return total <= cap ? SF_OK : fail(SF_ERR_CAPACITY, "snapshot rows exceed cap");
}
// ---------------------------------------------------------------- metrics.log
int sf_load_resource_names(sf_engine* e, const char* bytes, const uint64_t* offsets, const int32_t* types,
                           uint32_t n) {
    if (!e || (n && (!offsets || (!bytes && offsets[n])))) return fail(SF_ERR_INVALID, "null argument");
    for (uint32_t i = 0; i < n; i++)
        if (offsets[i + 1] < offsets[i]) return fail(SF_ERR_INVALID, "name offsets must be non-decreasing");
    std::lock_guard<std::mutex> lk(e->mu);
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->pool.release_all(e->rep.nm_bytes, e->rep.nm_off, e->rep.nm_types);
    e->rep.n_names = 0;
    const uint64_t nb = n ? offsets[n] - offsets[0] : 0;
    SF_TRY(e->pool.alloc(&e->rep.nm_bytes, min16(nb)));
    SF_TRY(e->pool.alloc(&e->rep.nm_off, ((size_t)n + 1) * 8));
    if (nb) HIP_TRY(hipMemcpy(e->rep.nm_bytes, bytes + offsets[0], nb, hipMemcpyHostToDevice));
    std::vector<uint64_t> off(offsets, offsets + n + 1);
    for (auto& o : off) o -= offsets[0];
    HIP_TRY(hipMemcpy(e->rep.nm_off, off.data(), off.size() * 8, hipMemcpyHostToDevice));
    if (types) {
        SF_TRY(e->pool.alloc(&e->rep.nm_types, min16((size_t)n * 4)));
        if (n) HIP_TRY(hipMemcpy(e->rep.nm_types, types, (size_t)n * 4, hipMemcpyHostToDevice));
    }
    e->rep.n_names = n;
    return SF_OK;
}

// The metric log's buffers: the per-node ones and the events on first use,
// the per-row ones for `rows` rows, the scan / sort scratch for both.  A
// failure anywhere leaves none (ml_pool cleared), and the next call starts over.
static int ml_build(sf_engine* e, uint32_t rows) {
    auto& ml = e->rep.ml;
    DevPool& m = e->rep.ml_pool;
    const uint32_t nodes = e->R + 1;
    if (!ml.ready) {
        SF_TRY(m.alloc(&ml.mask, (size_t)nodes * 8));
        SF_TRY(m.alloc(&ml.counts, (size_t)nodes * 4));
        SF_TRY(m.alloc(&ml.offsets, (size_t)nodes * 4));
        SF_TRY(m.alloc(&ml.total, 4));
        SF_TRY(m.alloc(&ml.bytes, 8));
        for (auto& x : e->rep.ml_ev) if (!x) HIP_TRY(hipEventCreate(&x));
        ml.ready = true;
    }
    if (rows > ml.row_cap || !ml.row_cap) {
        const uint32_t cap = std::max<uint32_t>(rows, 1024);
        m.release_all(ml.rows, ml.keys, ml.order, ml.len, ml.off);
        ml.row_cap = 0;
        SF_TRY(m.alloc(&ml.rows, (size_t)cap * sizeof(sf_metric_row)));
        SF_TRY(m.alloc(&ml.keys, (size_t)cap * 2));
        SF_TRY(m.alloc(&ml.order, (size_t)cap * 8));
        SF_TRY(m.alloc(&ml.len, (size_t)cap * 8));
        SF_TRY(m.alloc(&ml.off, (size_t)cap * 8));
        ml.row_cap = cap;
    }
    size_t tb = 0;
    HIP_TRY(mlog_temp_bytes(nodes, ml.row_cap, &tb));
    return ml.tmp.reserve(m, tb);
}
static int ml_reserve(sf_engine* e, uint32_t rows) {
    const int rc = ml_build(e, rows);
    if (rc) { e->rep.ml_pool.clear(); e->rep.ml = {}; }
    return rc;
}

// line lengths -> offsets -> lines, copied to the caller's host buffer
static int ml_format(sf_engine* e, const uint32_t* order, uint32_t n, int64_t tz, char* out, uint64_t cap,
                     uint64_t* len_out) {
    hipStream_t s = e->stream;
    HIP_TRY(launch_fmt_len(e->rep.ml.rows, order, n, e->rep.nm_bytes, e->rep.nm_off, e->rep.nm_types, e->rep.n_names, tz, e->rep.ml.len,
                           e->rep.ml.off, e->rep.ml.bytes, e->rep.ml.tmp.p, e->rep.ml.tmp.bytes, s));
    uint64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, e->rep.ml.bytes, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *len_out = total;
    if (total > cap) return fail(SF_ERR_CAPACITY, "metric log bytes exceed cap");
    SF_TRY(e->rep.ml.out.reserve(e->rep.ml_pool, total));
    HIP_TRY(launch_fmt_write(e->rep.ml.rows, order, n, e->rep.nm_bytes, e->rep.nm_off, e->rep.nm_types, e->rep.n_names, tz, e->rep.ml.off,
                             (char*)e->rep.ml.out.p, s));
    HIP_TRY(hipEventRecord(e->rep.ml_ev[2], s));
    if (total) HIP_TRY(hipMemcpyAsync(out, e->rep.ml.out.p, total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return SF_OK;
}

int sf_metric_log(sf_engine* e, int64_t now_ms, int64_t tz_offset_ms, int include_entry_node, char* out,
                  uint64_t cap, uint64_t* len_out, uint32_t* n_lines) {
    if (!e || !len_out || (cap && !out)) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    SF_TRY(en_fence(e));
    *len_out = 0;
    if (n_lines) *n_lines = 0;
    SF_TRY(ml_reserve(e, 0));
    hipStream_t s = e->stream;
    const bool with_en = include_entry_node != 0;
    const uint32_t nodes = e->R + (with_en ? 1u : 0u);
    // the ENTRY_NODE line: this engine's node, or the one set by sf_set_report_entry_node
    // (its windows; lastFetchTime stays this engine's, MetricTimerListener.java:40-69)
    EntryNode* en = e->en;
    if (with_en && e->rep.report_set) {
        if (!e->rep.en_report) SF_TRY(e->pool.alloc(&e->rep.en_report, sizeof(EntryNode)));
        HIP_TRY(hipMemcpyAsync(e->rep.en_report, &e->rep.report, sizeof(EntryNode), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(&e->rep.en_report->last_fetch, &e->en->last_fetch, 8, hipMemcpyDeviceToDevice, s));
        en = e->rep.en_report;
    }
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    const unsigned grid = (unsigned)std::min<uint64_t>(((uint64_t)nodes + 3) / 4, (uint64_t)cus * 16);
    HIP_TRY(hipEventRecord(e->rep.ml_ev[0], s));
    HIP_TRY(launch_mlog_count(e->st, en, with_en, e->cfg.shard_count, e->cfg.shard_index, now_ms, e->rep.ml.mask,
                              e->rep.ml.counts, e->rep.ml.offsets, e->rep.ml.total, e->rep.ml.tmp.p, e->rep.ml.tmp.bytes, grid, e->rep.ml_ev[1], s));
    uint32_t rows = 0;
    HIP_TRY(hipMemcpyAsync(&rows, e->rep.ml.total, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    SF_TRY(ml_reserve(e, rows));
    uint32_t* ord = e->rep.ml.order;
    HIP_TRY(launch_mlog_rows(e->st, en, with_en, e->cfg.shard_count, e->cfg.shard_index, now_ms, e->rep.ml.mask,
                             e->rep.ml.offsets, rows, e->rep.ml.rows, e->rep.ml.keys, e->rep.ml.keys + e->rep.ml.row_cap, ord,
                             ord + e->rep.ml.row_cap, e->rep.ml.tmp.p, e->rep.ml.tmp.bytes, grid, s));
    if (n_lines) *n_lines = rows;
    if (en != e->en) HIP_TRY(hipMemcpyAsync(&e->en->last_fetch, &en->last_fetch, 8, hipMemcpyDeviceToDevice, s));
    SF_TRY(ml_format(e, ord + e->rep.ml.row_cap, rows, tz_offset_ms, out, cap, len_out));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e->rep.ml_ev[0], e->rep.ml_ev[1]) == hipSuccess) e->stats.metric_scan_ms = ms;
    if (hipEventElapsedTime(&ms, e->rep.ml_ev[0], e->rep.ml_ev[2]) == hipSuccess) e->stats.metric_log_ms = ms;
    return SF_OK;
}

int sf_format_metric_rows(sf_engine* e, const sf_metric_row* rows, uint32_t n, int64_t tz_offset_ms, char* out,
                          uint64_t cap, uint64_t* len_out) {
    if (!e || !len_out || (n && !rows) || (cap && !out)) return fail(SF_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(e->mu);
    *len_out = 0;
    SF_TRY(ml_reserve(e, n));
    if (n) HIP_TRY(hipMemcpyAsync(e->rep.ml.rows, rows, (size_t)n * sizeof(sf_metric_row), hipMemcpyHostToDevice,
                                  e->stream));
    return ml_format(e, nullptr, n, tz_offset_ms, out, cap, len_out);
}

}  // extern "C"
