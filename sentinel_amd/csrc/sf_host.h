// sf_host.h — what the files of the host runtime share (internal; the C-ABI is
// include/sentinel_flow.h): the error helpers, the engine with one struct per
// subsystem, and the few helpers that cross files.
//   sf_engine.cpp        create / destroy, the rule loaders, the submit paths,
//                        the SystemRule rounds, the read-backs, comm, utilities
//   sf_host_cluster.cpp  token server, wire framing, RLS, concurrency tokens
//   sf_host_degrade.cpp  DegradeSlot circuit breakers
//   sf_host_gateway.cpp  API-gateway flow rules: the gateway list, the request parser
//   sf_host_report.cpp   metric snapshot and metrics.log
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "sf_decide.h"
#include "sf_pkargs.h"
#include "sf_xflow.h"
#include "sf_sysx.h"
#include "sf_token.h"
#include "sf_concur.h"
#include "sf_wire.h"
#include "sf_rls.h"
#include "sf_gateway.h"
#include "sf_degrade.h"
#include "sf_mem.h"
#include "sf_worksets.h"
#include <rccl/rccl.h>

using namespace sf;

// the call's error text (one thread-local, sf_engine.cpp) and its code
int fail(int code, const std::string& msg);
#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess)                                                           \
            return fail(_e == hipErrorOutOfMemory ? SF_ERR_NOMEM : SF_ERR_DEVICE,       \
                        std::string(#expr ": ") + hipGetErrorString(_e));               \
    } while (0)

// The backend of sf_mem.h: the only place where device and pinned host memory
// is allocated or freed.  Every pointer belongs to a DevPool: the engine's, a
// slot's two, a work set's, or a call's scratch pool (freed when the call returns).
static int hip_alloc_failed(const char* what, hipError_t e) {
    return fail(SF_ERR_NOMEM, std::string(what) + ": " + hipGetErrorString(e));
}
static int hip_dev_alloc(void** p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    return e == hipSuccess ? SF_OK : hip_alloc_failed("hipMalloc", e);
}
static int hip_host_alloc(void** p, size_t bytes) {
    const hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
    return e == hipSuccess ? SF_OK : hip_alloc_failed("hipHostMalloc", e);
}
static const MemOps HIP_MEM{hip_dev_alloc, [](void* p) { hipFree(p); }, hip_host_alloc, [](void* p) { hipHostFree(p); }};

// the copy callables of a StagePlan (sf_mem.h): on stream s, a failure is the call's SF_ERR_DEVICE
inline auto h2d_on(hipStream_t s) {
    return [s](void* dst, const void* src, size_t bytes) -> int {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
        return SF_OK;
    };
}
inline auto d2h_on(hipStream_t s) {
    return [s](void* dst, const void* src, size_t bytes) -> int {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
        return SF_OK;
    };
}

// cluster token server (sf_token.hip), its wire framing (sf_wire.hip)
struct TokHost {
    TokState ts{};
    TokWorkSet tw{HIP_MEM};
    std::vector<sf_namespace> host_ns;
    std::vector<sf_cluster_flow_rule> host_cflow;
    std::vector<sf_cluster_param_rule> host_cparam;
    std::vector<sf_hot_item> host_citems;
    std::vector<int64_t> cflow_ids;           // flow rule index -> flowId
    GrowBuf stage;
    int64_t* d_sum = nullptr;
    GrowBuf wire_arena;                                  // sf_serve_frames scratch
};

// cluster concurrency tokens (sf_concur.hip): the device state with the host's
// view of it as of the last call
struct CcHost {
    CcState cs{};
    CcWorkSet ws{HIP_MEM};
    CcCounters ctr{};                 // device counters after the last call (ctr.top: free slots)
    uint64_t grows = 0;
    std::vector<sf_concurrent_config> cfg;    // sf_load_concurrent_config
    GrowBuf stage, online;
};

// Envoy rate-limit service (sf_rls.hip): decided on the token server's state and work set
struct RlsHost {
    RlsWorkSet ws{HIP_MEM};
    GrowBuf stage;
    uint32_t* len = nullptr;                             // [3] table lengths of a device-memory batch
    uint32_t wave_min = RLS_WAVE_MIN;                    // diagnostics (SF_RLS_WAVE=0): every segment on the lane route
    sf_rls_stats stats{};
};

// API-gateway flow rules (sf_gateway.hip): the converted rules (the gateway list
// of the ParamFlow stage) and the parser's tables, in the engine's pool
struct GwHost {
    GwTables t{};                                        // t.of null: no gateway rule loaded
    std::vector<sf_param_rule> rules;                    // the gateway list (sf_gateway_convert's order)
    std::vector<sf_hot_item> items;
    GrowBuf stage, own;                                  // sf_gateway_args staging; [n_total] entry of an event position
    uint32_t* len = nullptr;                             // [8]: table lengths of a device-memory batch, a zero, the error word
};

// DegradeSlot circuit breakers (sf_degrade.hip)
struct DgHost {
    DegradeDev dev{};
    DegradeWorkSet ws{HIP_MEM};
    std::vector<uint32_t> pos;            // breaker index (load order) -> CSR position
    std::vector<sf_degrade_rule> rules;   // the valid rules of the loaded breakers (load order)
    GrowBuf stage;
};

// the metric snapshot (sf_entry.hip) and metrics.log (sf_metric.hip)
struct ReportHost {
    // sf_set_report_entry_node: the ENTRY_NODE sf_metric_log writes (node-wide merge), host copy
    bool report_set = false;
    EntryNode report{};
    EntryNode* en_report = nullptr;    // device staging of `report` for the metric kernels
    uint32_t* snap_counts = nullptr; uint32_t* snap_offsets = nullptr; uint32_t* snap_total = nullptr;
    void* snap_scan = nullptr; size_t snap_scan_bytes = 0;
    bool snap_ready = false;           // the four above are allocated
    GrowBuf snap_rows;
    char* nm_bytes = nullptr; uint64_t* nm_off = nullptr; int32_t* nm_types = nullptr; uint32_t n_names = 0;
    struct MetricLog {                 // ml_reserve: the per-node buffers (ready) and the per-row ones (row_cap)
        unsigned long long* mask = nullptr; uint32_t* counts = nullptr; uint32_t* offsets = nullptr;
        uint32_t* total = nullptr; uint64_t* bytes = nullptr;
        bool ready = false;
        sf_metric_row* rows = nullptr; uint8_t* keys = nullptr; uint32_t* order = nullptr;
        uint64_t* len = nullptr; uint64_t* off = nullptr; uint32_t row_cap = 0;
        GrowBuf out, tmp;
    } ml;
    DevPool ml_pool{HIP_MEM};
    hipEvent_t ml_ev[3]{};
};

// sharded SystemRules, the per-window exchange (sf_sysx.h, sf_submit_node), and
// the node-wide aggregate over the ranks of a node (RCCL over xGMI)
struct SxHost {
    int64_t* msg = nullptr;               // this rank's message [SX_WORDS] (+ the setup words)
    GrowBuf recv;
    int64_t* seq = nullptr;               // [max_batch] device copy of host sequence numbers
    uint8_t* ibuf = nullptr;              // [max_batch] inert flags of the round
    std::vector<int64_t> hsend, hrecv;    // host side of a callback all-gather
    int64_t* wmsg = nullptr;              // the wide kinds: this rank's message [SXW_WORDS]
    SxwSeg* wsegs = nullptr;              // [SXW_MAX_SEGS] device copy of a round's settled runs
    std::vector<SxwSeg> whsegs;
    int64_t* agg = nullptr;               // [ws (S+60) | gws (S+60) | vals ((S+60)*6+1) | minrt (S+60)]
};

// a device copy of host event arrays, remembered by their addresses (stage_in_events)
struct StageBuf {
    GrowBuf buf; const void* key[5] = {}; uint32_t n = 0;
    int64_t fp[3] = {};                                     // ts[0], ts[n-1], flags[0] of the staged arrays
    const uint8_t* st_src = nullptr; uint32_t st_n = 0;    // verdicts [0, st_n) of st_src already staged
};

// compact batches (sf_submit_packed): the device copy of the packed input of
// one slot's batch, its SoA expansion and the verdicts copied back
struct PkStage {
    GrowBuf buf;
    // ParamFlow arguments, elements, contexts (and staged origins), sized by the
    // batch: [0, a_in) the staged sparse inputs (free at `consumed`), [a_in,
    // a_in + a_x) what the expansion writes and the decide phase reads (free at
    // the slot's `end`).  The boundary moves only when the buffer is reallocated.
    GrowBuf abuf; size_t a_in = 0, a_x = 0;
    hipEvent_t h2d = nullptr, d2h = nullptr;
    hipEvent_t consumed = nullptr;     // the packed inputs expanded (the next H2D into them may start)
    bool d2h_pending = false, consumed_pending = false;
    const uint8_t* out_status = nullptr;   // host verdicts of the async batch in flight (sf_sync_packed)
    int32_t* err_host = nullptr;           // its error flag, copied back with its verdicts (pinned)
    // sf_sparse_verdicts of that batch: the caller's struct, the list lengths
    // (pinned, copied back with the status bytes), the device lists
    bool sparse = false;
    sf_sparse_verdicts sp{};
    uint32_t* sp_counts = nullptr;
    const unsigned long long* sp_wl = nullptr; const unsigned long long* sp_rl = nullptr;
};

// Everything one batch in flight owns.  Batch k sorts into slot k % SF_SLOTS
// while batch k-1 is decided; a synchronous batch does not advance the slot.
// The count stays 2: the wait in take_slot ("two submits ago") and the packed
// stage's reuse rules (submit_packed) are argued for two slots, and whether
// the pipeline is correct with three is not established.
constexpr int SF_SLOTS = 2;
struct Slot {
    Work w{};                       // the sorted-order buffers (allocated on first use: ready)
    DevPool wpool{HIP_MEM};         // owns them
    bool ready = false;
    bool used = false;              // a batch has been enqueued into the slot (its events are recorded)
    bool timed = false;             // that batch ran with timing on and is not yet in stats
    hipEvent_t sorted = nullptr;    // its sort phase is enqueued (the decide streams wait for it)
    hipEvent_t done = nullptr;      // its verdicts are scattered: the Work set is free
    hipEvent_t end = nullptr;       // done and its ENTRY_NODE update (which reads the caller's batch)
    hipEvent_t core = nullptr;      // its verdicts are written (the packed D2H copy waits for it)
    hipEvent_t evs[SF_NUM_EVENTS]{};   // fork / join and timing events of its batch
    PkStage pk;
    DevPool pkpool{HIP_MEM};        // owns the packed stage's buffers
    // [max_batch] effective flags of its batch (the AuthorityRule mark pass,
    // sf_authority.hip), in wpool; allocated once rules are loaded.  Read by
    // the batch up to `end`.
    uint8_t* aflags = nullptr;
};

struct sf_engine {
    sf_config cfg{};
    // owns everything below that has no pool of its own: the state tables, the
    // rule tables, the staging buffers, the origin / context node pool
    DevPool pool{HIP_MEM};
    DevPool user_dev{HIP_MEM}, user_host{HIP_MEM};   // sf_device_alloc / sf_host_alloc
    hipStream_t stream = nullptr, stream2 = nullptr, stream3 = nullptr, stream4 = nullptr;   // 4: the wave walk
    hipStream_t sstream = nullptr;  // sort phase of the next batch (overlaps the decide phase on `stream`)
    // ENTRY_NODE's update of an asynchronous batch (after its verdicts, beside
    // the next batch's decide phase: decisions read ENTRY_NODE only with
    // SystemRules, whose batches are synchronous); ev_en: the last one enqueued,
    // en_async: `stream` is not yet ordered after it (en_fence)
    hipStream_t enstream = nullptr;
    bool en_own = false;            // enstream is a stream of its own (else one of the decide streams)
    int side_mode = 3;
    hipEvent_t ev_en = nullptr;
    bool en_async = false;
    bool serial = false;            // diagnostics (SF_SERIAL_STREAMS=1): every kernel on one stream
    uint32_t R = 0, key_bits = 1;
    DevState st{};
    Slot slot[SF_SLOTS];
    int cur = 0, last = 0;          // slot of the next / last submitted batch
    unsigned pending = 0;           // slots (bit k) with an asynchronous batch not yet checked by sf_sync
    SysRule sys{};                  // SystemRuleManager statics; sys.check: batches go through the planner
    SysPlanDev* sys_plan = nullptr; SysExitQ* sys_pa = nullptr; SysEntQ* sys_pb = nullptr;
    uint8_t* sys_ibuf = nullptr;                  // the planner's inert flags (sys_plan)
    uint8_t* sys_mask = nullptr;    // [max_batch] planner verdicts (sf_system.h)
    // rules
    std::vector<uint32_t> flow_pos;        // loaded valid rule index -> CSR position
    uint32_t n_flow = 0, n_prule = 0;      // n_prule: both lists of the ParamFlow stage
    std::vector<sf_param_rule> host_prules;    // the list of sf_load_param_rules (the gateway list: gw.rules)
    std::vector<sf_hot_item> host_pitems;
    AuthTables auth{};                     // AuthorityRule tables in `pool` (auth.of null: no rule loaded)
    // the exact ParamFlow table's fill (param_reserve): inserts counted on the
    // device (st.pins), as of the last drain; upper bound of the inserts of
    // batches enqueued since; the most keys one event can insert
    uint64_t p_used = 0, p_pending = 0, p_kmax = 0, p_grows = 0;
    // staging for host-memory batches
    GrowBuf stage_in, stage_out;
    StageBuf plan_sb, en_sb;                       // sf_system_plan / sf_entry_node_add inputs
    bool timing = false;
    sf_stats stats{};
    std::mutex mu;
    // the subsystems beside the submit pipeline, one struct and one file each
    TokHost tok;
    CcHost cc;
    RlsHost rls;
    GwHost gw;
    DgHost dg;
    ReportHost rep;
    SxHost sx;
    // ENTRY_NODE (sf_entry.hip)
    EntryNode* en = nullptr;
    EntryAcc* en_acc = nullptr;
    ncclComm_t comm = nullptr;
    // embedded token server (sf_load_cluster_binds; xgroups_rebuild): host copies of the flow rule
    // tables the groups are rebuilt from, the raw rule array's CSR positions (-1: dropped as invalid)
    // and cluster_mode flags, the binds, and the device tables DevState::emb points to
    std::vector<DevRule> host_rules;
    std::vector<uint32_t> host_rule_off;
    std::vector<int32_t> flow_csr_of;
    std::vector<uint8_t> flow_cluster;
    std::vector<sf_cluster_bind> binds;
    EmbState* emb_dev = nullptr;
    int64_t* emb_bind = nullptr;
    unsigned long long* emb_stats = nullptr;      // [2] EmbState::stats
    uint32_t xcl_min = XCL_MIN;                   // diagnostics (SF_XCL_MIN=<n>): k_decide_xcl's shortest segment
    // xflow walk (sf_xflow.h): group keys and the origin / context node pool
    uint32_t* xmap_buf = nullptr;
    uint8_t* xw_buf = nullptr;
    // the pool's chunks (host mirror of the device directory st.ax_chunks) and
    // the index table's growth (sf_origin.hip); counts for sf_stats
    std::vector<AuxChunk> ax_host;
    AuxChunk* ax_dir = nullptr;
    uint64_t aux_grows = 0;
    // copy streams of compact batches (PkStage): H2D(k+1), decide(k) and D2H(k-1) overlap
    hipStream_t h2d = nullptr, d2h = nullptr;
    int32_t* rh_err = nullptr;            // rehash_table's overflow flag
};

// ---- helpers of sf_engine.cpp that the other files call (the caller holds e->mu)
// Drain asynchronously submitted batches and report the first error of any of them
int drain(sf_engine* e, bool all = false);
// the xflow groups and the embedded token server's tables from the host copies of the flow rules,
// binds, cluster rules and namespaces (drained)
int xgroups_rebuild(sf_engine* e);
// token state present (rules built, namespace limiter allocated)
int tok_ready(sf_engine* e);
// order `stream` after the last asynchronous ENTRY_NODE update
int en_fence(sf_engine* e);
// resource id -> local row of this shard (0: not this shard's)
int local_of(const sf_engine* e, uint32_t res, uint32_t* l);
// the slot's effective-flags array of the AuthorityRule mark pass
int slot_aflags(sf_engine* e, Slot& sl);
// the device's ParamFlow tables from the gateway list and the list of sf_load_param_rules (drained)
int install_param_rules(sf_engine* e, const std::vector<sf_param_rule>& gw, const std::vector<sf_hot_item>& gwi,
                        const sf_param_rule* rules, uint32_t n, const sf_hot_item* items, uint32_t n_items);
