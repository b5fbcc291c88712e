// sf_concur.hip — gfx950 kernels of one sf_request_concurrent and of the
// expiry sweep (product code; layout and chunk solver in sf_concur.h).
//
//   k_cc_prep     DefaultTokenService.requestConcurrentToken validation and rule
//                 lookup; a release reads its pool slot and claims it for the
//                 lowest request index (atomic min)
//   k_cc_keys     the claim's winner is the release that removes the token
//                 (RELEASE_OK, delta -count), the others ALREADY_RELEASE; key of
//                 a request that changes nowCalls: its flow rule index
//   radix sort    (key, index), stable: a flowId's requests in batch order
//   k_cc_bounds   each flow rule's range in the sorted order
//   k_cc_walk     one wavefront per flowId, 64 requests per step through
//                 cc_solve_chunk; nowCalls carried in a register
//   k_cc_commit   a passed acquire pops a slot, writes its node and its id
//   k_cc_free     a removing release frees its slot (generation + 1)
//   k_cc_expire   RegularExpireStrategy.clearToken over the whole pool
#include <algorithm>
#include <cstring>
#include <rocprim/rocprim.hpp>

#include "sf_concur.h"

namespace sf {

constexpr int8_t CC_PENDING = 100;

static inline unsigned cblocks(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

__device__ __forceinline__ bool cc_live(const CcState& cs, uint64_t tid, uint32_t* slot_out) {
    const uint32_t slot = (uint32_t)tid & CC_SLOT_MASK, gen = (uint32_t)(tid >> CC_SLOT_BITS) & CC_SLOT_MASK;
    if ((tid >> 56) == 0 || slot >= cs.cap) return false;
    const CcSlot& s = cs.slots[slot];
    if (!s.live || s.gen != gen) return false;
    *slot_out = slot;
    return true;
}

__global__ void k_cc_prep(TokState ts, CcState cs, CcBatch b, CcWork w, CcOut out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.n) return;
    const uint8_t op = b.op[i];
    const int64_t id = b.id[i];
    int8_t st = CC_PENDING;
    uint32_t key = CC_NONE, rs = CC_NONE;
    int32_t delta = 0;
    if (op == SF_CC_ACQUIRE) {
        const int32_t c = b.count[i];
        const int32_t r = id > 0 ? id_lookup(ts, id, false) : -1;
        // sharded token server: only the rule's owner decides (sf_token_shard)
        const uint32_t owner = id <= 0 ? 0u : (r >= 0 ? ts.rules[r].owner : (uint32_t)((uint64_t)id % ts.shard_count));
        if (owner != ts.shard_index) *ts.err = SF_ERR_INVALID;
        if (b.client[i] == SF_CLIENT_NONE || id <= 0 || c <= 0) st = SF_TOKEN_BAD_REQUEST;   // DefaultTokenService :68-70
        else if (r < 0) st = SF_TOKEN_NO_RULE_EXISTS;                                       // :73-76
        else { key = (uint32_t)r; delta = c; }
    } else if (op == SF_CC_RELEASE) {
        const uint64_t tid = (uint64_t)id;
        const uint32_t sh = (uint32_t)(tid >> 56);
        if (sh != 0 && sh - 1 != ts.shard_index) *ts.err = SF_ERR_INVALID;
        uint32_t slot;
        if (!cc_live(cs, tid, &slot)) st = SF_TOKEN_ALREADY_RELEASE;           // getTokenCacheNode == null :82-86
        else {
            const int32_t r = id_lookup(ts, cs.slots[slot].flow_id, false);
            if (r < 0) st = SF_TOKEN_NO_RULE_EXISTS;                           // :87-91, the token stays
            else {
                rs = slot; key = (uint32_t)r; delta = -cs.slots[slot].count;
                atomicMin(&cs.claim[slot], i);
            }
        }
    } else {
        *ts.err = SF_ERR_INVALID;
        st = SF_TOKEN_BAD_REQUEST;
    }
    w.key_in[i] = key;
    w.delta[i] = delta;
    w.rslot[i] = rs;
    out.status[i] = st;
    out.token_id[i] = 0;
}

__global__ void k_cc_keys(CcState cs, uint32_t n, uint32_t n_flow, CcWork w, CcOut out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t key = w.key_in[i];
    const uint32_t rs = w.rslot[i];
    if (rs != CC_NONE) {
        if (cs.claim[rs] == i) out.status[i] = SF_TOKEN_RELEASE_OK;            // removeTokenCacheNode != null :92-100
        else { out.status[i] = SF_TOKEN_ALREADY_RELEASE; key = CC_NONE; w.rslot[i] = CC_NONE; w.delta[i] = 0; }
    }
    w.key_in[i] = key == CC_NONE ? n_flow : key;                               // (sorts last)
    w.idx_in[i] = i;
}

__global__ void k_cc_bounds(const uint32_t* key, uint32_t n, uint32_t n_flow, uint32_t* lo, uint32_t* hi) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const uint32_t k = key[j];
    if (k >= n_flow) return;
    if (j == 0 || key[j - 1] != k) lo[k] = j;
    if (j == n - 1 || key[j + 1] != k) hi[k] = j + 1;
}

constexpr int CW_T = 256;        // k_cc_walk: four wavefronts per workgroup, one flowId each

// ConcurrentClusterFlowChecker.acquireConcurrentToken / releaseConcurrentToken on
// nowCalls of one flowId, its requests in batch order, 64 per step.
__global__ void __launch_bounds__(CW_T) k_cc_walk(TokState ts, CcState cs, CcWork w, CcOut out) {
    const uint32_t r = (blockIdx.x * CW_T + threadIdx.x) >> 6;
    if (r >= ts.n_flow || *ts.err) return;               // a refused batch (k_cc_prep) decides nothing
    const uint32_t lo = w.seg_lo[r], hi = w.seg_hi[r];
    if (hi <= lo) return;
    CcWaveDev wave{(int)(threadIdx.x & 63)};
    const ClRule& rule = ts.rules[r];
    // calcGlobalThreshold :36-46 (getConnectedCount: 0 when the namespace is not loaded)
    const int32_t connected = rule.ns >= 0 ? ts.ns[rule.ns].connected : 0;
    const double thr = rule.threshold_type == SF_THRESHOLD_GLOBAL ? rule.count : rule.count * connected;
    int32_t x = cs.now[r];
    CcSolveCount cnt;
    uint32_t chunks = 0;
    auto load = [&](uint32_t p, uint32_t* idx, int32_t* d) {
        const uint32_t j = p + (uint32_t)wave.lane;
        *idx = j < hi ? w.idx_out[j] : CC_NONE;
        *d = j < hi ? w.delta[*idx] : 0;
    };
    uint32_t idx, nidx = CC_NONE;
    int32_t d, nd = 0;
    load(lo, &idx, &d);
    for (uint32_t p = lo; p < hi; p += 64) {
        if (p + 64 < hi) load(p + 64, &nidx, &nd);          // the next chunk's loads fly during this solve
        const uint64_t pass = cc_solve_chunk(wave, d, thr, &x, &cnt);
        if (d > 0) out.status[idx] = ((pass >> wave.lane) & 1) ? SF_TOKEN_OK : SF_TOKEN_BLOCKED;
        chunks++;
        idx = nidx; d = nd;
    }
    if (wave.lane == 0) {
        cs.now[r] = x;
        atomicAdd(&cs.ctr->chunks, (unsigned long long)chunks);
        atomicAdd(&cs.ctr->chunks_all_pass, (unsigned long long)cnt.all_pass);
        atomicAdd(&cs.ctr->rounds, (unsigned long long)cnt.rounds);
    }
}

__device__ __forceinline__ void cc_push(const CcState& cs, uint32_t slot) {
    const uint32_t k = atomicAdd(&cs.ctr->top, 1u);
    if (k < cs.cap) cs.stack[k] = slot;
}

// TokenCacheNode.generateTokenCacheNode + putTokenCacheNode :74-77.  The host
// made sure the stack holds a slot for every request of the batch.
__global__ void k_cc_commit(TokState ts, CcState cs, CcBatch b, CcWork w, CcOut out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b.n || *ts.err) return;
    if (w.delta[i] <= 0 || out.status[i] != SF_TOKEN_OK) return;
    const uint32_t k = atomicSub(&cs.ctr->top, 1u) - 1u;
    if (k >= cs.cap) { *ts.err = SF_ERR_CAPACITY; return; }
    const uint32_t slot = cs.stack[k];
    if (slot >= cs.cap) { *ts.err = SF_ERR_CAPACITY; return; }
    const uint32_t r = w.key_in[i];
    const int64_t t = b.ts[i];
    CcSlot& s = cs.slots[slot];
    s.flow_id = b.id[i];
    s.client_deadline = wadd(t, cs.cfg[r].client_offline);
    s.resource_deadline = wadd(t, cs.cfg[r].resource_timeout);
    s.count = b.count[i];
    s.client = b.client[i];
    s.live = 1;
    out.token_id[i] = (int64_t)(((uint64_t)(ts.shard_index + 1) << 56) | ((uint64_t)s.gen << CC_SLOT_BITS) | slot);
}

__device__ __forceinline__ void cc_remove(const CcState& cs, uint32_t slot) {
    CcSlot& s = cs.slots[slot];
    s.live = 0;
    s.gen = (s.gen + 1) & CC_SLOT_MASK;
    cc_push(cs, slot);
}

// (a release that lost its claim has rslot CC_NONE since k_cc_keys: the winner
// clears the slot's claim word, also in a refused batch)
__global__ void k_cc_free(CcState cs, uint32_t n, CcWork w, const int32_t* refused) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t rs = w.rslot[i];
    if (rs == CC_NONE) return;
    cs.claim[rs] = CC_NONE;
    if (!*refused) cc_remove(cs, rs);
}

__global__ void k_cc_push_range(CcState cs, uint32_t lo, uint32_t hi) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (lo + k >= hi) return;
    cs.claim[lo + k] = CC_NONE;
    cc_push(cs, lo + k);
}

// RegularExpireStrategy.clearToken :94-136 at `now`, every live token
__global__ void k_cc_expire(TokState ts, CcState cs, int64_t now, const uint8_t* online, uint32_t n_clients) {
    uint32_t removed = 0;
    for (uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x; slot < cs.cap; slot += gridDim.x * blockDim.x) {
        const CcSlot s = cs.slots[slot];
        if (!s.live) continue;
        const bool is_online = s.client < n_clients && online[s.client];
        const int32_t r = id_lookup(ts, s.flow_id, false);
        bool rm = !is_online && wsub(s.client_deadline, now) < 0;                           // :110-114
        // (a token whose rule is gone is kept here: the reference throws at :118)
        if (!rm && r >= 0) rm = wsub(now, s.resource_deadline) > cs.cfg[r].resource_timeout;   // :118-122
        if (!rm) continue;
        cc_remove(cs, slot);
        if (r >= 0) atomicSub(&cs.now[r], s.count);                                        // removeToken :126-136
        removed++;
    }
    if (removed) atomicAdd(&cs.ctr->expired, (unsigned long long)removed);
}

hipError_t cc_query_temp(uint32_t max_n, size_t* sort_bytes) {
    return rocprim::radix_sort_pairs(nullptr, *sort_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                     (uint32_t*)nullptr, max_n, 0u, 32u);
}

hipError_t cc_push_range(const CcState& cs, uint32_t lo, uint32_t hi, hipStream_t s) {
    if (hi <= lo) return hipSuccess;
    hipLaunchKernelGGL(k_cc_push_range, dim3(cblocks(hi - lo, 256)), dim3(256), 0, s, cs, lo, hi);
    return hipGetLastError();
}

hipError_t cc_expire(const TokState& ts, const CcState& cs, int64_t now, const uint8_t* online, uint32_t n_clients,
                     hipStream_t s) {
    if (!cs.cap) return hipSuccess;
    const unsigned blocks = std::min<unsigned>(cblocks(cs.cap, 256), 2048u);
    hipLaunchKernelGGL(k_cc_expire, dim3(blocks), dim3(256), 0, s, ts, cs, now, online, n_clients);
    return hipGetLastError();
}

hipError_t cc_launch(const TokState& ts, const CcState& cs, CcWork& w, const CcBatch& b, const CcOut& out, hipStream_t s) {
    const uint32_t n = b.n, nf = ts.n_flow;
    if (!n) return hipSuccess;
    const unsigned T = 256;
    hipLaunchKernelGGL(k_cc_prep, dim3(cblocks(n, T)), dim3(T), 0, s, ts, cs, b, w, out);
    hipLaunchKernelGGL(k_cc_keys, dim3(cblocks(n, T)), dim3(T), 0, s, cs, n, nf, w, out);
    unsigned bits = 1;
    while (bits < 32 && (nf >> bits)) bits++;                  // keys are 0 .. n_flow
    hipError_t e = rocprim::radix_sort_pairs(w.sort_tmp, w.sort_bytes, w.key_in, w.key_out, w.idx_in, w.idx_out, n, 0u,
                                             bits, s);
    if (e != hipSuccess) return e;
    if (nf) {
        hipMemsetAsync(w.seg_lo, 0, (size_t)nf * 4, s);
        hipMemsetAsync(w.seg_hi, 0, (size_t)nf * 4, s);
        hipLaunchKernelGGL(k_cc_bounds, dim3(cblocks(n, T)), dim3(T), 0, s, w.key_out, n, nf, w.seg_lo, w.seg_hi);
        hipLaunchKernelGGL(k_cc_walk, dim3(cblocks((size_t)nf * 64, CW_T)), dim3(CW_T), 0, s, ts, cs, w, out);
    }
    hipLaunchKernelGGL(k_cc_commit, dim3(cblocks(n, T)), dim3(T), 0, s, ts, cs, b, w, out);
    hipLaunchKernelGGL(k_cc_free, dim3(cblocks(n, T)), dim3(T), 0, s, cs, n, w, ts.err);
    return hipGetLastError();
}

}  // namespace sf
