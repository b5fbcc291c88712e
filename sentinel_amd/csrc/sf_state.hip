// sf_state.hip — kernels on the engine's state outside a batch's phases (init,
// the per-resource rule summary, diagnostics reads) and the multi-range fill
// both phases use.  Product code.
#include "sf_launch.h"
#include "sf_xflow.h"

namespace sf {

__global__ void k_init_state(DevState st, size_t n_sec, size_t n_min) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t k = i; k < n_sec; k += stride) {
        st.second[k] = fresh_bucket(WS_NONE, st.max_rt);
        st.borrow[k].ws = WS_NONE; st.borrow[k].pass = 0;
    }
    for (size_t k = i; k < n_min; k += stride) st.minute[k] = fresh_bucket(WS_NONE, st.max_rt);
    for (size_t k = i; k < st.R; k += stride) st.threads[k] = 0;
}

__global__ void k_rdesc(DevState st, RDesc* out) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < st.R) out[r] = make_rdesc(st, r);
}
// after any change of rule_off / rules / prule_off / dg_rr_of
hipError_t launch_rdesc(const DevState& st, hipStream_t s) {
    hipLaunchKernelGGL(k_rdesc, dim3(blocks(st.R, 256)), dim3(256), 0, s, st, (RDesc*)st.rdesc);
    return hipGetLastError();
}

hipError_t launch_init_state(const DevState& st, hipStream_t s) {
    size_t n_sec = (size_t)st.R * st.S, n_min = (size_t)st.R * MINUTE;
    hipLaunchKernelGGL(k_init_state, dim3(2048), dim3(256), 0, s, st, n_sec, n_min);
    return hipGetLastError();
}

// occupancy and longest probe distance of the exact param table (diagnostics)
__global__ void k_param_stats(DevState st, unsigned long long* out) {
    unsigned long long used = 0, maxp = 0;
    const uint64_t cap = st.pcap_mask + 1;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * blockDim.x) {
        const ParamSlot& s = st.ptab[i];
        if (s.hi == 0) continue;
        used++;
        const uint64_t home = ParamTable::hash(s.hi, s.lo) & st.pcap_mask;
        const unsigned long long d = (i - home) & st.pcap_mask;
        if (d > maxp) maxp = d;
    }
    for (int o = 32; o > 0; o >>= 1) {
        used += __shfl_xor(used, o);
        const unsigned long long m = __shfl_xor(maxp, o);
        maxp = m > maxp ? m : maxp;
    }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&out[0], used); atomicMax(&out[1], maxp); }
}
hipError_t launch_param_stats(const DevState& st, unsigned long long* out, hipStream_t s) {
    hipMemsetAsync(out, 0, 16, s);
    hipLaunchKernelGGL(k_param_stats, dim3(2048), dim3(256), 0, s, st, out);
    return hipGetLastError();
}

// ParameterMetric.getThreadCount(index, value) (ParameterMetric.java:241-253) of one
// (local resource, param index, typed value): 0 when the value has no counter
__global__ void k_param_thread_read(DevState st, uint32_t l, int idx, uint32_t tag, uint64_t bits, long long* out) {
    if (threadIdx.x != 0) return;
    const ParamTable pt{st.ptab, st.pcap_mask, st.err, nullptr};
    *out = (long long)pm_thread_get(pt, l, idx, tag, bits);
}
hipError_t launch_param_thread_read(const DevState& st, uint32_t l, int idx, uint32_t tag, uint64_t bits,
                                    long long* out, hipStream_t s) {
    hipLaunchKernelGGL(k_param_thread_read, dim3(1), dim3(64), 0, s, st, l, idx, tag, bits, out);
    return hipGetLastError();
}

// sf_node_digests: one FNV-1a digest per resource row over its canonical
// sf_node_state words (absent buckets: SF_WS_ABSENT and zeros), in the word
// order of include/sentinel_flow.h.  A verification read, not a hot path: one
// thread per row walks the row's ~4 KB.
__device__ __forceinline__ uint64_t fnv_w(uint64_t h, int64_t w) { h ^= (uint64_t)w; return h * 0x100000001b3ull; }
__device__ __forceinline__ uint64_t fnv_bucket(uint64_t h, const Bucket& b) {
    if (b.ws == WS_NONE) {
        h = fnv_w(h, SF_WS_ABSENT);
        for (int k = 0; k < 7; k++) h = fnv_w(h, 0);
        return h;
    }
    h = fnv_w(h, b.ws); h = fnv_w(h, b.pass); h = fnv_w(h, b.block); h = fnv_w(h, b.exc);
    h = fnv_w(h, b.succ); h = fnv_w(h, b.rt); h = fnv_w(h, b.occ); return fnv_w(h, b.min_rt);
}
__global__ void k_node_digests(DevState st, uint32_t n, unsigned long long* out) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n) return;
    const NodeRows r = cluster_rows(st, l);
    uint64_t h = 0xcbf29ce484222325ull;
    for (int i = 0; i < st.S; i++) {
        h = fnv_bucket(h, r.sec[i]);
        const Borrow b = r.bor[i];
        h = fnv_w(h, b.ws == WS_NONE ? SF_WS_ABSENT : b.ws);
        h = fnv_w(h, b.ws == WS_NONE ? 0 : b.pass);
    }
    for (int i = 0; i < MINUTE; i++) h = fnv_bucket(h, r.min[i]);
    out[l] = fnv_w(h, *r.thr);
}
hipError_t launch_node_digests(const DevState& st, uint32_t n, unsigned long long* out, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_node_digests, dim3((n + 255) / 256), dim3(256), 0, s, st, n, out);
    return hipGetLastError();
}

// the ranges of a FillSet (sf_launch.h), range blockIdx.y
__global__ void k_fill(FillSet f) {
    const int r = blockIdx.y;
    uint8_t* p = f.p[r];
    const size_t n = f.n[r];
    const uint32_t v = f.v[r];
    size_t head = (16 - ((uintptr_t)p & 15)) & 15;
    if (head > n) head = n;
    const size_t body = (n - head) / 16, tail0 = head + body * 16;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    if (t < head) p[t] = (uint8_t)v;
    if (t < n - tail0) p[tail0 + t] = (uint8_t)v;
    uint4* q = (uint4*)(p + head);
    const uint4 w = make_uint4(v, v, v, v);
    for (size_t i = t; i < body; i += stride) q[i] = w;
}
void launch_fill(const FillSet& f, hipStream_t s) {
    if (!f.k) return;
    size_t most = 0;
    for (int r = 0; r < f.k; r++) most = std::max(most, f.n[r] / 16 + 16);
    hipLaunchKernelGGL(k_fill, dim3((unsigned)std::min<size_t>(2048, (most + 255) / 256), (unsigned)f.k), dim3(256), 0, s, f);
}

}  // namespace sf
