// sf_gateway.hip — gfx950 kernels of one sf_gateway_args (product code): a batch
// of gateway requests becomes the argument columns of an ordinary
// sf_event_batch, as GatewayParamParser.parseParameterFor would fill the args
// of each entry (sf_gateway.h).
//
//   k_gw_check      offset tables non-decreasing and starting at 0, every
//                   string index < n_str, every resource on this shard, every
//                   entry's event position inside [0, n_total) and claimed by
//                   one entry only (own[pos] = entry, by compare-and-swap)
//   k_gw_check_exit every exit_pos inside [0, n_total), not a gateway entry,
//                   its entry_ref a gateway entry of this batch
//                   (either: *err = SF_ERR_INVALID and nothing is written)
//   k_gw_args       one lane per entry: the event columns and the slots
//   k_gw_exits      one lane per listed EXIT: its entry's arguments
//
// One lane per entry: an entry has at most GW_MAX_SLOTS slots and scans its
// request's few values linearly; values and patterns are read byte by byte
// inside their own [str_off[s], str_off[s + 1]), so the last string of the
// table is as safe as any other.
#include <algorithm>

#include "sf_gateway.h"

namespace sf {

constexpr int GW_T = 256;
static inline unsigned gblocks(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

__global__ void k_gw_lengths(GwBatch b, uint32_t* out) {
    out[0] = b.res_off[b.n];
    out[1] = b.val_off[b.n];
    out[2] = b.str_off[b.n_str];
}
hipError_t gw_lengths(const GwBatch& b, uint32_t* d_out, hipStream_t s) {
    hipLaunchKernelGGL(k_gw_lengths, dim3(1), dim3(1), 0, s, b, d_out);
    return hipGetLastError();
}

__global__ void __launch_bounds__(GW_T) k_gw_check(GwTables t, GwBatch b, uint32_t* own, int32_t* err) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i == 0) bad |= b.res_off[0] != 0 || b.val_off[0] != 0;
    if (i < b.n) bad |= b.res_off[i] > b.res_off[i + 1] || b.val_off[i] > b.val_off[i + 1] || b.ev_index[i] > b.n_total;
    if (i < b.n_val) bad |= b.val_str[i] >= b.n_str;
    if (i < b.n_str) bad |= b.str_off[i] > b.str_off[i + 1];
    if (i < b.n_ent) {
        const uint32_t res = b.res_id[i];
        bad |= res % t.shard_count != t.shard_index || res / t.shard_count >= t.R;
        // (with a decreasing res_off the request found is arbitrary: the position is checked before it is used)
        const uint32_t req = gw_req_of(b, i);
        const uint64_t pos = (uint64_t)b.ev_index[req] + (uint64_t)(i - b.res_off[req]);
        if (i < b.res_off[req] || pos >= b.n_total) bad = true;
        else bad |= atomicCAS(&own[pos], GW_NONE, i) != GW_NONE;
    }
    if (bad) *err = SF_ERR_INVALID;
}

__global__ void __launch_bounds__(GW_T) k_gw_check_exit(GwBatch b, const uint32_t* own, int32_t* err) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= b.n_exit) return;
    const uint32_t p = b.exit_pos[k];
    bool bad = p >= b.n_total;
    if (!bad) {
        const int64_t ref = b.entry_ref[p];
        bad = own[p] != GW_NONE || ref < 0 || ref >= (int64_t)b.n_total;
        if (!bad) bad = own[ref] == GW_NONE;
    }
    if (bad) *err = SF_ERR_INVALID;
}

__global__ void __launch_bounds__(GW_T) k_gw_args(GwTables t, GwBatch b, GwOut o) {
    const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= b.n_ent) return;
    gw_entry(t, b, o, d);
}

__global__ void __launch_bounds__(GW_T) k_gw_exits(GwBatch b, GwOut o) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= b.n_exit) return;
    const uint32_t p = b.exit_pos[k];
    const size_t ref = (size_t)b.entry_ref[p];
    o.n_args[p] = o.n_args[ref];
    for (int a = 0; a < GW_MAX_SLOTS; a++) {
        o.arg_tag[(size_t)a * b.n_total + p] = o.arg_tag[(size_t)a * b.n_total + ref];
        o.arg_bits[(size_t)a * b.n_total + p] = o.arg_bits[(size_t)a * b.n_total + ref];
    }
}

hipError_t gw_launch(const GwTables& t, const GwBatch& b, const GwOut& o, uint32_t* own, int32_t* err, int32_t* err_host,
                     hipStream_t s) {
    const unsigned T = GW_T;
    hipError_t e = hipMemsetAsync(own, 0xFF, std::max<size_t>(b.n_total, 1) * 4, s);
    if (e != hipSuccess) return e;
    const size_t most = std::max<size_t>({b.n, b.n_ent, b.n_val, b.n_str, 1});
    hipLaunchKernelGGL(k_gw_check, dim3(gblocks(most, T)), dim3(T), 0, s, t, b, own, err);
    if (b.n_exit) hipLaunchKernelGGL(k_gw_check_exit, dim3(gblocks(b.n_exit, T)), dim3(T), 0, s, b, own, err);
    if ((e = hipMemcpyAsync(err_host, err, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    if (*err_host) return hipSuccess;
    if (b.n_ent) hipLaunchKernelGGL(k_gw_args, dim3(gblocks(b.n_ent, T)), dim3(T), 0, s, t, b, o);
    if (b.n_exit) hipLaunchKernelGGL(k_gw_exits, dim3(gblocks(b.n_exit, T)), dim3(T), 0, s, b, o);
    return hipGetLastError();
}

}  // namespace sf
