// sf_launch.h — private header of the batch pipeline's translation units
// (sf_segs.hip, sf_decide.hip, sf_xwave.hip, sf_heavy.hip, sf_scatter.hip,
// sf_packed.hip, sf_state.hip): the launchers they call across files and the
// few helpers more than one of them uses.  A kernel is launched only from the
// file that defines it; launch_sort (sf_segs.hip) and launch_decide
// (sf_decide.hip) compose these launchers into the stream graph of a batch.
// What the host runtime calls is declared in sf_internal.h.
#pragma once
#include <algorithm>
#include <type_traits>

#include "sf_heavy.h"

namespace sf {

// ---------------------------------------------------------------- host helpers
static inline unsigned blocks(size_t n, unsigned t) { return (unsigned)((n + t - 1) / t); }

// the batch's sorted events for a kernel (t0 is read on the device: ev_open)
static inline SortedEv sorted_ev(const Work& w, const DevBatch& b) { return SortedEv{w.s_meta, w.perm, b.ts, b.cnt, 0}; }

// The kernels templated on the sample count exist for 2 and for
// SF_MAX_SAMPLE_COUNT: f(std::integral_constant<int, MAXS>) for the engine's S
template <class F>
static inline void for_sample_count(const DevState& st, F&& f) {
    if (st.S <= 2) f(std::integral_constant<int, 2>{});
    else f(std::integral_constant<int, SF_MAX_SAMPLE_COUNT>{});
}

struct LightLists { const uint32_t* list; const uint32_t* counts; uint32_t off[LCLS]; uint32_t cap[LCLS]; };

// Several buffer fills in one launch (each hipMemsetAsync is a launch of its
// own: the SystemRule planner's small sub-batches paid more for the launch gaps
// than for the bytes).  Range blockIdx.y: a byte head up to 16-B alignment,
// 16-B stores, a byte tail.
struct FillSet {
    static constexpr int MAX = 8;
    uint8_t* p[MAX]; size_t n[MAX]; uint32_t v[MAX];   // v: the byte repeated
    int k = 0;
    void add(void* ptr, size_t bytes, uint8_t byte) {
        if (!ptr || !bytes) return;
        p[k] = (uint8_t*)ptr; n[k] = bytes; v[k] = 0x01010101u * byte; k++;
    }
};
void launch_fill(const FillSet& f, hipStream_t s);                       // sf_state.hip (k_fill)

HeavyCtx heavy_ctx(const Work& w);                                       // sf_heavy.hip

// -------------------------------------------------------------- device helpers
// k_heavy_stream's segment list (sf_stream.h), also walked by k_fill_tiles and k_heavy_apply
struct StreamCtx {
    const uint32_t* list;
    const uint32_t* n_list;                         // Work::counters + WC_STREAM_FRONT: front count, then back count
    uint32_t seg_cap;
    uint64_t* sticks;
    uint32_t* next;                                 // work queue head (k_heavy_stream)
};

__device__ __forceinline__ bool stream_at(const StreamCtx& sc, uint32_t b, uint32_t* s) {
    const uint32_t nf = sc.n_list[0], nb = sc.n_list[WC_STREAM_BACK - WC_STREAM_FRONT];
    if (b < nf) { *s = sc.list[b]; return true; }
    if (b < nf + nb) { *s = sc.list[sc.seg_cap - 1 - (b - nf)]; return true; }
    return false;
}

// heavy-list entry of workgroup b: front part, then the back part
// (k_heavy_apply walks both lists: every heavy item segment is in one of them)
__device__ __forceinline__ bool heavy_at(const HeavyCtx& hc, uint32_t b, uint32_t* s) {
    const uint32_t nf = hc.n_heavy[0], nb = hc.n_heavy[WC_HEAVY_BACK - WC_HEAVY_FRONT];
    if (b < nf) { *s = hc.heavy_list[b]; return true; }
    if (b < nf + nb) { *s = hc.heavy_list[hc.seg_cap - 1 - (b - nf)]; return true; }
    return false;
}

// inclusive sum scan over the 64 lanes of a wavefront (DPP: row shifts, then row broadcasts)
__device__ __forceinline__ int wave_scan_add(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);     // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);     // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);     // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);     // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);     // row_bcast:15
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);     // row_bcast:31
    return v;
}
// (k_thr_heads, k_pk_count and the PAcc flushes)
__device__ inline unsigned long long wave_sum(unsigned long long v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ------------------------------------------------------------------- launchers
// Each takes the stream and the grid inputs launch_decide computes; none
// records or waits on an event except launch_classify's two timing records.
// sf_segs.hip: k_classify + k_fill_tiles (EV_CLASSIFY_START / EV_CLASSIFIED when timing)
void launch_classify(const DevState& st, Work& w, const DevBatch& b, hipStream_t s, hipEvent_t* ev, bool timing);
// sf_heavy.hip
void launch_thr_prep(Work& w, const DevBatch& b, hipStream_t s);
void launch_heavy_stream(const DevState& st, const SegIO& io, const HeavyCtx& hc, const StreamCtx& sc, const Work& w,
                         uint32_t max_heavy, hipStream_t s);
void launch_heavy_decide(const DevState& st, const SegIO& io, const HeavyCtx& hc, uint32_t max_heavy, hipStream_t s);
// cls 0: k_heavy_decide's list, 1: k_heavy_stream's
void launch_heavy_fill(const DevState& st, const SegIO& io, const HeavyCtx& hc, const Work& w, uint32_t fgrid, int cls,
                       hipStream_t s);
void launch_heavy_apply(const DevState& st, const HeavyCtx& hc, const StreamCtx& sc, const Work& w, uint32_t max_heavy,
                        int cls, hipStream_t s);
// sf_xwave.hip: k_decide_xw over Work::xw_list
void launch_xw(const DevState& st, const SegIO& io, const Work& w, uint32_t n, hipStream_t s);
// sf_xcluster.hip: k_decide_xcl over Work::xcl_list (engines with an embedded token server)
void launch_xcl(const DevState& st, const SegIO& io, const Work& w, uint32_t n, hipStream_t s);
// sf_scatter.hip: statuses of a decided batch, sorted order -> the caller's array (submission order)
void launch_scatter(Work& w, uint32_t n, uint8_t* o_status, hipStream_t s);

}  // namespace sf
