// sf_concur.h — cluster concurrency tokens (product code): batched
// DefaultTokenService.requestConcurrentToken / releaseConcurrentToken and the
// RegularExpireStrategy sweep.
//
// Reference (CS = sentinel-cluster/sentinel-cluster-server-default/src/main/java/com/alibaba/csp/sentinel/cluster):
//   DefaultTokenService            CS/flow/DefaultTokenService.java:66-93
//   ConcurrentClusterFlowChecker   CS/flow/ConcurrentClusterFlowChecker.java:36-101
//   CurrentConcurrencyManager      CS/flow/statistic/concurrent/CurrentConcurrencyManager.java
//   TokenCacheNode                 CS/flow/statistic/concurrent/TokenCacheNode.java
//   RegularExpireStrategy          CS/flow/statistic/concurrent/expire/RegularExpireStrategy.java:94-136
//   ClusterFlowRuleManager         CS/flow/rule/ClusterFlowRuleManager.java:271-375
//
// The first part of this file, the chunk solver, is plain C++ behind a small
// wave seam (prefix sum, ballot, broadcast): the device walk runs it on one
// wavefront, the CPU suite runs the same code on a plain-loop wave
// (SF_HOSTSIM, tests/hostsim/concur_check.cpp).
//
// HBM layout (second part):
//   slots   [cap]     CcSlot (40 B): the token pool, indexed by the id's slot bits
//   stack   [cap]     free slot numbers, `top` of them (CcCounters.top)
//   claim   [cap]     per call: lowest request index releasing the slot
//   now     [n_flow]  int32 nowCalls of a flow rule (CurrentConcurrencyManager)
//   cfg     [n_flow]  the rule's two time-outs
#pragma once
#include <stdint.h>
#ifndef SF_HOSTSIM
#include "sf_token.h"
#endif

#ifndef SF_HD
#ifdef SF_HOSTSIM
#define SF_HD inline
#else
#define SF_HD __host__ __device__ __forceinline__
#endif
#endif

namespace sf {

// ---------------------------------------------------------------- chunk solver
// A chunk is up to 64 consecutive requests of one flowId in batch order, lane l
// holding the signed delta d[l]: +count of an acquire, -count of a release that
// removes its token, 0 for an unused lane.  The reference decides them one by
// one (ConcurrentClusterFlowChecker.java:57-70, :96-98; Java int arithmetic):
//     d < 0:  x += d
//     d > 0:  blocked iff (double)(int)(x + d) > thr, else x += d
// The solver gives the same pass mask and the same final x in a few wave-wide
// steps.  With A the inclusive prefix sum of d and R that of min(d, 0), and x_s
// the exact value of x before lane s (x_0 = x):
//   peel     under "every acquire from s on passes", x after lane l is
//            x_s + A[l] - A[s-1].  If no acquire lane exceeds thr there, the
//            hypothesis holds for every lane by induction and all pass.  Else
//            the first such lane f saw only passes before it, so its x is
//            exact: s..f-1 pass, f is blocked, x_f = x_s + A[f-1] - A[s-1].
//   shortcut under "no acquire after f passes", x before lane l is
//            x_f + R[l] - R[f].  If every acquire after f exceeds thr there,
//            that hypothesis holds by induction and all are blocked (the
//            saturated regime: one round per chunk).  Else the first acquire
//            g that does not exceed saw only blocked acquires before it, so
//            f+1..g-1 are blocked, g passes, and the peel resumes at s = g.
// Both inductions use each lane's exact predecessor state, not monotonicity,
// so they hold under int wrap-around too.  All sums are taken modulo 2^32.
struct CcSolveCount { uint32_t all_pass = 0, rounds = 0; };

SF_HD bool cc_over(uint32_t v, double thr) { return (double)(int32_t)v > thr; }
SF_HD int cc_ctz(uint64_t m) { return __builtin_ctzll(m); }

// W: the wave seam.  W::Vec is one int32 per lane; w.map(f) builds one from
// f(lane), w.at(v, l) reads lane l's own element inside f, w.scan(v) is the
// inclusive prefix sum, w.ballot(f) the mask of lanes with f(lane), and
// w.bcast(v, l) lane l's element for every lane.  Control flow is wave-uniform.
template <class W>
SF_HD uint64_t cc_solve_chunk(W& w, const typename W::Vec& d, double thr, int32_t* x, CcSolveCount* cnt) {
    using V = typename W::Vec;
    const V A = w.scan(d);
    const V R = w.scan(w.map([&](int l) { const int32_t v = w.at(d, l); return v < 0 ? v : 0; }));
    const uint64_t acq = w.ballot([&](int l) { return w.at(d, l) > 0; });
    uint64_t pass = 0;
    int s = 0;
    uint32_t xs = (uint32_t)*x, a_prev = 0;          // x before lane s, A[s-1]
    for (uint32_t round = 0;; round++) {
        cnt->rounds++;
        const uint32_t base = xs - a_prev;
        const uint64_t from_s = ~0ull << s;
        const uint64_t fail = w.ballot([&](int l) { return cc_over(base + (uint32_t)w.at(A, l), thr); }) & acq & from_s;
        if (!fail) {
            pass |= acq & from_s;
            xs = base + (uint32_t)w.bcast(A, 63);
            if (round == 0) cnt->all_pass++;
            break;
        }
        const int f = cc_ctz(fail);
        pass |= acq & from_s & ((1ull << f) - 1);
        const uint32_t xf = base + (uint32_t)w.bcast(A, f) - (uint32_t)w.bcast(d, f);
        if (f == 63) { xs = xf; break; }
        const uint64_t after = ~0ull << (f + 1);
        const uint32_t rbase = xf - (uint32_t)w.bcast(R, f);
        const uint64_t ok = w.ballot([&](int l) {
            return !cc_over(rbase + (uint32_t)w.at(R, l) + (uint32_t)w.at(d, l), thr); }) & acq & after;
        if (!ok) { xs = rbase + (uint32_t)w.bcast(R, 63); break; }
        s = cc_ctz(ok);
        xs = rbase + (uint32_t)w.bcast(R, s);         // (R[s] == R[s-1]: lane s is an acquire)
        a_prev = (uint32_t)w.bcast(A, s) - (uint32_t)w.bcast(d, s);
    }
    *x = (int32_t)xs;
    return pass;
}

// the seam on the host: a wave is 64 array elements and every step a plain loop
struct CcWaveHost {
    struct Vec { int32_t v[64]; };
    template <class F> Vec map(F f) const { Vec r; for (int l = 0; l < 64; l++) r.v[l] = f(l); return r; }
    int32_t at(const Vec& v, int l) const { return v.v[l]; }
    Vec scan(const Vec& v) const {
        Vec r; uint32_t a = 0;
        for (int l = 0; l < 64; l++) { a += (uint32_t)v.v[l]; r.v[l] = (int32_t)a; }
        return r;
    }
    template <class F> uint64_t ballot(F f) const {
        uint64_t m = 0;
        for (int l = 0; l < 64; l++) if (f(l)) m |= 1ull << l;
        return m;
    }
    int32_t bcast(const Vec& v, int l) const { return v.v[l]; }
};

}  // namespace sf

#ifndef SF_HOSTSIM
namespace sf {

constexpr uint32_t CC_SLOT_BITS = 28;
constexpr uint32_t CC_SLOT_MASK = (1u << CC_SLOT_BITS) - 1;
constexpr uint64_t CC_MAX_SLOTS = 1ull << CC_SLOT_BITS;
constexpr uint32_t CC_NONE = 0xFFFFFFFFu;
constexpr int64_t CC_DEFAULT_TIMEOUT = 2000;      // ClusterFlowConfig: resourceTimeout, clientOfflineTime

#if defined(__HIPCC__)
// the seam on the device: a lane's element lives in its register
struct CcWaveDev {
    using Vec = int32_t;
    int lane;
    template <class F> __device__ __forceinline__ Vec map(F f) const { return f(lane); }
    __device__ __forceinline__ int32_t at(const Vec& v, int) const { return v; }
    __device__ __forceinline__ Vec scan(Vec v) const {
        uint32_t a = (uint32_t)v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t u = (uint32_t)__shfl_up((int)a, o, 64);
            if (lane >= o) a += u;
        }
        return (int32_t)a;
    }
    template <class F> __device__ __forceinline__ uint64_t ballot(F f) const { return __ballot(f(lane)); }
    __device__ __forceinline__ int32_t bcast(const Vec& v, int l) const { return __shfl(v, l, 64); }
};
#endif

struct CcSlot {                  // TokenCacheNode, 40 B
    int64_t flow_id, client_deadline, resource_deadline;
    int32_t count; uint32_t client;
    uint32_t gen, live;          // gen: 28 bits, +1 each time the slot is freed
};
struct CcCfg { int64_t resource_timeout, client_offline; };
struct CcCounters {
    unsigned long long chunks, chunks_all_pass, rounds, expired;
    uint32_t top, pad;           // free slots on the stack
};
struct CcState {
    CcSlot* slots; uint32_t cap;
    uint32_t* stack; uint32_t* claim;
    int32_t* now; const CcCfg* cfg;
    CcCounters* ctr;
};
struct CcBatch {
    uint32_t n;
    const uint8_t* op; const int64_t* id; const int32_t* count; const uint32_t* client; const int64_t* ts;
};
struct CcOut { int8_t* status; int64_t* token_id; };
struct CcWork {                  // sized for `cap` requests and `nf_cap` flow rules
    uint32_t* key_in; uint32_t* key_out; uint32_t* idx_in; uint32_t* idx_out;
    int32_t* delta;              // [n] signed delta of a request that reaches the walk
    uint32_t* rslot;             // [n] pool slot a release claims (CC_NONE: none)
    uint32_t* seg_lo; uint32_t* seg_hi;     // [n_flow] a flow rule's range in the sorted order
    void* sort_tmp; size_t sort_bytes;
    uint32_t cap, nf_cap;
};

hipError_t cc_query_temp(uint32_t max_n, size_t* sort_bytes);
hipError_t cc_launch(const TokState& ts, const CcState& cs, CcWork& w, const CcBatch& b, const CcOut& out, hipStream_t s);
// slots [lo, hi) pushed on the free stack, their claim words cleared
hipError_t cc_push_range(const CcState& cs, uint32_t lo, uint32_t hi, hipStream_t s);
hipError_t cc_expire(const TokState& ts, const CcState& cs, int64_t now, const uint8_t* online, uint32_t n_clients,
                     hipStream_t s);

}  // namespace sf
#endif
