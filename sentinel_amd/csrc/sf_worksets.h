// sf_worksets.h — the work sets whose sizing needs no device: the scratch
// buffers of the token server (TokWork), the concurrency tokens (CcWork) and
// the circuit breakers (DegradeWork), each beside the pool that owns them, and
// the functions that grow them (the rule of sf_mem.h: capacity last, a failure
// leaves an empty set).  The sort / scan scratch sizes come from a query the
// caller passes: rocPRIM's in the engine, a constant in tests/mem_check.cpp.
#pragma once
#include <algorithm>

#include "sf_concur.h"
#include "sf_degrade.h"
#include "sf_mem.h"
#include "sf_rls.h"
#include "sf_token.h"

namespace sf {

template <class W> struct WorkSet {
    W w{};
    DevPool pool;
    explicit WorkSet(const MemOps& ops) : pool(ops) {}
    void reset() { pool.clear(); w = W{}; }
    // build(): the allocations of a growth step; a failure empties the set
    template <class F> int grow(F build) {
        const int rc = build();
        if (rc) reset();
        return rc;
    }
};

struct TokWorkSet : WorkSet<TokWork> {
    using WorkSet::WorkSet;
    uint32_t cap = 0;                         // requests the set is sized for (TokWork has no field for it)
};
using TokTempQuery = int (*)(uint32_t n, size_t* sort8, size_t* sort64, size_t* scan);

inline int tok_work_ensure(TokWorkSet& s, uint32_t n, uint32_t max_batch, TokTempQuery query) {
    if (n <= s.cap) return 0;
    s.reset();
    s.cap = 0;
    const size_t N = std::max(n, max_batch);
    TokWork& w = s.w;
    DevPool& m = s.pool;
    return s.grow([&]() -> int {
        SF_TRY(m.alloc(&w.nskey_in, min16(N))); SF_TRY(m.alloc(&w.nskey_out, min16(N)));
        SF_TRY(m.alloc(&w.idx_in, min16(N * 4))); SF_TRY(m.alloc(&w.idx_out, min16(N * 4)));
        SF_TRY(m.alloc(&w.key_in, min16(N * 8))); SF_TRY(m.alloc(&w.key_out, min16(N * 8)));
        SF_TRY(m.alloc(&w.rule_of, min16(N * 4))); SF_TRY(m.alloc(&w.pending, min16(N)));
        SF_TRY(m.alloc(&w.head, std::max<size_t>(N, 512) * 4)); SF_TRY(m.alloc(&w.head_scan, min16(N * 4)));
        SF_TRY(m.alloc(&w.seg_start, min16((N + 1) * 4))); SF_TRY(m.alloc(&w.n_seg, min16(4)));
        SF_TRY(query((uint32_t)N, &w.sort8_bytes, &w.sort64_bytes, &w.scan_bytes));
        SF_TRY(m.alloc(&w.sort8_tmp, min16(w.sort8_bytes)));
        SF_TRY(m.alloc(&w.sort64_tmp, min16(w.sort64_bytes)));
        SF_TRY(m.alloc(&w.scan_tmp, min16(w.scan_bytes)));
        s.cap = (uint32_t)N;
        return 0;
    });
}

// RlsWork (sf_rls.h) beside the TokWork it is used with: room for n requests and n descriptors
using RlsWorkSet = WorkSet<RlsWork>;

inline int rls_work_ensure(RlsWorkSet& s, uint32_t n, uint32_t max_batch) {
    if (n <= s.w.cap) return 0;
    s.reset();
    const size_t N = std::max(n, max_batch);
    RlsWork& w = s.w;
    DevPool& m = s.pool;
    return s.grow([&]() -> int {
        SF_TRY(m.alloc(&w.dom, min16(N * sizeof(RlsKey)))); SF_TRY(m.alloc(&w.req_err, min16(N)));
        SF_TRY(m.alloc(&w.d_req, min16(N * 4))); SF_TRY(m.alloc(&w.d_fid, min16(N * 8)));
        SF_TRY(m.alloc(&w.d_ts, min16(N * 8))); SF_TRY(m.alloc(&w.d_cnt, min16(N * 4)));
        SF_TRY(m.alloc(&w.ctr, sizeof(RlsCounters)));
        w.cap = (uint32_t)N;
        return 0;
    });
}

// CcWork carries its capacities (cap requests, nf_cap flow rules): reset() zeroes them
using CcWorkSet = WorkSet<CcWork>;
using CcTempQuery = int (*)(uint32_t n, size_t* sort_bytes);

inline int cc_work_ensure(CcWorkSet& s, uint32_t n, uint32_t nf, CcTempQuery query) {
    if (n <= s.w.cap && nf <= s.w.nf_cap) return 0;
    const size_t N = std::max(n, s.w.cap), F = std::max({nf, s.w.nf_cap, 1u});
    s.reset();
    CcWork& w = s.w;
    DevPool& m = s.pool;
    return s.grow([&]() -> int {
        SF_TRY(m.alloc(&w.key_in, min16(N * 4))); SF_TRY(m.alloc(&w.key_out, min16(N * 4)));
        SF_TRY(m.alloc(&w.idx_in, min16(N * 4))); SF_TRY(m.alloc(&w.idx_out, min16(N * 4)));
        SF_TRY(m.alloc(&w.delta, min16(N * 4))); SF_TRY(m.alloc(&w.rslot, min16(N * 4)));
        SF_TRY(m.alloc(&w.seg_lo, min16(F * 4))); SF_TRY(m.alloc(&w.seg_hi, min16(F * 4)));
        SF_TRY(query((uint32_t)N, &w.sort_bytes));
        SF_TRY(m.alloc(&w.sort_tmp, min16(w.sort_bytes)));
        w.cap = (uint32_t)N; w.nf_cap = (uint32_t)F;
        return 0;
    });
}

// DegradeWork carries cap (events) and beg_cap (breaker resources) too
using DegradeWorkSet = WorkSet<DegradeWork>;
using DgTempQuery = int (*)(uint32_t n, uint32_t key_bits, size_t* bytes);

// room for n events over n_rres breaker resources; the sort scratch follows
// the event capacity and the key width (dg_drop_sort_tmp when that changes)
inline int dg_work_ensure(DegradeWorkSet& s, uint32_t n, uint32_t n_rres, uint32_t key_bits, DgTempQuery query) {
    DegradeWork& w = s.w;
    DevPool& m = s.pool;
    return s.grow([&]() -> int {
        if (n > w.cap) {
            m.release_all(w.keys_in, w.keys_out, w.idx_in, w.idx_out, w.sev, w.inv);
            SF_TRY(m.alloc(&w.keys_in, (size_t)n * 4)); SF_TRY(m.alloc(&w.keys_out, (size_t)n * 4));
            SF_TRY(m.alloc(&w.idx_in, (size_t)n * 4)); SF_TRY(m.alloc(&w.idx_out, (size_t)n * 4));
            SF_TRY(m.alloc(&w.sev, (size_t)n * sizeof(DgEv))); SF_TRY(m.alloc(&w.inv, (size_t)n * 4));
            m.release(w.sort_tmp);
            w.sort_tmp_bytes = 0;
            w.cap = n;
        }
        if (!w.sort_tmp) {
            size_t bytes = 0;
            SF_TRY(query(w.cap, key_bits, &bytes));
            SF_TRY(m.alloc(&w.sort_tmp, nz(bytes)));
            w.sort_tmp_bytes = bytes;
        }
        if (n_rres > w.beg_cap || !w.beg) {
            m.release_all(w.beg, w.end, w.heavy);
            const uint32_t c = std::max<uint32_t>(n_rres, 1);
            SF_TRY(m.alloc(&w.beg, (size_t)c * 4)); SF_TRY(m.alloc(&w.end, (size_t)c * 4));
            SF_TRY(m.alloc(&w.heavy, (size_t)c * 4));
            w.beg_cap = c;
        }
        if (!w.err) SF_TRY(m.alloc(&w.err, 4));
        if (!w.n_heavy) SF_TRY(m.alloc(&w.n_heavy, 4));
        return 0;
    });
}
// a reload changed the key width: the scratch is sized again by the next batch
inline void dg_drop_sort_tmp(DegradeWorkSet& s) {
    s.pool.release(s.w.sort_tmp);
    s.w.sort_tmp_bytes = 0;
}

}  // namespace sf
