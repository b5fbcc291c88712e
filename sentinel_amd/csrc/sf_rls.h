// sf_rls.h — Envoy rate-limit service, batched shouldRateLimit (product code).
//
// Reference (RLS = sentinel-cluster/sentinel-cluster-server-envoy-rls/src/main/java/
// com/alibaba/csp/sentinel/cluster/server/envoy/rls):
//   SentinelEnvoyRlsServiceImpl.shouldRateLimit   RLS/service/v3/SentinelEnvoyRlsServiceImpl.java:34-85
//   checkToken / generateKey                      RLS/service/v3/SentinelEnvoyRlsServiceImpl.java:99-117
//   EnvoySentinelRuleConverter.generateFlowId     RLS/rule/EnvoySentinelRuleConverter.java:68-74
//   SimpleClusterFlowChecker.acquireClusterToken  RLS/flow/SimpleClusterFlowChecker.java:33-65
//
// The first half needs neither the HIP runtime nor a device (tests/rls_check.cpp
// runs it on the host under the sanitizers, with SF_RLS_KEYS_ONLY defined): the
// UTF-8 decoder / validator, the running String.hashCode over UTF-16 code
// units, StringUtil.isBlank and the flowId of a key.  It is the one
// implementation behind the key kernels and sf_rls_flow_id.  The second half is
// the device interface of sf_rls.hip and the per-descriptor decision.
//
// A key is never built in memory: key = domain ("|" key "|" value)*, and
// String.hashCode is a left fold, so the state after the domain (RlsKey) is
// computed once per request and every descriptor continues from a copy of it.
//
// Character.isWhitespace (Java 11+), all in the BMP:
//   0009-000D, 001C-001F, 0020, 1680, 2000-2006, 2008-200A, 2028, 2029, 205F, 3000
// (U+180E is not whitespace since Java 11 / Unicode 6.3; 00A0, 2007 and 202F
// are the no-break spaces Java excludes).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stdint.h>

#ifndef SF_HD
#if defined(__HIPCC__)
#define SF_HD __host__ __device__ __forceinline__
#else
#define SF_HD inline
#endif
#endif

namespace sf {

// segments of at least this many descriptors take the wave route (one
// wavefront per segment), shorter ones one lane each
constexpr uint32_t RLS_WAVE_MIN = 256;
constexpr int RLS_CHUNK = 64;        // descriptors solved at once by the wave route: one per lane
constexpr int RLS_LANE_T = 64;       // lanes per workgroup of the lane route (LDS: one ClFlowState per lane)
constexpr int RLS_T = 256;           // lanes per workgroup of the per-request / per-descriptor kernels

struct RlsKey {
    uint32_t h;          // String.hashCode of the code units so far (wrapping 32-bit)
    uint8_t blank;       // every character so far is whitespace (an empty key is blank)
    uint8_t ok;          // 0: ill-formed UTF-8 met
};
SF_HD RlsKey rls_key_begin() { return RlsKey{0u, 1, 1}; }

SF_HD bool rls_is_whitespace(uint32_t cp) {
    return (cp >= 0x0009 && cp <= 0x000D) || (cp >= 0x001C && cp <= 0x0020) || cp == 0x1680 ||
           (cp >= 0x2000 && cp <= 0x2006) || (cp >= 0x2008 && cp <= 0x200A) || cp == 0x2028 || cp == 0x2029 ||
           cp == 0x205F || cp == 0x3000;
}
// one code point: its UTF-16 code units enter the hash (a supplementary one as its surrogate pair)
SF_HD void rls_key_cp(RlsKey& k, uint32_t cp) {
    if (cp < 0x10000u) {
        k.h = 31u * k.h + cp;
    } else {
        const uint32_t v = cp - 0x10000u;
        k.h = 31u * k.h + (0xD800u + (v >> 10));
        k.h = 31u * k.h + (0xDC00u + (v & 0x3FFu));
    }
    k.blank = (uint8_t)(k.blank && rls_is_whitespace(cp));
}
// The UTF-8 string p[0, len) appended to the key.  Ill-formed (k.ok = 0, the
// rest of the string is not read): a lone or missing continuation byte, an
// overlong form (C0, C1, E0 80-9F, F0 80-8F), a sequence cut by the string's
// end, a code point D800-DFFF or above 10FFFF (F4 90+, F5-F7), bytes F8-FF.
SF_HD void rls_key_feed(RlsKey& k, const uint8_t* p, uint32_t len) {
    uint32_t i = 0;
    while (i < len) {
        const uint32_t b0 = p[i];
        if (b0 < 0x80u) { rls_key_cp(k, b0); i++; continue; }
        uint32_t need, cp, min;
        if (b0 < 0xC2u) { k.ok = 0; return; }                    // continuation byte, or overlong C0 / C1
        else if (b0 < 0xE0u) { need = 1; cp = b0 & 0x1Fu; min = 0x80u; }
        else if (b0 < 0xF0u) { need = 2; cp = b0 & 0x0Fu; min = 0x800u; }
        else if (b0 < 0xF5u) { need = 3; cp = b0 & 0x07u; min = 0x10000u; }
        else { k.ok = 0; return; }
        if (len - i <= need) { k.ok = 0; return; }               // cut by the string's end
        for (uint32_t j = 1; j <= need; j++) {
            const uint32_t c = p[i + j];
            if ((c & 0xC0u) != 0x80u) { k.ok = 0; return; }
            cp = (cp << 6) | (c & 0x3Fu);
        }
        if (cp < min || cp > 0x10FFFFu || (cp >= 0xD800u && cp <= 0xDFFFu)) { k.ok = 0; return; }
        rls_key_cp(k, cp);
        i += need + 1;
    }
}
// EnvoySentinelRuleConverter.generateFlowId of a well-formed key
SF_HD int64_t rls_key_id(const RlsKey& k) {
    if (k.blank) return -1;                                      // StringUtil.isBlank(key)
    return (int64_t)INT32_MAX + (int64_t)(int32_t)k.h;
}

}  // namespace sf

#ifndef SF_RLS_KEYS_ONLY
#include "sf_token.h"

namespace sf {

struct RlsBatch {                // device pointers (sf_rls_batch staged or in place)
    uint32_t n, n_desc, n_ent, n_str, n_bytes;
    const int64_t* ts; const int32_t* hits; const uint32_t* desc_off;
    const int64_t* desc_fid;     // pre-hashed form, or null
    const uint32_t* domain; const uint32_t* ent_off; const uint32_t* ent_key; const uint32_t* ent_val;
    const uint32_t* str_off; const uint8_t* bytes;
};
struct RlsOut { uint8_t* overall; uint8_t* code; int32_t* limit; int32_t* remaining; int64_t* flow_id; };
struct RlsCounters {             // of one call; the engine sums them into sf_rls_stats
    unsigned long long error_requests, no_rule, segs_lane, segs_wave, chunks, chunks_serial, rounds;
    uint32_t n_wave, pad;        // segments listed for the wave route (list: TokWork::head)
};
struct RlsWork {                 // beside the TokWork of the engine; cap requests and cap descriptors
    RlsKey* dom;                 // [n] key state after the domain (string form)
    uint8_t* req_err;            // [n] a string of the request is ill-formed (string form)
    uint32_t* d_req;             // [n_desc] request of a descriptor
    int64_t* d_fid;              // [n_desc] flowId that is looked up
    int64_t* d_ts; int32_t* d_cnt;   // [n_desc] time and acquireCount of a descriptor that reaches the checker
    RlsCounters* ctr;
    uint32_t cap;
};

#if defined(__HIPCC__)
// SimpleClusterFlowChecker.acquireClusterToken (:41-64) for one descriptor on
// its rule's ClusterMetric; thr = rule.count * exceedCount
__device__ __forceinline__ void rls_decide(ClMetric& m, double thr, int64_t t, int32_t c, uint8_t* code, int32_t* rem) {
    const double latest = m.avg(CE_PASS, t);
    const double next = thr - latest - c;
    if (next >= 0) {
        m.add(CE_PASS, c, t); m.add(CE_PASS_REQUEST, 1, t);
        *code = SF_RLS_OK; *rem = j_d2i(next);
    } else {
        m.add(CE_BLOCK, c, t); m.add(CE_BLOCK_REQUEST, 1, t);
        *code = SF_RLS_OVER_LIMIT; *rem = 0;
    }
}
#endif

// {n_desc, n_ent, n_bytes} of a batch in device memory (b.n, b.n_str and the table pointers set) -> d_out[3]
hipError_t rls_lengths(const RlsBatch& b, uint32_t* d_out, hipStream_t s);
// One sf_request_rls on stream s.  The tables are checked first
// (*ts.err = SF_ERR_INVALID and nothing is decided).  The call synchronises
// once, between the segment table and the decide kernels, to launch only the
// routes that have segments.  wave_min: segments of at least that many
// descriptors take the wave route.
hipError_t rls_launch(const TokState& ts, TokWork& w, const RlsWork& rw, const RlsBatch& b, const RlsOut& out,
                      uint32_t wave_min, hipStream_t s);

}  // namespace sf
#endif
