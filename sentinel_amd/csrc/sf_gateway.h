// sf_gateway.h — API-gateway flow rules (product code): the request-item parser
// of GatewayParamParser.parseParameterFor and the validity rules of
// GatewayRuleManager, shared by the kernels of sf_gateway.hip, the host
// conversion (sf_gateway_convert, sf_rules.cpp) and sf_gateway_string_bits.
//
// Reference (GW = sentinel-adapter/sentinel-api-gateway-adapter-common/src/main/java/
// com/alibaba/csp/sentinel/adapter/gateway/common):
//   GatewayRuleManager.isValidRule / isValidParamItem     GW/rule/GatewayRuleManager.java:117-145
//   applyGatewayRuleInternal                              GW/rule/GatewayRuleManager.java:179-237
//   GatewayRuleConverter.applyToParamRule                 GW/rule/GatewayRuleConverter.java:37-86
//   GatewayParamParser.parseParameterFor / parseInternal  GW/param/GatewayParamParser.java:51-174
//
// Everything but the two launch declarations at the end needs neither the HIP
// runtime nor a device: with SF_GATEWAY_HOST_ONLY defined,
// tests/gateway_check.cpp runs the match and hash code on the host under the
// sanitizers, and tools/gateway_host.cpp times gw_entry, the per-entry body of
// the kernel, on one core.
//
// String identity.  A parsed value enters ParamFlow as (SF_TAG_STRING, FNV-1a 64
// of its UTF-8 bytes); "$NM" and "$D" are hashed like any value, so a request
// value "$NM" equals the constant as it does in Java.  Values and patterns are
// compared byte by byte: String.equals / String.contains for well-formed UTF-8
// on both sides (a UTF-8 sequence is never a proper infix of another one's
// encoding at a different alignment).  Nothing validates UTF-8, and no byte
// outside [p, p + len) of a string is read.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif
#include <stddef.h>
#include <stdint.h>

#ifndef SF_HD
#if defined(__HIPCC__)
#define SF_HD __host__ __device__ __forceinline__
#else
#define SF_HD inline
#endif
#endif

#if defined(__HIPCC__)
#define SF_GW_UNROLL _Pragma("unroll")
#else
#define SF_GW_UNROLL
#endif

namespace sf {

constexpr int GW_MAX_SLOTS = 4;                    // == SF_MAX_ARGS
constexpr uint32_t GW_NONE = 0xFFFFFFFFu;          // == SF_GW_NONE
constexpr uint8_t GW_NOMATCH = 0x01;               // == SF_GW_NOMATCH
constexpr uint8_t GW_TAG_NULL = 0, GW_TAG_STRING = 3;   // == SF_TAG_NULL / SF_TAG_STRING
constexpr uint8_t GW_EV_KEEP = 0x02 | 0x04;             // == SF_EV_IN | SF_EV_PRIO: the flag bits a request carries
constexpr int32_t GW_GATE_ANY = -1, GW_GATE_NEVER = -2;
// SentinelGatewayConstants.PARAM_MATCH_STRATEGY_*
constexpr int32_t GW_MATCH_EXACT = 0, GW_MATCH_PREFIX = 1, GW_MATCH_REGEX = 2, GW_MATCH_CONTAINS = 3;

constexpr uint64_t GW_FNV_SEED = 0xcbf29ce484222325ULL, GW_FNV_PRIME = 0x100000001b3ULL;
SF_HD uint64_t gw_hash(const uint8_t* p, uint32_t len) {
    uint64_t h = GW_FNV_SEED;
    for (uint32_t i = 0; i < len; i++) { h ^= p[i]; h *= GW_FNV_PRIME; }
    return h;
}
// gw_hash of "$NM" (GATEWAY_NOT_MATCH_PARAM) and "$D" (GATEWAY_DEFAULT_PARAM)
constexpr uint64_t gw_hash_lit(const char* s) {
    uint64_t h = GW_FNV_SEED;
    for (; *s; s++) { h ^= (uint8_t)*s; h *= GW_FNV_PRIME; }
    return h;
}
constexpr uint64_t GW_BITS_NM = gw_hash_lit("$NM"), GW_BITS_D = gw_hash_lit("$D");

SF_HD bool gw_equal(const uint8_t* v, uint32_t vl, const uint8_t* p, uint32_t pl) {
    if (vl != pl) return false;
    for (uint32_t i = 0; i < vl; i++)
        if (v[i] != p[i]) return false;
    return true;
}
// p occurs in v (pl >= 1): every start is tried, so overlapping prefixes ("aab" in "aaab") are found
SF_HD bool gw_contains(const uint8_t* v, uint32_t vl, const uint8_t* p, uint32_t pl) {
    if (pl > vl) return false;
    for (uint32_t s = 0; s + pl <= vl; s++) {
        uint32_t k = 0;
        while (k < pl && v[s + k] == p[k]) k++;
        if (k == pl) return true;
    }
    return false;
}

// One argument slot of a resource: the request item an item rule reads and how
// its value is matched.  pat_len 0: a null or empty pattern (the value as is).
struct GwSlot {
    uint32_t field_id;
    int32_t parse, match;
    uint32_t pat_off, pat_len;           // in the pattern bytes of the loaded rules
};
// parseInternal + parseWithMatchStrategyInternal for a value that is present:
// true = the value itself, false = "$NM".  flags: val_flags of the request item
// (REGEX is evaluated by the caller, who owns GatewayRegexCache).
SF_HD bool gw_match(const GwSlot& s, const uint8_t* pat, const uint8_t* v, uint32_t vl, uint8_t flags) {
    if (s.pat_len == 0) return true;                                   // StringUtil.isEmpty(pattern)
    switch (s.match) {
        case GW_MATCH_EXACT: return gw_equal(v, vl, pat, s.pat_len);
        case GW_MATCH_CONTAINS: return gw_contains(v, vl, pat, s.pat_len);
        case GW_MATCH_REGEX: return !(flags & GW_NOMATCH);
        default: return true;                                          // PREFIX included (the reference's default:)
    }
}
// the (tag, bits) of one item slot; present false: the request has no such item
SF_HD void gw_parse(const GwSlot& s, const uint8_t* pat, bool present, const uint8_t* v, uint32_t vl, uint8_t flags,
                    uint8_t* tag, uint64_t* bits) {
    if (!present || s.parse < 0 || s.parse > 4) { *tag = GW_TAG_NULL; *bits = 0; return; }
    *tag = GW_TAG_STRING;
    *bits = gw_match(s, pat, v, vl, flags) ? gw_hash(v, vl) : GW_BITS_NM;
}

// GatewayRuleManager.isValidRule on the fields of sf_gateway_rule (the resource
// is an id: never blank).  pattern_empty: null or "".
SF_HD bool gw_valid_rule(int32_t resource_mode, int32_t grade, double count, int32_t burst, int32_t behavior,
                         int32_t max_queue_ms, int64_t interval_sec, bool has_item, int32_t parse, bool field_blank,
                         bool pattern_empty, int32_t match) {
    if (resource_mode < 0 || grade < 0 || count < 0 || burst < 0 || behavior < 0) return false;   // (NaN is not < 0)
    if (behavior == 2 && max_queue_ms < 0) return false;               // CONTROL_BEHAVIOR_RATE_LIMITER
    if (interval_sec <= 0) return false;
    if (!has_item) return true;
    if (parse < 0) return false;                                       // isValidParamItem
    if ((parse == 2 || parse == 3 || parse == 4) && field_blank) return false;   // FIELD_REQUIRED_SET
    return pattern_empty || match >= 0;
}

// The argument slots of one resource with gateway rules (sf_gateway_desc on the device).
struct GwDesc {
    uint32_t n_slots, n_item;            // n_slots > n_item: the last slot is "$D"
    int32_t gate;                        // GW_GATE_ANY, GW_GATE_NEVER, or the one resource mode of the item rules
    uint32_t pad;
    GwSlot slot[GW_MAX_SLOTS];
};
struct GwTables {                        // of: null = no gateway rule loaded
    const uint32_t* of;                  // [R] local resource -> index into desc, GW_NONE
    const GwDesc* desc;
    const uint8_t* pat;
    uint32_t R, shard_count, shard_index;
};
struct GwBatch {                         // device pointers (sf_gateway_batch staged or in place)
    uint32_t n, n_ent, n_val, n_str, n_exit, n_total;
    const int64_t* ts; const int32_t* count; const uint8_t* flags;
    const uint32_t* res_off; const uint32_t* res_id; const int32_t* res_mode;
    const uint32_t* val_off; const uint32_t* val_field; const uint32_t* val_str; const uint8_t* val_flags;
    const uint32_t* str_off; const uint8_t* bytes;
    const uint32_t* ev_index;
    const int64_t* entry_ref; const uint32_t* exit_pos;
};
struct GwOut {                           // the caller's event columns, stride n_total
    uint32_t* res_id; int64_t* ts; int32_t* count; uint8_t* flags; uint8_t* n_args; uint8_t* arg_tag; uint64_t* arg_bits;
};

// request of entry d: the i with res_off[i] <= d < res_off[i + 1] (n >= 1)
SF_HD uint32_t gw_req_of(const GwBatch& b, uint32_t d) {
    uint32_t lo = 0, hi = b.n - 1;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (b.res_off[mid + 1] <= d) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Entry d of a checked batch: its event columns and argument slots
// (parseParameterFor).  The kernel runs it one lane per entry; the host
// baseline of tools/gateway_bench.py in a loop.
SF_HD void gw_entry(const GwTables& t, const GwBatch& b, const GwOut& o, uint32_t d) {
    const uint32_t req = gw_req_of(b, d);
    const uint32_t pos = b.ev_index[req] + (d - b.res_off[req]);
    const uint32_t res = b.res_id[d];
    o.res_id[pos] = res;
    o.ts[pos] = b.ts[req];
    o.count[pos] = b.count[req];
    o.flags[pos] = b.flags[req] & GW_EV_KEEP;
    uint8_t tag[GW_MAX_SLOTS];
    uint64_t bits[GW_MAX_SLOTS];
SF_GW_UNROLL
    for (int a = 0; a < GW_MAX_SLOTS; a++) { tag[a] = GW_TAG_NULL; bits[a] = 0; }
    uint32_t n_args = 0;
    const uint32_t di = t.of ? t.of[res / t.shard_count] : GW_NONE;
    if (di != GW_NONE) {
        const GwDesc& g = t.desc[di];
        // predSet of parseParameterFor: every item rule must be of the entry's mode
        if (g.gate == GW_GATE_ANY || g.gate == b.res_mode[d]) {
            n_args = g.n_slots;
            const uint32_t v0 = b.val_off[req], v1 = b.val_off[req + 1];
SF_GW_UNROLL
            for (int a = 0; a < GW_MAX_SLOTS; a++) {
                if ((uint32_t)a >= g.n_item) break;
                const GwSlot s = g.slot[a];
                uint32_t v = v0;
                while (v < v1 && b.val_field[v] != s.field_id) v++;     // the first entry of a field is used
                const bool present = v < v1;
                const uint32_t si = present ? b.val_str[v] : 0;
                const uint32_t lo = present ? b.str_off[si] : 0, hi = present ? b.str_off[si + 1] : 0;
                gw_parse(s, t.pat + s.pat_off, present, b.bytes + lo, hi - lo, present && b.val_flags ? b.val_flags[v] : 0,
                         &tag[a], &bits[a]);
            }
            if (g.n_slots > g.n_item) {
SF_GW_UNROLL
                for (int a = 0; a < GW_MAX_SLOTS; a++)
                    if ((uint32_t)a == g.n_slots - 1) { tag[a] = GW_TAG_STRING; bits[a] = GW_BITS_D; }
            }
        }
    }
    o.n_args[pos] = (uint8_t)n_args;
SF_GW_UNROLL
    for (int a = 0; a < GW_MAX_SLOTS; a++) {
        o.arg_tag[(size_t)a * b.n_total + pos] = tag[a];
        o.arg_bits[(size_t)a * b.n_total + pos] = bits[a];
    }
}

}  // namespace sf

#ifndef SF_GATEWAY_HOST_ONLY
#include "../../include/sentinel_flow.h"

namespace sf {

// {res_off[n], val_off[n], str_off[n_str]} of a batch in device memory -> d_out[3]
hipError_t gw_lengths(const GwBatch& b, uint32_t* d_out, hipStream_t s);
// One sf_gateway_args on stream s.  own: [n_total] scratch.  The tables are
// checked first (*err = SF_ERR_INVALID and nothing is written); the call
// synchronises once, between the checks and the writes, and returns with the
// writes enqueued.  *err_host: the error word as read.
hipError_t gw_launch(const GwTables& t, const GwBatch& b, const GwOut& o, uint32_t* own, int32_t* err, int32_t* err_host,
                     hipStream_t s);

}  // namespace sf
#endif
