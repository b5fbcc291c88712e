// sf_authority.h — AuthorityRule black / white lists (product code; nothing
// here needs the HIP runtime, so tests/authority_check.cpp runs it on the host
// under the sanitizers).
//
// Reference (sentinel-core/.../slots/block/authority/):
//   AuthoritySlot.checkBlackWhiteAuthority   AuthoritySlot.java:51-70
//   AuthorityRuleChecker.passCheck           AuthorityRuleChecker.java:30-71
//   AuthorityRuleManager.loadAuthorityConf   AuthorityRuleManager.java:108-139
//   AuthorityRuleManager.isValidRule         AuthorityRuleManager.java:147-150
//
// The check reads (resource, origin, rules) and no statistics: an entry it
// blocks is exactly an SF_EV_BLOCKED entry (StatisticSlot.java:102-124), so the
// engine marks such entries once per batch, ahead of the sort (k_auth_mark,
// sf_authority.hip), and everything downstream treats them as pre-blocked.
//
// Strings stay with the caller: limitApp is split at "," (no trimming, as
// String.split does) and each piece interned with the interner of the event
// origins.  Tables, per engine (= shard):
//   of   [R]  rule slot of local row l = res / shard_count, AUTH_NONE: no rule
//   rule [k]  {strategy, off, cnt}
//   apps []   each rule's origin ids, sorted and de-duplicated
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/sentinel_flow.h"

#ifndef SF_HD
#if defined(__HIPCC__)
#define SF_HD __host__ __device__ __forceinline__
#else
#define SF_HD inline
#endif
#endif

namespace sf {

// Internal flag bit of the engine's effective-flags array: the entry was
// blocked by a loaded AuthorityRule (always together with SF_EV_BLOCKED; verdict
// SF_V_BLOCK_AUTHORITY).  Only the mark pass sets it; a caller's 0x20 / 0x40
// are stripped where that array is made and never read where it is not.
constexpr uint8_t EVF_AUTH = 0x20u;
constexpr uint8_t EVF_CALLER_STRIP = 0x60u;
constexpr uint32_t AUTH_NONE = 0xFFFFFFFFu;
// lists of at most this many ids are searched linearly, longer ones by bisection
constexpr uint32_t AUTH_LINEAR_MAX = 8;

struct AuthRule { int32_t strategy; uint32_t off, cnt; };
struct AuthTables {
    const uint32_t* of;            // [R], null: no rule loaded
    const AuthRule* rule;
    const uint32_t* apps;
    uint32_t R, shard_count, shard_index;
};

// origin in the sorted list a[0, cnt)
SF_HD bool auth_contains(const uint32_t* a, uint32_t cnt, uint32_t origin) {
    if (cnt <= AUTH_LINEAR_MAX) {
        bool hit = false;
        for (uint32_t k = 0; k < cnt; k++) hit |= a[k] == origin;
        return hit;
    }
    uint32_t lo = 0, hi = cnt;     // first element >= origin
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < origin) lo = mid + 1; else hi = mid;
    }
    return lo < cnt && a[lo] == origin;
}

// AuthorityRuleChecker.passCheck negated, for the one rule the manager keeps on
// the resource: the per-event predicate of the mark kernel and of the host
// check.  A resource outside this shard or its rows has no rule here.
// The predicate has two halves, so that the kernel can issue the gathers of
// several events before it waits for any: auth_slot is the rule slot the event
// has to be checked against (AUTH_NONE: it passes without a look at a rule),
// auth_rule_blocks the check against that rule's record.
SF_HD uint32_t auth_slot(const AuthTables& t, uint32_t res, uint32_t origin) {
    if (origin == SF_ORIGIN_NONE || !t.of) return AUTH_NONE;    // :33-35 an empty origin passes
    uint32_t l = res;
    if (t.shard_count != 1) {
        if (res % t.shard_count != t.shard_index) return AUTH_NONE;
        l = res / t.shard_count;
    }
    if (l >= t.R) return AUTH_NONE;
    return t.of[l];
}
SF_HD bool auth_rule_blocks(const AuthTables& t, const AuthRule& r, uint32_t origin) {
    if ((uint32_t)r.strategy > (uint32_t)SF_AUTHORITY_BLACK) return false;   // neither list kind: passes
    const bool contain = auth_contains(t.apps + r.off, r.cnt, origin);
    return r.strategy == SF_AUTHORITY_BLACK ? contain : !contain;            // :62-68
}
SF_HD bool auth_blocks(const AuthTables& t, uint32_t res, uint32_t origin) {
    const uint32_t k = auth_slot(t, res, origin);
    return k != AUTH_NONE && auth_rule_blocks(t, t.rule[k], origin);
}

// ---- host side: AuthorityRuleManager.loadAuthorityConf over interned ids
struct AuthHost {
    std::vector<uint32_t> of;      // empty when no rule was kept
    std::vector<AuthRule> rule;
    std::vector<uint32_t> apps;
    AuthTables view(uint32_t R, uint32_t shard_count, uint32_t shard_index) const {
        return AuthTables{of.empty() ? nullptr : of.data(), rule.data(), apps.data(), R, shard_count, shard_index};
    }
};

// Builds the tables of one shard.  Every rule's id range is checked before any
// id is read (SF_ERR_INVALID, `out` untouched).  isValidRule: a blank resource
// (SF_REF_NONE), strategy < 0 or a blank limitApp (app_cnt 0) is ignored; of
// the valid rules of one resource the first in list order is kept (:125-131,
// a later one does not replace it); rules of another shard are ignored.  A
// local resource beyond the shard's rows is SF_ERR_INVALID like the other loaders.
inline int auth_build(const sf_authority_rule* rules, uint32_t n, const uint32_t* apps, uint32_t n_apps, uint32_t R,
                      uint32_t shard_count, uint32_t shard_index, AuthHost& out) {
    for (uint32_t i = 0; i < n; i++)
        if (rules[i].app_cnt && (uint64_t)rules[i].app_off + rules[i].app_cnt > n_apps) return SF_ERR_INVALID;
    AuthHost h;
    for (uint32_t i = 0; i < n; i++) {
        const sf_authority_rule& r = rules[i];
        if (r.resource == SF_REF_NONE || r.strategy < 0 || r.app_cnt == 0) continue;
        if (r.resource % shard_count != shard_index) continue;
        const uint32_t l = r.resource / shard_count;
        if (l >= R) return SF_ERR_INVALID;
        if (h.of.empty()) h.of.assign(R, AUTH_NONE);
        if (h.of[l] != AUTH_NONE) continue;
        const uint32_t off = (uint32_t)h.apps.size();
        h.apps.insert(h.apps.end(), apps + r.app_off, apps + r.app_off + r.app_cnt);
        std::sort(h.apps.begin() + off, h.apps.end());
        h.apps.erase(std::unique(h.apps.begin() + off, h.apps.end()), h.apps.end());
        h.of[l] = (uint32_t)h.rule.size();
        h.rule.push_back(AuthRule{r.strategy, off, (uint32_t)h.apps.size() - off});
    }
    out = std::move(h);
    return SF_OK;
}

// the flag byte of the effective array: the caller's flags without the
// internal bits, plus the mark.  A caller-flagged SF_EV_BLOCKED entry stays
// the caller's (SF_V_BLOCK_OTHER); an EXIT is never marked.
SF_HD bool auth_markable(uint8_t f) { return !(f & (SF_EV_EXIT | SF_EV_BLOCKED)); }
SF_HD uint8_t auth_flag(const AuthTables& t, uint32_t res, uint32_t origin, uint8_t f, uint8_t mark) {
    f &= (uint8_t)~EVF_CALLER_STRIP;
    if (auth_markable(f) && auth_blocks(t, res, origin)) f |= mark;
    return f;
}

}  // namespace sf
