// TEST-ONLY stand-alone check of param_run_rule (sf_decide.h): the by-value
// form the wavefront walk of SM_PARAM segments runs, which the host build of
// the interpreter never reaches (tests/hostsim demotes SM_PARAM).
//
// For rule chains and occurrence lists of one value -- the border lists of
// tests/param_cases.py's families a to c, restated, and a few thousand seeded
// random ones -- it runs, on one table, heavy_param's order (rule by rule,
// param_run_rule over the live mask of each) and, on a second table, the
// reference's order (occurrence by occurrence, param_pass_single rule by rule
// until one blocks), and compares the surviving mask, the blocking rule, the
// waits (a blocked occurrence keeps what the rules before made it wait) and
// the final slot of every (rule, value).  Several groups follow each other on
// the same tables, so later groups start from stored state; the tables have 32
// slots and hold the neighbouring values (one half of the bits or the tag differs), so probes
// pass them and wrap.
//
//   param_run_check               run the checks; prints "... 0 failures"
//   param_run_check hash HI LO    prints ParamTable::hash(HI, LO) and
//                                 pkey_hi(0, PK_RULE, 0, 2) (drift test)
//
// Build: g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
// [-fsanitize=address,undefined]; has its own main, run directly.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../sentinel_amd/csrc/sf_decide.h"

using namespace sf;

namespace {

struct Occ { int64_t now; int32_t acq; };
struct Case {
    std::vector<DevParamRule> rules;
    std::vector<DevHotItem> items;
    uint32_t tag; uint64_t bits;
    std::vector<std::vector<Occ>> groups;        // consecutive 64-event groups (<= 64 occurrences each)
    uint64_t skip = 0;                           // occurrence bits never live (another value's lanes)
};

int failures = 0, checked = 0;

DevParamRule rule(int behavior, double count, int burst = 0, int64_t dur = 1, int queue = 0, int item_off = 0,
                  int item_cnt = 0) {
    DevParamRule r{};
    r.grade = SF_GRADE_QPS; r.param_idx = 0; r.behavior = behavior; r.max_queue_ms = queue; r.count = count;
    r.duration_sec = dur; r.burst = burst; r.item_off = item_off; r.item_cnt = item_cnt; r.host_index = 0;
    return r;
}
DevParamRule D(double count, int burst = 0, int64_t dur = 1, int io = 0, int ic = 0) {
    return rule(SF_BEHAVIOR_DEFAULT, count, burst, dur, 0, io, ic);
}
DevParamRule Th(double count, int queue, int64_t dur = 1, int io = 0, int ic = 0) {
    return rule(SF_BEHAVIOR_RATE_LIMITER, count, 0, dur, queue, io, ic);
}

struct Table {
    std::vector<ParamSlot> slots; int32_t err = 0;
    explicit Table(size_t n) : slots(n, ParamSlot{0, 0, 0, 0}) {}
    ParamTable pt() { ParamTable t{slots.data(), slots.size() - 1, &err}; return t; }
};

void fail(const char* name, const char* what, int g, int o, long long a, long long b) {
    if (failures < 20) std::printf("FAIL %s: %s group %d occurrence %d: run=%lld single=%lld\n", name, what, g, o, a, b);
    failures++;
}

void run_case(const char* name, const Case& c) {
    const uint32_t res = 3;
    Table ta(32), tb(32);
    // other keys around the value's home slots, so finds and inserts probe past them:
    // another resource's, and under each rule's own key the values that differ from
    // this one in the high half, the low half or the tag only (they must stay as they are)
    const int64_t SENT = -7777;
    const uint64_t near_bits[3] = {c.bits ^ (1ull << 32), c.bits ^ 1ull, c.bits};
    for (Table* t : {&ta, &tb}) {
        for (uint64_t x = 1; x <= 5; x++) t->pt().insert(pkey_hi(res + 1, PK_RULE, 0, c.tag), c.bits + x)->a = (int64_t)x;
        for (size_t k = 0; k < c.rules.size(); k++)
            for (int v = 0; v < 3; v++) {
                ParamSlot* s = t->pt().insert(pkey_hi(res, PK_RULE, (uint32_t)k, v == 2 ? c.tag + 1 : c.tag), near_bits[v]);
                s->a = SENT; s->b = SENT - v;
            }
    }
    const DevHotItem* items = c.items.empty() ? nullptr : c.items.data();
    for (size_t g = 0; g < c.groups.size(); g++) {
        const std::vector<Occ>& oc = c.groups[g];
        const int n = (int)oc.size();
        uint64_t mine = n == 64 ? ~0ull : ((1ull << n) - 1ull);
        mine &= ~c.skip;
        // heavy_param's order
        int64_t wait_a[64] = {0}; int rule_a[64]; uint64_t live = mine;
        for (int o = 0; o < 64; o++) rule_a[o] = -1;
        ParamTable pa = ta.pt();
        for (size_t k = 0; k < c.rules.size() && live; k++) {
            const uint64_t before = live;
            live = param_run_rule(pa, res, (int)k, c.rules[k], items, c.tag, c.bits, live,
                                  [&](int o) { return oc[o].now; }, [&](int o) { return oc[o].acq; },
                                  [&](int o, int64_t w) { wait_a[o] += w; });
            for (uint64_t m = before & ~live; m; m &= m - 1) rule_a[__builtin_ctzll(m)] = (int)k;
        }
        // the reference's order
        int64_t wait_b[64] = {0}; int rule_b[64]; uint64_t live_b = mine;
        ParamTable pb = tb.pt();
        for (int o = 0; o < n; o++) {
            rule_b[o] = -1;
            if (!((mine >> o) & 1)) continue;
            for (size_t k = 0; k < c.rules.size(); k++) {
                int64_t w = 0;
                const int ok = param_pass_single(pb, res, (int)k, c.rules[k], items, oc[o].now, oc[o].acq, c.tag, c.bits, &w);
                if (!ok) { rule_b[o] = (int)k; live_b &= ~(1ull << o); break; }
                if (w > 0) wait_b[o] += w;
            }
        }
        checked += n;
        if (live != live_b) fail(name, "live mask", (int)g, -1, (long long)live, (long long)live_b);
        for (int o = 0; o < n; o++) {
            if (wait_a[o] != wait_b[o]) fail(name, "wait", (int)g, o, wait_a[o], wait_b[o]);
            if (rule_a[o] != rule_b[o]) fail(name, "blocking rule", (int)g, o, rule_a[o], rule_b[o]);
        }
        for (size_t k = 0; k < c.rules.size(); k++) {
            const uint64_t hi = pkey_hi(res, PK_RULE, (uint32_t)k, c.tag);
            const ParamSlot* sa = ta.pt().find(hi, c.bits);
            const ParamSlot* sb = tb.pt().find(hi, c.bits);
            if (!sa != !sb) { fail(name, "slot present", (int)g, (int)k, sa != nullptr, sb != nullptr); continue; }
            if (sa && (sa->a != sb->a || sa->b != sb->b)) {
                fail(name, "slot a", (int)g, (int)k, sa->a, sb->a);
                fail(name, "slot b", (int)g, (int)k, sa->b, sb->b);
            }
        }
        if (ta.err || tb.err) fail(name, "table error", (int)g, -1, ta.err, tb.err);
    }
    for (Table* t : {&ta, &tb})
        for (size_t k = 0; k < c.rules.size(); k++)
            for (int v = 0; v < 3; v++) {
                const ParamSlot* s = t->pt().find(pkey_hi(res, PK_RULE, (uint32_t)k, v == 2 ? c.tag + 1 : c.tag), near_bits[v]);
                if (!s || s->a != SENT || s->b != SENT - v) fail(name, "neighbour value's slot", (int)k, v, s ? s->a : 0, SENT);
            }
}

const int64_t T0 = 1700000000000LL, WEEKS = 14LL * 24 * 3600 * 1000;

std::vector<Occ> at(std::initializer_list<Occ> l) {
    std::vector<Occ> v;
    for (const Occ& o : l) v.push_back(Occ{T0 + o.now, o.acq});
    return v;
}

void listed() {
    const uint32_t LONG_ = SF_TAG_LONG;
    auto C = [&](std::vector<DevParamRule> r, std::vector<std::vector<Occ>> g, std::vector<DevHotItem> it = {}) {
        Case c; c.rules = r; c.items = it; c.tag = LONG_; c.bits = 77; c.groups = g; return c;
    };
    // a. token bucket
    run_case("refill_d1", C({D(3)}, {at({{0, 1}, {0, 1}, {0, 1}, {1000, 1}, {1001, 1}})}));
    run_case("refill_d1_groups", C({D(3)}, {at({{0, 1}, {0, 1}, {0, 1}}), at({{1000, 1}}), at({{1001, 1}})}));
    run_case("refill_d3", C({D(3, 0, 3)}, {at({{0, 3}, {3000, 1}, {3001, 1}})}));
    run_case("toadd_d1", C({D(3, 1)}, {at({{0, 4}, {1333, 4}, {1334, 4}, {1334, 1}})}));
    run_case("toadd_d3", C({D(3, 1, 3)}, {at({{0, 4}, {3999, 4}, {4000, 4}, {4000, 1}})}));
    run_case("over_max", C({D(3, 1)}, {at({{0, 3}, {1334, 4}, {1334, 1}})}));
    run_case("acq_max", C({D(2, 3)}, {at({{0, 6}, {0, 5}, {0, 1}, {1001, 6}, {1001, 5}, {1001, 2}, {1001, 1}})}));
    run_case("acq_255", C({D(1, 0, 1, 0, 1)}, {at({{0, 255}, {0, 256}, {0, 256}, {0, 255}, {0, 256}, {0, 233}, {0, 1}})},
                          {DevHotItem{77, 1000, LONG_}}));
    for (double cnt : {0.5, 1.9, (double)NAN, -1.0, 1e19, 1099511627776.0})
        for (int burst : {0, 1, 2})
            run_case("counts", C({D(cnt, burst)}, {at({{0, 1}, {0, 1}, {0, 2}, {5, 2147483647}}),
                                                   at({{1500, 1}, {WEEKS, 1}, {WEEKS + 1, 3}, {2 * WEEKS, 1}})}));
    run_case("hot_zero", C({D(5, 0, 1, 0, 1)}, {at({{0, 1}, {1200, 1}})}, {DevHotItem{77, 0, LONG_}}));
    run_case("hot_negative", C({D(5, 3, 1, 0, 1)}, {at({{0, 1}, {0, 1}, {0, 2}})}, {DevHotItem{77, -2, LONG_}}));
    run_case("hot_other_tag", C({D(2, 0, 1, 0, 1)}, {at({{0, 1}, {0, 1}, {0, 1}})}, {DevHotItem{77, 0, SF_TAG_INT}}));
    run_case("hot_first_wins", C({D(9, 0, 1, 0, 2)}, {at({{0, 1}, {0, 1}})},
                                 {DevHotItem{77, 1, LONG_}, DevHotItem{77, 5, LONG_}}));
    run_case("hot_high_half", C({D(9, 0, 1, 0, 2)}, {at({{0, 1}, {0, 1}})},
                                {DevHotItem{77 | 1ull << 32, 0, LONG_}, DevHotItem{77, 1, LONG_}}));
    // b. throttle
    {
        std::vector<Occ> v(15, Occ{T0, 1});
        v[13].now = v[14].now = T0 + 1;
        run_case("half_cost", C({Th(2000, 10)}, {v}));
    }
    run_case("cost_333", C({Th(3, 500)}, {at({{0, 1}, {0, 1}, {0, 1}, {167, 1}, {167, 1}})}));
    run_case("cost_0", C({Th(1e15, 5)}, {at({{0, 1}, {0, 1}, {0, 1}, {3, 255}})}));
    run_case("queue_0", C({Th(10, 0)}, {at({{0, 1}, {50, 1}, {99, 1}, {100, 1}, {100, 1}})}));
    run_case("throttle_hot_negative", C({Th(10, 0, 1, 0, 1)}, {at({{0, 1}, {0, 1}, {0, 1}, {7, 3}})},
                                        {DevHotItem{77, -5, LONG_}}));
    run_case("two_throttles", C({Th(10, 500), Th(5, 500)}, {at({{0, 1}, {0, 1}, {0, 1}, {0, 1}, {50, 1}, {150, 1}})}));
    for (int order = 0; order < 2; order++) {
        std::vector<Occ> v;
        for (int k = 0; k < 40; k++) v.push_back(Occ{T0 + k / 8, 1});
        run_case(order ? "default_first" : "throttle_first",
                 order ? C({D(2), Th(10, 500)}, {v}) : C({Th(10, 500), D(2)}, {v}));
    }
    run_case("three_rules", C({D(4), Th(50, 30), D(2, 1, 1, 0, 1)},
                              {at({{0, 1}, {0, 2}, {3, 1}, {40, 2}, {900, 1}}), at({{1001, 1}, {1001, 2}, {1500, 1}})},
                              {DevHotItem{77, 6, LONG_}}));
    // c. value identity: bits 0 and ~0, high and low halves, other lanes' occurrences skipped
    for (uint64_t bits : {0ull, ~0ull, 5ull, 5ull | 1ull << 32, 5ull | 1ull << 63}) {
        Case c = C({D(2)}, {at({{0, 1}, {0, 1}, {0, 1}, {1, 1}, {2, 1}, {2, 1}})});
        c.bits = bits; c.skip = 0x12;
        c.items = {DevHotItem{bits ^ (1ull << 32), 0, LONG_}, DevHotItem{bits ^ 1ull, 0, LONG_}};
        c.rules[0].item_cnt = 2;
        run_case("identity", c);
    }
}

uint64_t rng_state = 0x243F6A8885A308D3ull;
uint64_t rnd() { rng_state += 0x9e3779b97f4a7c15ULL; return mix64(rng_state); }
template <class T, size_t N> T pick(const T (&a)[N]) { return a[rnd() % N]; }

void random_cases(int n_cases) {
    const double counts[] = {0.5, 1, 1.9, 2, 3, 5, 10, 50, 2000, 1e15, 1e19, 1099511627776.0, (double)NAN, -1};
    const int bursts[] = {0, 0, 1, 3}, queues[] = {0, 10, 30, 500};
    const int64_t durs[] = {1, 1, 3}, gaps[] = {0, 0, 0, 0, 1, 1, 7, 333, 999, 1000, 1001, 2999, 3000, 3001, WEEKS};
    const int32_t acqs[] = {1, 1, 1, 1, 2, 3, 4, 5, 255, 256, 2147483647};
    const int32_t hots[] = {0, -2, -5, 1, 6, 1000};
    for (int i = 0; i < n_cases; i++) {
        Case c; c.tag = SF_TAG_LONG; c.bits = rnd() % 3 ? rnd() : (rnd() & 3) * 0x100000001ull;
        const int nr = 1 + (int)(rnd() % 3);
        for (int k = 0; k < nr; k++) {
            const int io = (int)c.items.size(), ic = (int)(rnd() % 3);
            for (int j = 0; j < ic; j++) {
                const uint64_t b = rnd() % 2 ? c.bits : c.bits ^ (1ull << (rnd() % 64));
                c.items.push_back(DevHotItem{b, pick(hots), rnd() % 4 ? c.tag : (uint32_t)SF_TAG_INT});
            }
            c.rules.push_back(rnd() % 3 ? D(pick(counts), pick(bursts), pick(durs), io, ic)
                                        : Th(pick(counts), pick(queues), pick(durs), io, ic));
        }
        int64_t now = T0;
        const int ng = 1 + (int)(rnd() % 3);
        for (int g = 0; g < ng; g++) {
            const int lens[] = {1, 2, 5, 17, 63, 64};
            std::vector<Occ> v(pick(lens));
            for (Occ& o : v) { now += pick(gaps); o = Occ{now, pick(acqs)}; }
            c.groups.push_back(v);
        }
        c.skip = rnd() % 4 ? 0 : rnd();
        run_case("random", c);
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && !std::strcmp(argv[1], "hash")) {
        const uint64_t hi = std::strtoull(argv[2], nullptr, 0), lo = std::strtoull(argv[3], nullptr, 0);
        std::printf("%" PRIu64 " %" PRIu64 "\n", ParamTable::hash(hi, lo), pkey_hi(0, PK_RULE, 0, SF_TAG_LONG));
        return 0;
    }
    listed();
    random_cases(4000);
    std::printf("param_run_check: %d occurrences checked, %d failures\n", checked, failures);
    return failures ? 1 : 0;
}
