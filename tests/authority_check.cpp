// TEST-ONLY stand-alone host program: the AuthorityRule tables
// (sentinel_amd/csrc/sf_authority.h).  The table builder the engine's loader
// runs and the per-event predicate the mark kernel runs are driven here over
// cases that tests/test_authority_model.py writes from the string model
// (tests/authority_model.py):
//
//   case <name>
//   cfg <R> <shard_count> <shard_index>
//   apps <n_apps> id ...
//   rules <n> then n x: <resource> <strategy> <app_off> <app_cnt>
//   expect <rc of auth_build> <rules kept>
//   pairs <m> then m x: <resource> <origin> <blocks 0/1>
//
// Every array is a heap block of exactly its stated length, so the address
// sanitizer this is built with sees any access outside it -- in particular a
// malformed app range must be refused before anything is read.  Each pair is
// also put through auth_flag with the flag bytes whose handling the mark pass
// promises (an exit, a caller-flagged entry, the reserved bits).
// Exit status 0: every case as expected.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "../sentinel_amd/csrc/sf_authority.h"

using namespace sf;

static long bad = 0;
static void fail(const std::string& what) {
    if (bad++ < 20) std::printf("FAIL %s\n", what.c_str());
}

template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {          // a block of exactly v.size() elements
    std::unique_ptr<T[]> p(new T[v.size()]);
    for (size_t i = 0; i < v.size(); i++) p[i] = v[i];
    return p;
}

int main(int argc, char** argv) {
    if (argc != 2) { std::printf("usage: authority_check <cases>\n"); return 2; }
    std::ifstream in(argv[1]);
    std::string word, name;
    long cases = 0, pairs_checked = 0;
    while (in >> word) {
        if (word != "case") { std::printf("bad case file at '%s'\n", word.c_str()); return 2; }
        in >> name;
        uint32_t R, sc, si, n_apps, n, m, kept;
        int rc_want;
        in >> word >> R >> sc >> si;
        in >> word >> n_apps;
        std::vector<uint32_t> apps(n_apps);
        for (auto& x : apps) in >> x;
        in >> word >> n;
        std::vector<sf_authority_rule> rules(n);
        for (auto& r : rules) in >> r.resource >> r.strategy >> r.app_off >> r.app_cnt;
        in >> word >> rc_want >> kept;
        in >> word >> m;
        std::vector<uint32_t> pr(m), po(m), pb(m);
        for (uint32_t k = 0; k < m; k++) in >> pr[k] >> po[k] >> pb[k];
        if (!in) { std::printf("truncated case %s\n", name.c_str()); return 2; }
        cases++;

        const auto h_apps = exact(apps);
        const auto h_rules = exact(rules);
        AuthHost host;
        host.rule.push_back(AuthRule{77, 0, 0});                        // must survive a refused build
        const int rc = auth_build(h_rules.get(), n, h_apps.get(), n_apps, R, sc, si, host);
        if (rc != rc_want) { fail(name + ": auth_build returned " + std::to_string(rc)); continue; }
        if (rc != SF_OK) {
            if (host.rule.size() != 1 || host.rule[0].strategy != 77) fail(name + ": a refused build changed the tables");
            continue;
        }
        if (host.rule.size() != kept) fail(name + ": kept " + std::to_string(host.rule.size()) + " rules");
        if (host.rule.empty() != host.of.empty()) fail(name + ": auth_of allocated without a rule");
        for (const AuthRule& r : host.rule) {                           // sorted, de-duplicated, inside apps
            if ((size_t)r.off + r.cnt > host.apps.size() || r.cnt == 0) { fail(name + ": rule range"); break; }
            for (uint32_t k = 1; k < r.cnt; k++)
                if (host.apps[r.off + k - 1] >= host.apps[r.off + k]) { fail(name + ": list not sorted / unique"); break; }
        }
        // the kernel's view: exact-length copies of the three tables
        const auto d_of = exact(host.of);
        const auto d_rule = exact(host.rule);
        const auto d_apps = exact(host.apps);
        const AuthTables t{host.of.empty() ? nullptr : d_of.get(), d_rule.get(), d_apps.get(), R, sc, si};
        const uint8_t IN = SF_EV_IN, MARK = SF_EV_BLOCKED | EVF_AUTH;
        for (uint32_t k = 0; k < m; k++) {
            pairs_checked++;
            const bool got = auth_blocks(t, pr[k], po[k]);
            if (got != (pb[k] != 0)) {
                fail(name + ": (" + std::to_string(pr[k]) + ", " + std::to_string(po[k]) + ") blocks=" + std::to_string(got));
                continue;
            }
            const uint8_t want = got ? (uint8_t)(IN | MARK) : IN;
            if (auth_flag(t, pr[k], po[k], IN, MARK) != want) fail(name + ": entry flag");
            if (auth_flag(t, pr[k], po[k], IN | SF_EV_EXIT, MARK) != (IN | SF_EV_EXIT)) fail(name + ": an exit was marked");
            if (auth_flag(t, pr[k], po[k], IN | SF_EV_BLOCKED, MARK) != (IN | SF_EV_BLOCKED))
                fail(name + ": a caller-flagged entry was marked");
            if (auth_flag(t, pr[k], po[k], IN | 0x60, MARK) != want) fail(name + ": reserved bits not stripped");
            if (auth_flag(t, pr[k], po[k], IN | SF_EV_BLOCKED | 0x20, MARK) != (IN | SF_EV_BLOCKED))
                fail(name + ": a caller's 0x20 survived");
        }
    }
    std::printf("%ld cases, %ld pairs, %ld failures\n", cases, pairs_checked, bad);
    return bad ? 1 : 0;
}
