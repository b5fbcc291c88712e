// TEST-ONLY: the wide kinds of the per-window SystemRule exchange
// (sentinel_amd/csrc/sf_sysx.h: sxw_bin, sxw_range, sxw_reduce) on random small
// node streams, as a stand-alone program (ASan + UBSan, tests/
// test_system_exchange_wide.py), and, built with -DSXW_SHARED, as a small
// library that gives tests/sysx_wide_sim.py the product's plan step.
//
// The program draws a SysBase, a SystemRule of each kind and combinations, and
// 1..300 events -- entries (acquireCount 1..5), certain and uncertain exits --
// spread over 1..4 ranks, builds each rank's per-bin message (host_stats, the
// loop of k_sxw_stats) and runs sxw_reduce level by level, round by round.  It
// asserts, against sys_classify on the exact node-wide prefix of every entry:
//   - soundness: every entry of a settled run has exactly that outcome;
//   - every entry before q lies in a settled run, and q is the first entry
//     sys_classify calls unknown or lies before it;
//   - q > s_p;
//   - the ranks' messages in another order give the same plan.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <random>
#include <vector>

#include "../sentinel_amd/csrc/sf_sysx.h"

using namespace sf;

// one rank's events (local arrays, submission order) and how far it has decided
struct Rank {
    std::vector<int64_t> ts, eref, cts, seq;
    std::vector<int32_t> cnt;
    std::vector<uint8_t> flags, vstatus;
    uint32_t lp = 0;
};

static void put(int64_t* tab, int f, int64_t bin, int64_t v) {
    int64_t* p = tab + (size_t)f * SXW_B + bin;
    if (f == SXW_XC_MIN || f == SXW_XU_MIN || f == SXW_CMIN) *p = std::min(*p, v);
    else if (f == SXW_CMAX) *p = std::max(*p, v);
    else *p = wadd(*p, v);
}

// k_sxw_stats on the host: this rank's message of one level (no inert entries)
static void host_stats(const int64_t* ts, const int32_t* cnt, const uint8_t* flags, const int64_t* eref,
                       const int64_t* cts, const uint8_t* vstatus, const int64_t* seq, uint32_t n, uint32_t lp,
                       int64_t lo, int64_t hi, int64_t w, int64_t M, int64_t* msg) {
    for (int k = 0; k < SXW_F * SXW_B; k++) msg[SX_DELTA + k] = sxw_identity(k / SXW_B);
    for (uint32_t i = lp; i < n; i++) {
        if (seq[i] < lo || seq[i] >= hi) continue;
        const uint8_t f = flags[i];
        if (!(f & SF_EV_IN)) continue;
        const bool is_exit = (f & SF_EV_EXIT) != 0;
        if (!is_exit && (f & SF_EV_BLOCKED)) continue;
        const int64_t bin = (seq[i] - lo) / w;
        int64_t* tab = msg + SX_DELTA;
        const int32_t c = cnt[i];
        if (!is_exit) {
            put(tab, SXW_NE, bin, 1); put(tab, SXW_NB, bin, 1); put(tab, SXW_NB_C, bin, c > 0 ? c : 0);
            put(tab, SXW_CMIN, bin, c); put(tab, SXW_CMAX, bin, c);
            continue;
        }
        const SysExitQ q = sys_exit_q(ts, cnt, flags, eref, cts, vstatus, lp, i, M);
        if (q.xc) {
            put(tab, SXW_XC, bin, 1); put(tab, SXW_XC_C, bin, q.xc_c); put(tab, SXW_XC_RT, bin, q.xc_rt);
            put(tab, SXW_XC_MIN, bin, q.xc_min);
            bool bad = q.xc_c <= 0 || q.xc_rt < 0;
            if (M != INT64_MAX) {
                const __int128 d = (__int128)q.xc_rt - (__int128)M * q.xc_c, lim = (__int128)1 << 62;
                if (d >= lim || d <= -lim) bad = true;
                else if (d > 0) { put(tab, SXW_RP_LO, bin, (int64_t)d & 0xFFFFFFFFll); put(tab, SXW_RP_HI, bin, (int64_t)d >> 32); }
                else { put(tab, SXW_RN_LO, bin, (int64_t)(-d) & 0xFFFFFFFFll); put(tab, SXW_RN_HI, bin, (int64_t)(-d) >> 32); }
            }
            if (bad) put(tab, SXW_XBAD, bin, 1);
        } else if (q.xu) {
            put(tab, SXW_XU, bin, 1); put(tab, SXW_XU_C, bin, q.xu_c); put(tab, SXW_XU_BAD, bin, q.xu_bad);
            put(tab, SXW_XU_MIN, bin, q.xu_min);
            put(tab, SXW_XUP_LO, bin, q.xu_pos & 0xFFFFFFFFll); put(tab, SXW_XUP_HI, bin, q.xu_pos >> 32);
        }
    }
}

#ifdef SXW_SHARED
// ---- the plan step behind a C interface (tests/sysx_wide_sim.py)
struct SimRule { double qps, highest_load, highest_cpu, cur_load, cur_cpu; int64_t max_rt, max_thread; };
static SysRule sim_rule(const SimRule* x) {
    SysRule r{};
    r.check = 1;
    r.qps = x->qps;
    r.load_set = x->highest_load >= 0; r.highest_load = x->highest_load; r.cur_load = x->cur_load;
    r.cpu_set = x->highest_cpu >= 0; r.highest_cpu = x->highest_cpu; r.cur_cpu = x->cur_cpu;
    r.max_rt = x->max_rt; r.max_thread = x->max_thread;
    return r;
}
extern "C" {
int sxw_c_words() { return SXW_WORDS; }
int sxw_c_bins() { return SXW_B; }
int sxw_c_rule_ok(const SimRule* x) { return sx_rule_ok(sim_rule(x)) ? 1 : 0; }
void* sxw_c_plan_new() { return new SxwPlan(); }
void sxw_c_plan_free(void* p) { delete (SxwPlan*)p; }
void sxw_c_begin(void* p, int64_t lo, int64_t hi) { sxw_begin((SxwPlan*)p, lo, hi); }
// ENTRY_NODE's second buckets as rows of (window start, pass, succ, rt, minRt); WS_NONE: never used
void sxw_c_base(void* p, const int64_t* rows, int S, int wl, int interval, int64_t stat_max_rt, int64_t threads,
                int64_t t) {
    std::vector<Bucket> sec(S);
    for (int i = 0; i < S; i++) {
        sec[i] = fresh_bucket(rows[i * 5], stat_max_rt);
        sec[i].pass = rows[i * 5 + 1]; sec[i].succ = rows[i * 5 + 2]; sec[i].rt = rows[i * 5 + 3];
        sec[i].min_rt = rows[i * 5 + 4];
    }
    ((SxwPlan*)p)->base = sys_base(sec.data(), S, wl, interval, stat_max_rt, threads, t);
}
int64_t sxw_c_ws_none() { return WS_NONE; }
void sxw_c_stats(const int64_t* ts, const int32_t* cnt, const uint8_t* flags, const int64_t* eref, const int64_t* cts,
                 const uint8_t* vstatus, const int64_t* seq, uint32_t n, uint32_t lp, const void* p, int64_t max_rt,
                 int64_t* msg) {
    const SxwPlan* pl = (const SxwPlan*)p;
    for (int k = 0; k < SX_DELTA; k++) msg[k] = k == SXD_KEY ? -1 : 0;
    if (pl->done) { for (int k = 0; k < SXW_F * SXW_B; k++) msg[SX_DELTA + k] = sxw_identity(k / SXW_B); return; }
    host_stats(ts, cnt, flags, eref, cts, vstatus, seq, n, lp, pl->lo, pl->hi, pl->w, max_rt, msg);
}
// one level; segs: int64 triples (lo, hi, outcome), room for sxw_c_max_segs(); out: lo, hi, w, q, done, level, nseg, overflow
int sxw_c_max_segs() { return SXW_MAX_SEGS; }
void sxw_c_reduce(const int64_t* msgs, int N, void* p, int64_t* segs, const SimRule* x, int S, double interval_sec,
                  int64_t* out) {
    static_assert(sizeof(SxwSeg) == 24, "three words");
    SxwPlan* pl = (SxwPlan*)p;
    sxw_reduce(msgs, N, pl, (SxwSeg*)segs, sim_rule(x), S, interval_sec);
    out[0] = pl->lo; out[1] = pl->hi; out[2] = pl->w; out[3] = pl->q; out[4] = pl->done; out[5] = pl->level;
    out[6] = pl->nseg; out[7] = pl->overflow;
}
}
#else
// ---- the stand-alone program
static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (g_fail < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
    std::printf(__VA_ARGS__); std::printf("\n"); } g_fail++; } } while (0)

struct Ev { int rank; uint32_t li; };     // node stream, sequence order

static bool plan_eq(const SxwPlan& a, const SxwPlan& b) {
    return a.lo == b.lo && a.hi == b.hi && a.w == b.w && a.q == b.q && a.done == b.done && a.level == b.level &&
           a.nseg == b.nseg && a.overflow == b.overflow && !std::memcmp(&a.x, &b.x, sizeof a.x) &&
           a.e.nb == b.e.nb && a.e.nb_c == b.e.nb_c;
}

int main(int argc, char** argv) {
    const int trials = argc > 1 ? std::atoi(argv[1]) : 3000;
    std::mt19937_64 rng(20240611);
    auto ri = [&](int64_t a, int64_t b) { return a + (int64_t)(rng() % (uint64_t)(b - a + 1)); };   // [a, b]
    long rounds_total = 0, settled_pass = 0, settled_block[5] = {0, 0, 0, 0, 0}, deep = 0, unknown_q = 0, multi = 0;
    std::vector<SxwSeg> segs(SXW_MAX_SEGS), segs2(SXW_MAX_SEGS);
    for (int trial = 0; trial < trials; trial++) {
        const int N = (int)ri(1, 4), n = (int)ri(1, 300), S = (int)ri(1, 2);
        const double isec = S == 1 ? 1.5 : 1.0;
        // ---- the rule: each kind alone (trial % 6 < 4), then combinations
        SysRule r{};
        r.check = 1;
        r.qps = 1e300; r.max_rt = INT64_MAX; r.max_thread = INT64_MAX;
        const int kind = trial % 6;
        const bool k_qps = kind == 0 || (kind >= 4 && ri(0, 1)), k_thr = kind == 1 || (kind >= 4 && ri(0, 1));
        const bool k_rt = kind == 2 || (kind >= 4 && ri(0, 1)), k_load = kind == 3 || (kind >= 4 && ri(0, 2) == 0);
        SysBase base{};
        base.P = ri(0, 3000); base.T = ri(0, 60);
        base.SU = ri(0, 400); base.RT = base.SU * ri(3, 30) + ri(0, 50);
        base.cur_succ = ri(0, base.SU); base.other_max_succ = ri(0, 1) ? ri(0, 300) : 0;
        base.min_rt = ri(0, 3) ? ri(1, 40) : 5000;
        base.valid_other = base.other_max_succ ? 1 : 0;
        if (k_qps) r.qps = (double)(base.P + ri(-50, 700)) / isec + (ri(0, 1) ? 0.5 : 0.0);
        if (k_thr) r.max_thread = base.T + ri(-8, 60);
        if (k_rt) r.max_rt = ri(0, 9) ? ri(2, 32) : ri(0, 1);
        if (k_load) { r.load_set = 1; r.highest_load = 1.0; r.cur_load = ri(0, 5) ? 2.0 : 0.5; }
        if (kind == 5 && ri(0, 3) == 0) { r.cpu_set = 1; r.highest_cpu = 0.5; r.cur_cpu = ri(0, 1) ? 0.9 : 0.1; }
        // ---- the node stream
        std::vector<Rank> R(N);
        std::vector<Ev> stream;
        std::vector<std::vector<uint32_t>> open(N);              // local indices of entries not exited yet
        int64_t s = ri(0, 1000), t = ri(1000, 100000);
        const int p_exit = (int)ri(10, 60), p_cert = (int)ri(0, 100);
        for (int k = 0; k < n; k++) {
            const int rk = (int)ri(0, N - 1);
            Rank& a = R[rk];
            if (ri(0, 3) == 0) t += ri(0, 6);
            s += ri(0, 4) == 0 ? ri(2, 5) : 1;                   // gaps: bins without events
            const uint32_t li = (uint32_t)a.ts.size();
            uint8_t f = SF_EV_IN;
            int32_t c = (int32_t)ri(1, 5);
            int64_t er = -1, ct = 0;
            if (ri(0, 99) < p_exit) {
                f |= SF_EV_EXIT;
                if (ri(0, 99) < p_cert || open[rk].empty()) {    // its entry: an earlier batch (or blocked there)
                    er = ri(0, 19) == 0 ? EREF_DEAD : -1;
                    ct = t - ri(0, 60);
                } else {
                    const size_t j = (size_t)ri(0, (int64_t)open[rk].size() - 1);
                    er = open[rk][j];
                    open[rk].erase(open[rk].begin() + (long)j);
                    c = a.cnt[er];
                }
            } else if (ri(0, 29) == 0) {
                f |= SF_EV_BLOCKED;                              // blocked before SystemSlot
                if (ri(0, 1)) open[rk].push_back(li);            // (its exit counts as nothing)
            } else if (ri(0, 19) == 0) {
                f = 0;                                           // an OUT entry: not the node's business
            } else {
                open[rk].push_back(li);
            }
            a.ts.push_back(t); a.cnt.push_back(c); a.flags.push_back(f); a.eref.push_back(er); a.cts.push_back(ct);
            a.seq.push_back(s); a.vstatus.push_back(0);
            stream.push_back(Ev{rk, li});
        }
        const int64_t seq_end = s + 1;
        if (N > 1) multi++;
        // ---- rounds
        int64_t sp = R[stream[0].rank].seq[stream[0].li];
        size_t gp = 0;                                           // stream position of sp
        for (int round = 0; sp < seq_end; round++) {
            SxwPlan pl, pl2;
            sxw_begin(&pl, sp, seq_end);
            sxw_begin(&pl2, sp, seq_end);
            pl.base = pl2.base = base;
            std::vector<int64_t> msgs((size_t)N * SXW_WORDS, 0), msgs2((size_t)N * SXW_WORDS, 0);
            for (int level = 0; !pl.done; level++) {
                CHECK(level <= SXW_MAX_LEVELS, "trial %d: did not converge", trial);
                if (level > SXW_MAX_LEVELS) return 1;
                for (int k = 0; k < N; k++) {
                    const Rank& a = R[k];
                    host_stats(a.ts.data(), a.cnt.data(), a.flags.data(), a.eref.data(), a.cts.data(), a.vstatus.data(),
                               a.seq.data(), (uint32_t)a.ts.size(), a.lp, pl.lo, pl.hi, pl.w, r.max_rt,
                               &msgs[(size_t)k * SXW_WORDS]);
                    std::memcpy(&msgs2[(size_t)(N - 1 - k) * SXW_WORDS], &msgs[(size_t)k * SXW_WORDS], SXW_WORDS * 8);
                }
                sxw_reduce(msgs.data(), N, &pl, segs.data(), r, S, isec);
                sxw_reduce(msgs2.data(), N, &pl2, segs2.data(), r, S, isec);      // another rank order
                CHECK(plan_eq(pl, pl2), "trial %d round %d level %d: the plan depends on the rank order", trial, round, level);
                CHECK(!std::memcmp(segs.data(), segs2.data(), (size_t)pl.nseg * sizeof(SxwSeg)), "trial %d: runs differ", trial);
                if (level > 0) deep++;
            }
            CHECK(!pl.overflow, "trial %d: run list full", trial);
            CHECK(pl.q > sp && pl.q <= seq_end, "trial %d round %d: q %lld, s_p %lld", trial, round, (long long)pl.q, (long long)sp);
            if (!(pl.q > sp)) return 1;
            // ---- the exact prefix of every entry from s_p (sys_classify's own reading)
            SysExitQ X;
            SysEntQ E;
            X.clear(); E.clear();
            int64_t first_unknown = seq_end;
            size_t g = gp;
            int nseg_i = 0;
            for (; g < stream.size(); g++) {
                const Rank& a = R[stream[g].rank];
                const uint32_t i = stream[g].li;
                const int64_t sq = a.seq[i];
                const uint8_t f = a.flags[i];
                if ((f & SF_EV_IN) && !(f & (SF_EV_EXIT | SF_EV_BLOCKED))) {
                    bool fire = false;
                    const int res = sys_classify(r, base, S, isec, X, E, a.cnt[i], &fire);
                    if (res == -1 && first_unknown == seq_end) first_unknown = sq;
                    if (sq < pl.q) {
                        while (nseg_i < pl.nseg && segs[nseg_i].hi <= sq) nseg_i++;
                        const bool in = nseg_i < pl.nseg && segs[nseg_i].lo <= sq;
                        CHECK(in, "trial %d round %d: entry %lld before q %lld in no settled run", trial, round,
                              (long long)sq, (long long)pl.q);
                        const int64_t want = res >= 0 ? res : (res == -2 ? (int64_t)SYS_NONE : -1);
                        if (in) {
                            CHECK(segs[nseg_i].outcome == want, "trial %d round %d: entry %lld settled %lld, sys_classify %d",
                                  trial, round, (long long)sq, (long long)segs[nseg_i].outcome, res);
                            if (want == (int64_t)SYS_NONE) settled_pass++;
                            else if (want >= 0 && want < 5) settled_block[want]++;
                        }
                    }
                    if (!fire) { SysEntQ e1; e1.clear(); e1.nb = 1; e1.nb_c = a.cnt[i] > 0 ? a.cnt[i] : 0; E.add(e1); }
                }
                X.add(sys_exit_q(a.ts.data(), a.cnt.data(), a.flags.data(), a.eref.data(), a.cts.data(), a.vstatus.data(),
                                 a.lp, i, r.max_rt));
            }
            CHECK(pl.q <= first_unknown, "trial %d round %d: q %lld past the first unknown entry %lld", trial, round,
                  (long long)pl.q, (long long)first_unknown);
            if (pl.q < seq_end) unknown_q++;
            // ---- decide [s_p, q): settled blocks are blocked, the others pass or are blocked by a later slot
            nseg_i = 0;
            for (; gp < stream.size(); gp++) {
                Rank& a = R[stream[gp].rank];
                const uint32_t i = stream[gp].li;
                if (a.seq[i] >= pl.q) break;
                const uint8_t f = a.flags[i];
                uint8_t v = SF_V_PASS;
                if (!(f & SF_EV_EXIT)) {
                    if (f & SF_EV_BLOCKED) v = SF_V_BLOCK_OTHER;
                    else if (f & SF_EV_IN) {
                        while (nseg_i < pl.nseg && segs[nseg_i].hi <= a.seq[i]) nseg_i++;
                        if (nseg_i < pl.nseg && segs[nseg_i].outcome != (int64_t)SYS_NONE) v = SF_V_BLOCK_SYSTEM;
                        else if (ri(0, 3) == 0) v = SF_V_BLOCK_FLOW;
                    }
                }
                a.vstatus[i] = v;
                a.lp = i + 1;
            }
            sp = pl.q;
            rounds_total++;
            // ENTRY_NODE moved on: another base for the next round (soundness is per base)
            base.P += ri(0, 40); base.T = std::max<int64_t>(0, base.T + ri(-5, 5));
            const int64_t du = ri(0, 20);
            base.SU += du; base.RT += du * ri(0, 30); base.cur_succ += du;
        }
    }
    std::printf("rounds %ld, deeper levels %ld, rounds ending at an unknown entry %ld, trials with several ranks %ld\n",
                rounds_total, deep, unknown_q, multi);
    std::printf("settled entries: pass %ld, qps %ld, thread %ld, rt %ld, load %ld, cpu %ld\n", settled_pass,
                settled_block[0], settled_block[1], settled_block[2], settled_block[3], settled_block[4]);
    // the draws must reach every outcome and the refinement, or the run proves little
    CHECK(settled_pass > 1000 && settled_block[0] > 100 && settled_block[1] > 100 && settled_block[2] > 100 &&
          settled_block[3] > 100 && settled_block[4] > 0, "an outcome is never settled");
    CHECK(deep > 100 && unknown_q > 100 && multi > 100, "the refinement is never reached");
    std::printf("%d trials, %d failures\n", trials, g_fail);
    return g_fail ? 1 : 0;
}
#endif
