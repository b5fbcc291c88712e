// TEST-ONLY stand-alone host program: the memory ownership types of the engine
// (sentinel_amd/csrc/sf_mem.h) and the work-set growth functions built on them
// (sf_worksets.h), on a malloc backend that can fail the k-th allocation.
//   - DevPool: every allocation is freed exactly once, by release or by the
//     destructor; a pointer released twice or never seen is reported, not freed;
//   - GrowBuf: reallocates only when it must, and is empty after a failure;
//   - the work sets (TokWork, CcWork, DegradeWork): with any one allocation of
//     a growth step failing, the set reads capacity 0, every pointer null and
//     nothing leaked, and the retry builds the whole set;
//   - Layout: its own offsets;
//   - StagePlan: the rooms of the token request staging and of the host batch
//     staging lie where the align_up chains the engine computed by hand put
//     them, inside size(), apart, aligned and in declaration order; upload and
//     download copy exactly the declared bytes of the pieces that asked, in
//     order, and stop at a failing copy; device-form pieces are the caller's
//     pointers with no room and no copy; a piece that is off is null.
// Built with the address and undefined-behaviour sanitizers: a double free, a
// leak at exit or an access outside a block ends the run.  Exit status 0 and
// " 0 failures": every case as expected.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "../sentinel_amd/csrc/sf_worksets.h"

using namespace sf;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) { failures++; std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

// ---------------------------------------------------------------- the backend
static long n_alloc = 0, n_free = 0, fail_in = 0;   // fail_in = k: the k-th allocation from now fails
static std::set<void*> live_dev, live_host;
static const int NOMEM = -3;

static int t_alloc(std::set<void*>& live, void** p, size_t bytes) {
    if (fail_in && --fail_in == 0) { *p = (void*)0x1; return NOMEM; }   // (a failing backend may leave garbage)
    *p = std::malloc(bytes);
    n_alloc++;
    live.insert(*p);
    return 0;
}
static void t_free(std::set<void*>& live, void* p) {
    CHECK(live.erase(p) == 1);                       // freed once, by the kind that allocated it
    n_free++;
    std::free(p);
}
static const MemOps MEM{[](void** p, size_t b) { return t_alloc(live_dev, p, b); }, [](void* p) { t_free(live_dev, p); },
                        [](void** p, size_t b) { return t_alloc(live_host, p, b); }, [](void* p) { t_free(live_host, p); }};
static size_t live() { return live_dev.size() + live_host.size(); }

// ---------------------------------------------------------------- DevPool
static void pool_cases() {
    const long a0 = n_alloc, f0 = n_free;
    void* foreign = std::malloc(8);
    {
        DevPool pool(MEM);
        char* p[20];
        for (int i = 0; i < 20; i++) CHECK((i % 3 ? pool.alloc(&p[i], 1 + i) : pool.alloc_host(&p[i], 1 + i)) == 0);
        CHECK(pool.count() == 20 && n_alloc - a0 == 20);
        char* again = p[10];
        CHECK(pool.release(p[0]) && !p[0]);
        CHECK(pool.release(p[10]) && !p[10]);
        CHECK(pool.release(p[19]) && !p[19]);
        CHECK(n_free - f0 == 3 && pool.count() == 17);
        CHECK(!pool.release(again) && again);        // released before: reported, not freed again
        void* f = foreign;
        CHECK(!pool.release(f) && f == foreign);     // never seen
        CHECK(n_free - f0 == 3);
        CHECK(pool.release(p[0]));                   // (a null pointer: nothing to do)
        int* q = nullptr;
        fail_in = 1;
        CHECK(pool.alloc(&q, 64) == NOMEM && !q && pool.count() == 17);
    }
    CHECK(n_free - f0 == n_alloc - a0 && n_alloc - a0 == 20 && live() == 0);
    std::free(foreign);
}

// ---------------------------------------------------------------- GrowBuf
static void growbuf_cases() {
    DevPool pool(MEM);
    GrowBuf g;
    const size_t sizes[] = {0, 1, 256, 100, 257};
    const bool grows[] = {false, true, true, false, true};
    size_t cap = 0;
    for (int i = 0; i < 5; i++) {
        const long a = n_alloc;
        CHECK(g.reserve(pool, sizes[i]) == 0);
        CHECK((n_alloc - a == 1) == grows[i]);
        if (grows[i]) cap = sizes[i];                // exactly what was asked for
        CHECK(g.bytes == cap && (g.p != nullptr) == (cap != 0) && pool.count() == (cap ? 1u : 0u));
    }
    fail_in = 1;
    CHECK(g.reserve(pool, 1000) == NOMEM);
    CHECK(!g.p && g.bytes == 0 && pool.count() == 0 && live() == 0);
    CHECK(g.reserve(pool, 1000) == 0 && g.p && g.bytes == 1000);
    ((char*)g.p)[999] = 1;
}

// ---------------------------------------------------------------- the work sets
static int tok_query(uint32_t n, size_t* a, size_t* b, size_t* c) { *a = n; *b = 8 * (size_t)n; *c = 0; return 0; }
static int cc_query(uint32_t n, size_t* a) { *a = 4 * (size_t)n; return 0; }
static int dg_query(uint32_t n, uint32_t kb, size_t* a) { *a = (size_t)n * kb; return 0; }
static int bad_query3(uint32_t, size_t*, size_t*, size_t*) { return -2; }

static int tok_ptrs(const TokWork& w) {
    const void* p[] = {w.nskey_in, w.nskey_out, w.idx_in, w.idx_out, w.key_in, w.key_out, w.rule_of, w.pending,
                       w.head, w.head_scan, w.seg_start, w.n_seg, w.sort8_tmp, w.sort64_tmp, w.scan_tmp};
    int k = 0;
    for (const void* x : p) k += x != nullptr;
    return k;
}
static int cc_ptrs(const CcWork& w) {
    const void* p[] = {w.key_in, w.key_out, w.idx_in, w.idx_out, w.delta, w.rslot, w.seg_lo, w.seg_hi, w.sort_tmp};
    int k = 0;
    for (const void* x : p) k += x != nullptr;
    return k;
}
static int dg_ptrs(const DegradeWork& w) {
    const void* p[] = {w.keys_in, w.keys_out, w.idx_in, w.idx_out, w.beg, w.end, w.sort_tmp, w.err, w.heavy, w.n_heavy,
                       w.sev, w.inv};
    int k = 0;
    for (const void* x : p) k += x != nullptr;
    return k;
}

static void tok_cases() {
    {   // how many allocations a growth step makes
        TokWorkSet s(MEM);
        const long a = n_alloc;
        CHECK(tok_work_ensure(s, 100, 64, tok_query) == 0 && n_alloc - a == 15 && s.cap == 100 && tok_ptrs(s.w) == 15);
        CHECK(tok_work_ensure(s, 100, 64, tok_query) == 0 && tok_work_ensure(s, 3, 64, tok_query) == 0 && n_alloc - a == 15);
        CHECK(tok_work_ensure(s, 200, 64, tok_query) == 0 && n_alloc - a == 30 && s.cap == 200 && s.pool.count() == 15);
        CHECK(s.w.sort64_bytes == 1600);
    }
    CHECK(live() == 0);
    for (int k = 1; k <= 15; k++) {
        TokWorkSet s(MEM);
        CHECK(tok_work_ensure(s, 100, 64, tok_query) == 0);      // a populated set
        fail_in = k;
        CHECK(tok_work_ensure(s, 200, 64, tok_query) == NOMEM);
        CHECK(fail_in == 0);                                      // (the k-th allocation was reached)
        CHECK(s.cap == 0 && tok_ptrs(s.w) == 0 && s.pool.count() == 0 && live() == 0);
        CHECK(tok_work_ensure(s, 50, 64, tok_query) == 0);       // (a stale capacity of 100 would let this through on null buffers)
        CHECK(s.cap == 64 && tok_ptrs(s.w) == 15 && s.pool.count() == 15);
        CHECK(tok_work_ensure(s, 200, 64, tok_query) == 0 && s.cap == 200 && tok_ptrs(s.w) == 15);
    }
    {
        TokWorkSet s(MEM);
        CHECK(tok_work_ensure(s, 100, 64, bad_query3) == -2 && s.cap == 0 && tok_ptrs(s.w) == 0 && live() == 0);
    }
    CHECK(live() == 0);
}

static void cc_cases() {
    for (int k = 1; k <= 9; k++) {
        CcWorkSet s(MEM);
        const long a = n_alloc;
        CHECK(cc_work_ensure(s, 100, 5, cc_query) == 0 && n_alloc - a == 9 && s.w.cap == 100 && s.w.nf_cap == 5);
        fail_in = k;
        CHECK(cc_work_ensure(s, 300, 2, cc_query) == NOMEM && fail_in == 0);
        CHECK(s.w.cap == 0 && s.w.nf_cap == 0 && cc_ptrs(s.w) == 0 && s.pool.count() == 0 && live() == 0);
        CHECK(cc_work_ensure(s, 3, 2, cc_query) == 0 && s.w.cap == 3 && s.w.nf_cap == 2 && cc_ptrs(s.w) == 9);
        CHECK(cc_work_ensure(s, 3, 9, cc_query) == 0 && s.w.cap == 3 && s.w.nf_cap == 9 && s.pool.count() == 9);
    }
    CHECK(live() == 0);
}

static void dg_cases() {
    for (int k = 1; k <= 12; k++) {                  // from nothing: 6 + scratch + 3 + err + n_heavy
        DegradeWorkSet s(MEM);
        const long a = n_alloc;
        fail_in = k;
        CHECK(dg_work_ensure(s, 10, 3, 2, dg_query) == NOMEM && fail_in == 0 && n_alloc - a == k - 1);
        CHECK(s.w.cap == 0 && s.w.beg_cap == 0 && s.w.sort_tmp_bytes == 0 && dg_ptrs(s.w) == 0 && live() == 0);
        CHECK(dg_work_ensure(s, 10, 3, 2, dg_query) == 0 && dg_ptrs(s.w) == 12 && s.w.cap == 10 && s.w.beg_cap == 3);
    }
    for (int k = 1; k <= 10; k++) {                  // from a populated set: 6 + scratch + 3
        DegradeWorkSet s(MEM);
        CHECK(dg_work_ensure(s, 10, 3, 2, dg_query) == 0 && s.w.sort_tmp_bytes == 20);
        const long a = n_alloc;
        fail_in = k;
        CHECK(dg_work_ensure(s, 50, 7, 2, dg_query) == NOMEM && fail_in == 0 && n_alloc - a == k - 1);
        CHECK(s.w.cap == 0 && s.w.beg_cap == 0 && dg_ptrs(s.w) == 0 && s.pool.count() == 0 && live() == 0);
        CHECK(dg_work_ensure(s, 5, 1, 2, dg_query) == 0);          // (a stale capacity of 10 would let this through on null buffers)
        CHECK(dg_ptrs(s.w) == 12 && s.w.cap == 5 && s.w.beg_cap == 1 && s.pool.count() == 12);
    }
    {   // no growth: nothing is allocated; a new key width: only the scratch
        DegradeWorkSet s(MEM);
        CHECK(dg_work_ensure(s, 10, 3, 2, dg_query) == 0);
        const long a = n_alloc;
        CHECK(dg_work_ensure(s, 3, 2, 2, dg_query) == 0 && n_alloc - a == 0);
        dg_drop_sort_tmp(s);
        CHECK(dg_work_ensure(s, 3, 2, 5, dg_query) == 0 && n_alloc - a == 1 && s.w.sort_tmp_bytes == 50 && s.pool.count() == 12);
    }
    CHECK(live() == 0);
}

// ---------------------------------------------------------------- Layout
static size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// ---------------------------------------------------------------- StagePlan
// One declared piece and what the checks know about it.
struct Decl { int kind; bool on; size_t bytes, room; bool copy_back; };   // kind: 0 in, 1 out, 2 scratch
static Decl d_in(bool on, size_t bytes, size_t room = 0) { return Decl{0, on, bytes, room ? room : bytes, false}; }
static Decl d_out(bool on, size_t bytes, bool copy_back = true) { return Decl{1, on, bytes, bytes, copy_back}; }
static Decl d_scratch(bool on, size_t bytes) { return Decl{2, on, bytes, bytes, false}; }

static const int COPY_ERR = -7;
struct CopyLog {
    struct Rec { void* dst; const void* src; size_t bytes; };
    std::vector<Rec> recs;
    long fail_at = 0;                                  // k: the k-th call fails (after k - 1 copies)
    int operator()(void* dst, const void* src, size_t bytes) {
        if (fail_at && (long)recs.size() + 1 == fail_at) { recs.push_back(Rec{nullptr, nullptr, 0}); return COPY_ERR; }
        std::memcpy(dst, src, bytes);
        recs.push_back(Rec{dst, src, bytes});
        return 0;
    }
};

// The pieces `d` declared on one plan in the given forms; want: the offsets of
// the hand-written chain for the staged pieces (SIZE_MAX: not checked), want_size its end.
static void plan_check(const std::vector<Decl>& d, bool host_in, bool host_out, const std::vector<size_t>* want = nullptr,
                       size_t want_size = 0) {
    const size_t N = d.size();
    std::vector<std::vector<unsigned char>> host(N);
    std::vector<const unsigned char*> ip(N, (const unsigned char*)0x10);
    std::vector<unsigned char*> op(N, (unsigned char*)0x10);
    StagePlan plan(host_in, host_out);
    size_t scratch_room = 0;
    for (size_t i = 0; i < N; i++) {
        host[i].assign(d[i].bytes + 1, 0);             // (+1: an address of its own even when empty)
        for (size_t j = 0; j < d[i].bytes; j++) host[i][j] = (unsigned char)(i * 37 + j * 11 + 1);
        if (d[i].kind == 0) plan.in(d[i].on, &ip[i], host[i].data(), d[i].bytes, d[i].room == d[i].bytes ? 0 : d[i].room);
        else if (d[i].kind == 1) plan.out(d[i].on, &op[i], host[i].data(), d[i].bytes, d[i].copy_back);
        else plan.scratch(d[i].on, &op[i], d[i].bytes);
        if (d[i].kind == 2 && d[i].on) scratch_room += align_up(d[i].room);
    }
    auto staged = [&](size_t i) { return d[i].on && (d[i].kind == 2 || (d[i].kind == 0 ? host_in : host_out)); };
    auto ptr = [&](size_t i) { return d[i].kind == 0 ? ip[i] : (const unsigned char*)op[i]; };
    if (!host_in && !host_out) CHECK(plan.size() == scratch_room);
    if (want) CHECK(plan.size() == want_size);
    // the buffer: a failing allocation leaves it empty, the retry succeeds
    DevPool pool(MEM);
    GrowBuf buf;
    if (plan.size()) {
        fail_in = 1;
        CHECK(buf.reserve(pool, plan.size()) == NOMEM && !buf.p && buf.bytes == 0 && pool.count() == 0);
    }
    CHECK(buf.reserve(pool, plan.size()) == 0 && buf.bytes == plan.size());
    plan.bind(buf.p);
    const unsigned char* base = (const unsigned char*)buf.p;
    size_t end = 0;                                     // the end of the room before
    for (size_t i = 0; i < N; i++) {
        if (!d[i].on) { CHECK(ptr(i) == nullptr); continue; }
        if (!staged(i)) { CHECK(ptr(i) == host[i].data()); continue; }    // device form: the caller's pointer
        const size_t off = (size_t)(ptr(i) - base);
        CHECK(off % 256 == 0 && off >= end && off + d[i].room <= plan.size());
        CHECK(off == end);                              // declaration order, nothing between the rooms
        if (want && (*want)[i] != SIZE_MAX) CHECK(off == (*want)[i]);
        end = off + align_up(d[i].room);
    }
    CHECK(end == plan.size());
    // upload: exactly `bytes` of every staged input with bytes, in order
    CopyLog up;
    CHECK(plan.upload(up) == 0);
    size_t k = 0;
    for (size_t i = 0; i < N; i++) {
        if (!(staged(i) && d[i].kind == 0 && d[i].bytes)) continue;
        CHECK(k < up.recs.size());
        if (k >= up.recs.size()) break;
        CHECK(up.recs[k].dst == ptr(i) && up.recs[k].src == host[i].data() && up.recs[k].bytes == d[i].bytes);
        CHECK(std::memcmp(ptr(i), host[i].data(), d[i].bytes) == 0);
        k++;
    }
    CHECK(k == up.recs.size());
    // the "kernels" write every result; download brings back the pieces that asked
    for (size_t i = 0; i < N; i++)
        if (staged(i) && d[i].kind == 1 && d[i].bytes) std::memset(op[i], 0xA0 + (int)i, d[i].bytes);
    CopyLog down;
    CHECK(plan.download(down) == 0);
    k = 0;
    for (size_t i = 0; i < N; i++) {
        if (!(staged(i) && d[i].kind == 1)) continue;
        const bool back = d[i].copy_back && d[i].bytes;
        if (back) {
            CHECK(k < down.recs.size());
            if (k >= down.recs.size()) break;
            CHECK(down.recs[k].dst == host[i].data() && down.recs[k].src == op[i] && down.recs[k].bytes == d[i].bytes);
            k++;
        }
        for (size_t j = 0; j < d[i].bytes; j++)
            CHECK(host[i][j] == (back ? (unsigned char)(0xA0 + i) : (unsigned char)(i * 37 + j * 11 + 1)));
        CHECK(host[i][d[i].bytes] == 0);                 // nothing past the declared bytes
    }
    CHECK(k == down.recs.size());
    // a copy that fails on its k-th call: that error, and no copy after it
    for (int dir = 0; dir < 2; dir++) {
        const size_t total = dir ? down.recs.size() : up.recs.size();
        for (size_t f = 1; f <= total; f++) {
            CopyLog bad;
            bad.fail_at = (long)f;
            CHECK((dir ? plan.download(bad) : plan.upload(bad)) == COPY_ERR && bad.recs.size() == f);
        }
    }
}

// sf_request_tokens' staging: the offsets as they were written before Layout
static void token_chain(uint32_t n, uint32_t n_vals, bool has_param, bool param_off, bool want_rem, bool want_wait) {
    size_t off_fid = 0, off_cnt = align_up(off_fid + (size_t)n * 8), off_fl = align_up(off_cnt + (size_t)n * 4),
           off_ts = align_up(off_fl + n), off_tag = align_up(off_ts + (size_t)n * 8),
           off_bits = align_up(off_tag + (has_param ? n_vals : 0)),
           off_po = align_up(off_bits + (has_param ? (size_t)n_vals * 8 : 0)),
           off_st = align_up(off_po + (param_off ? ((size_t)n + 1) * 4 : 0)),
           off_rem = align_up(off_st + n), off_wt = align_up(off_rem + (size_t)n * 4), need = align_up(off_wt + (size_t)n * 4);
    const std::vector<Decl> d = {d_in(true, (size_t)n * 8), d_in(true, (size_t)n * 4), d_in(true, n), d_in(true, (size_t)n * 8),
                                 d_in(has_param, n_vals), d_in(has_param, (size_t)n_vals * 8),
                                 d_in(param_off, ((size_t)n + 1) * 4),
                                 d_out(true, n), d_out(true, (size_t)n * 4, want_rem), d_out(true, (size_t)n * 4, want_wait)};
    const std::vector<size_t> want = {off_fid, off_cnt, off_fl, off_ts, off_tag, off_bits, off_po, off_st, off_rem, off_wt};
    plan_check(d, true, true, &want, need);
    for (int form = 0; form < 3; form++) plan_check(d, form & 1, form & 2);    // mixed and device forms
}

// stage_batch's host input staging: the offsets as they were written before Layout
static void stage_chain(uint32_t n, uint32_t arg_slots, uint32_t n_elems, bool entry_ref, bool create_ts, bool n_args,
                        bool coll, bool origin, bool context) {
    size_t need = 0;
    size_t o_res = need; need += align_up((size_t)n * 4);
    size_t o_ts = need; need += align_up((size_t)n * 8);
    size_t o_cnt = need; need += align_up((size_t)n * 4);
    size_t o_fl = need; need += align_up((size_t)n);
    size_t o_er = need; need += entry_ref ? align_up((size_t)n * 8) : 0;
    size_t o_ct = need; need += (entry_ref && create_ts) ? align_up((size_t)n * 8) : 0;
    size_t o_na = need; need += n_args ? align_up((size_t)n) : 0;
    size_t o_at = need; need += align_up((size_t)n * arg_slots);
    size_t o_ab = need; need += align_up((size_t)n * arg_slots * 8);
    size_t o_eo = need; need += coll ? align_up(((size_t)n * arg_slots + 1) * 4) : 0;
    size_t o_et = need; need += coll ? align_up((size_t)n_elems) : 0;
    size_t o_eb = need; need += coll ? align_up((size_t)n_elems * 8) : 0;
    size_t o_og = need; need += origin ? align_up((size_t)n * 4) : 0;
    size_t o_cx = need; need += context ? align_up((size_t)n * 4) : 0;
    // (an array is declared off when the batch has none of it: n == 0, no slots, no elements)
    const size_t na = (size_t)n * arg_slots;
    const std::vector<Decl> d = {
        d_in(n, (size_t)n * 4), d_in(n, (size_t)n * 8), d_in(n, (size_t)n * 4), d_in(n, n),
        d_in(entry_ref && n, (size_t)n * 8), d_in(entry_ref && create_ts && n, (size_t)n * 8), d_in(n_args && n, n),
        d_in(na, na), d_in(na, na * 8), d_in(coll, (na + 1) * 4), d_in(coll && n_elems, n_elems),
        d_in(coll && n_elems, (size_t)n_elems * 8), d_in(origin && n, (size_t)n * 4), d_in(context && n, (size_t)n * 4)};
    const std::vector<size_t> want = {o_res, o_ts, o_cnt, o_fl, o_er, o_ct, o_na, o_at, o_ab, o_eo, o_et, o_eb, o_og, o_cx};
    plan_check(d, true, false, &want, need);
    plan_check(d, false, false);
    // the verdicts: status always, wait_ms / rule_idx when the caller has them
    for (int m = 0; m < 4; m++) {
        const std::vector<Decl> v = {d_out(true, n), d_out(m & 1, (size_t)n * 4), d_out(m & 2, (size_t)n * 2)};
        plan_check(v, false, true);
        plan_check(v, false, false);
    }
}

// scratch in either form, a room wider than the copy, and the inline capacity
static void plan_cases() {
    for (uint32_t n : {0u, 1u, 255u, 256u, 257u})
        for (int m = 0; m < 8; m++) {
            const std::vector<Decl> d = {d_in(true, n, (size_t)n + 16), d_scratch(m & 1, (size_t)n * 4), d_out(m & 2, n, m & 4),
                                         d_scratch(true, 16), d_in(m & 4, 0)};
            for (int form = 0; form < 4; form++) plan_check(d, form & 1, form & 2);
        }
    StagePlan full(true, true);
    char* p[StagePlan::CAP];
    for (int i = 0; i < StagePlan::CAP; i++) full.scratch(&p[i], 1);
    CHECK(full.size() == (size_t)StagePlan::CAP * 256);
}

static void layout_cases() {
    const uint32_t ns[] = {0, 1, 255, 256, 257};
    for (uint32_t n : ns) {
        for (int m = 0; m < 16; m++) {
            token_chain(n, n, m & 1, m & 2, m & 4, m & 8);
            token_chain(n, 2 * n + 3, m & 1, m & 2, m & 4, m & 8);   // collection params: more values than requests
            token_chain(n, 0, m & 1, m & 2, m & 4, m & 8);           // param arrays passed with no value
        }
        for (int m = 0; m < 64; m++)
            for (uint32_t slots : {0u, 1u, 3u})
                stage_chain(n, slots, 2 * n + 1, m & 1, m & 2, m & 4, m & 8, m & 16, m & 32);
    }
    Layout L;
    CHECK(L.size() == 0 && L.take(0) == 0 && L.size() == 0 && L.take(1) == 0 && L.take(256) == 256 && L.take(257) == 512);
    CHECK(L.size() == 1024 && L.take_if(false, 99) == 1024 && L.size() == 1024);
}

int main() {
    pool_cases();
    growbuf_cases();
    tok_cases();
    cc_cases();
    dg_cases();
    layout_cases();
    plan_cases();
    CHECK(live() == 0 && n_alloc == n_free && fail_in == 0);
    std::printf("%ld allocations, %ld frees, %d failures\n", n_alloc, n_free, failures);
    return failures ? 1 : 0;
}
