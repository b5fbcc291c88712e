// TEST-ONLY stand-alone host program: the memory ownership types of the engine
// (sentinel_amd/csrc/sf_mem.h) and the work-set growth functions built on them
// (sf_worksets.h), on a malloc backend that can fail the k-th allocation.
//   - DevPool: every allocation is freed exactly once, by release or by the
//     destructor; a pointer released twice or never seen is reported, not freed;
//   - GrowBuf: reallocates only when it must, and is empty after a failure;
//   - the work sets (TokWork, CcWork, DegradeWork): with any one allocation of
//     a growth step failing, the set reads capacity 0, every pointer null and
//     nothing leaked, and the retry builds the whole set;
//   - Layout: the offsets of the token request staging and of the host batch
//     staging equal the align_up chains the engine computed by hand before.
// Built with the address and undefined-behaviour sanitizers: a double free, a
// leak at exit or an access outside a block ends the run.  Exit status 0 and
// " 0 failures": every case as expected.
#include <cstdio>
#include <cstdlib>
#include <set>

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

// sf_request_tokens' staging as it was written before Layout
static void token_chain(uint32_t n, uint32_t n_vals, bool has_param, bool param_off) {
    size_t off_fid = 0, off_cnt = align_up(off_fid + (size_t)n * 8), off_fl = align_up(off_cnt + (size_t)n * 4),
           off_ts = align_up(off_fl + n), off_tag = align_up(off_ts + (size_t)n * 8),
           off_bits = align_up(off_tag + (has_param ? n_vals : 0)),
           off_po = align_up(off_bits + (has_param ? (size_t)n_vals * 8 : 0)),
           off_st = align_up(off_po + (param_off ? ((size_t)n + 1) * 4 : 0)),
           off_rem = align_up(off_st + n), off_wt = align_up(off_rem + (size_t)n * 4), need = align_up(off_wt + (size_t)n * 4);
    Layout L;
    CHECK(L.take((size_t)n * 8) == off_fid); CHECK(L.take((size_t)n * 4) == off_cnt); CHECK(L.take(n) == off_fl);
    CHECK(L.take((size_t)n * 8) == off_ts);
    const size_t g_tag = L.take_if(has_param, n_vals), g_bits = L.take_if(has_param, (size_t)n_vals * 8);
    const size_t g_po = L.take_if(param_off, ((size_t)n + 1) * 4);
    if (has_param) { CHECK(g_tag == off_tag); CHECK(g_bits == off_bits); }
    if (param_off) CHECK(g_po == off_po);
    CHECK(L.take(n) == off_st); CHECK(L.take((size_t)n * 4) == off_rem); CHECK(L.take((size_t)n * 4) == off_wt);
    CHECK(L.size() == need);
}

// stage_batch's host input staging as it was written before Layout
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
    Layout L;
    CHECK(L.take((size_t)n * 4) == o_res); CHECK(L.take((size_t)n * 8) == o_ts); CHECK(L.take((size_t)n * 4) == o_cnt);
    CHECK(L.take(n) == o_fl);
    CHECK(L.take_if(entry_ref, (size_t)n * 8) == o_er);
    CHECK(L.take_if(entry_ref && create_ts, (size_t)n * 8) == o_ct);
    CHECK(L.take_if(n_args, n) == o_na);
    CHECK(L.take((size_t)n * arg_slots) == o_at); CHECK(L.take((size_t)n * arg_slots * 8) == o_ab);
    CHECK(L.take_if(coll, ((size_t)n * arg_slots + 1) * 4) == o_eo);
    CHECK(L.take_if(coll, n_elems) == o_et); CHECK(L.take_if(coll, (size_t)n_elems * 8) == o_eb);
    CHECK(L.take_if(origin, (size_t)n * 4) == o_og); CHECK(L.take_if(context, (size_t)n * 4) == o_cx);
    CHECK(L.size() == need);
}

static void layout_cases() {
    const uint32_t ns[] = {0, 1, 255, 256, 257};
    for (uint32_t n : ns) {
        for (int m = 0; m < 4; m++) {
            token_chain(n, n, m & 1, m & 2);
            token_chain(n, 2 * n + 3, m & 1, m & 2);             // collection params: more values than requests
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
    CHECK(live() == 0 && n_alloc == n_free && fail_in == 0);
    std::printf("%ld allocations, %ld frees, %d failures\n", n_alloc, n_free, failures);
    return failures ? 1 : 0;
}
