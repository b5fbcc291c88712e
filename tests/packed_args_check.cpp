// TEST-ONLY stand-alone host program: the argument tables of a packed batch
// (sf_packed_batch, sentinel_amd/csrc/sf_pkargs.h).  The same functions the
// device kernel runs are run here, one call per index as the kernel makes
// them, over
//   - random valid tables in all three shapes (both NULL shortcuts, the
//     explicit lists, explicit lists with collections): the dense slot-major
//     arrays must equal a direct construction from the per-event values;
//   - every malformed table: each must be refused, the copied element CSR must
//     stay within n_elems, and -- every array here is a heap block of exactly
//     its stated length -- the address sanitizer this is built with must see no
//     access outside them.
// Exit status 0: every case as expected.
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../sentinel_amd/csrc/sf_pkargs.h"

using namespace sf;

struct Table {
    uint32_t n = 0, slots = 0, n_elems = 0;
    bool has_event = true, has_off = true, has_eoff = true;
    std::vector<uint32_t> arg_event, arg_off, elem_off;
    std::vector<uint8_t> tag;
    std::vector<uint64_t> bits;
    long force_nae = -1;                                     // n_arg_events as stated, when not what the arrays imply
    uint32_t nae() const { return force_nae >= 0 ? (uint32_t)force_nae : has_event ? (uint32_t)arg_event.size() : n; }
    uint32_t nv() const { return (uint32_t)tag.size(); }
};
struct Dense {
    std::vector<uint8_t> nargs, atag;
    std::vector<uint64_t> abits;
    std::vector<uint32_t> eoff;
};

static const uint64_t UNSET = 0xA5A5A5A5A5A5A5A5ull;

// what the engine does with a table: the header, then one call per index
static bool expand(const Table& t, Dense& d) {
    d.nargs.assign(t.n, 0);
    d.atag.assign((size_t)t.n * t.slots, 0);
    d.abits.assign((size_t)t.n * t.slots, UNSET);
    d.eoff.assign(t.has_eoff ? t.nv() + 1 : 0, 0xFFFFFFFFu);
    const PkArgIn in{t.n, t.nae(), t.nv(), t.slots, t.n_elems,
                     t.has_event ? t.arg_event.data() : nullptr, t.has_off ? t.arg_off.data() : nullptr,
                     t.tag.data(), t.bits.data(), t.has_eoff ? t.elem_off.data() : nullptr};
    const PkArgOut out{d.nargs.data(), d.atag.data(), d.abits.data(), t.has_eoff ? d.eoff.data() : nullptr};
    if (!pk_args_header_ok(in)) return false;
    bool ok = true;                                           // pass 1: the verdict on the whole table
    for (uint32_t j = 0; j < in.n_arg_events; j++) ok &= pk_args_event_ok(in, j);
    if (in.elem_off)
        for (uint32_t v = 0; v <= in.n_values; v++) ok &= pk_args_elem_off(in, out, v);
    if (ok)                                                   // pass 2: only an accepted table is expanded
        for (uint32_t j = 0; j < in.n_arg_events; j++) pk_args_event_put(in, out, j);
    return ok;
}

// a random valid table and the dense arrays it stands for.  shape 0: both
// shortcuts, 1: explicit lists, 2: explicit lists with collections
static Table make(uint32_t seed, int shape, uint32_t n, uint32_t slots, Dense& want) {
    std::mt19937_64 rng(seed);
    Table t;
    t.n = n; t.slots = slots;
    t.has_event = t.has_off = shape != 0;
    t.has_eoff = shape == 2;
    want.nargs.assign(n, 0);
    want.atag.assign((size_t)n * slots, 0);
    want.abits.assign((size_t)n * slots, UNSET);
    if (t.has_off) t.arg_off.push_back(0);
    if (t.has_eoff) t.elem_off.push_back(0);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t na = shape == 0 ? slots : (uint32_t)(rng() % (slots + 1));
        if (shape != 0 && na == 0) continue;
        want.nargs[i] = (uint8_t)na;
        if (t.has_event) t.arg_event.push_back(i);
        for (uint32_t s = 0; s < na; s++) {
            const bool coll = shape == 2 && rng() % 3 == 0;
            const uint8_t tg = coll ? (uint8_t)SF_TAG_COLLECTION : (uint8_t)(rng() % 10);
            const uint64_t b = rng();
            want.atag[(size_t)s * n + i] = tg;
            want.abits[(size_t)s * n + i] = coll ? (uint64_t)t.tag.size() : b;     // a collection: its value index
            t.tag.push_back(tg);
            t.bits.push_back(b);
            if (t.has_eoff) {
                if (coll) t.n_elems += (uint32_t)(rng() % 5);
                t.elem_off.push_back(t.n_elems);
            }
        }
        if (t.has_off) t.arg_off.push_back((uint32_t)t.tag.size());
    }
    want.eoff = t.elem_off;
    return t;
}

static long bad = 0;
static void fail(const std::string& what) {
    if (bad++ < 20) std::printf("FAIL %s\n", what.c_str());
}

static void check_valid(uint32_t seed, int shape, uint32_t n, uint32_t slots) {
    Dense want, got;
    const Table t = make(seed, shape, n, slots, want);
    const std::string id = "valid seed " + std::to_string(seed) + " shape " + std::to_string(shape);
    if (!expand(t, got)) { fail(id + ": refused"); return; }
    if (got.nargs != want.nargs) fail(id + ": n_args");
    if (got.atag != want.atag) fail(id + ": tags");
    if (got.eoff != want.eoff) fail(id + ": element offsets");
    for (uint32_t i = 0; i < n; i++)
        for (uint32_t s = 0; s < want.nargs[i]; s++)
            if (got.abits[(size_t)s * n + i] != want.abits[(size_t)s * n + i]) { fail(id + ": bits"); return; }
}

static void check_refused(const char* name, Table t) {
    Dense got;
    if (expand(t, got)) fail(std::string(name) + ": accepted");
    // the verdict is global: no event of a refused table has arguments
    for (uint8_t x : got.nargs) if (x) { fail(std::string(name) + ": an event of a refused table has arguments"); break; }
    for (uint8_t x : got.atag) if (x) { fail(std::string(name) + ": a tag of a refused table was written"); break; }
    for (uint64_t x : got.abits) if (x != UNSET) { fail(std::string(name) + ": bits of a refused table were written"); break; }
    for (uint32_t x : got.eoff)
        if (x > t.n_elems && x != 0xFFFFFFFFu) fail(std::string(name) + ": copied element offset past n_elems");
}

int main() {
    uint32_t cases = 0;
    for (uint32_t seed = 1; seed <= 40; seed++)
        for (int shape = 0; shape < 3; shape++) {
            check_valid(seed, shape, 1 + seed * 37 % 500, 1 + seed % SF_MAX_ARGS);
            cases++;
        }
    check_valid(99, 1, 1, 1);
    check_valid(98, 2, 3000, SF_MAX_ARGS);

    // the malformed tables, each a valid one with one entry changed
    Dense unused;
    Table base = make(7, 2, 400, 3, unused);
    while (base.arg_event.size() < 8 || base.n_elems < 8) base = make(base.n + 1, 2, 400, 3, unused);
    const size_t m = base.arg_event.size();
    { Table t = base; t.arg_event[m - 1] = t.n; check_refused("index == n", t); }
    { Table t = base; t.arg_event[m - 1] = 0xFFFFFFFFu; check_refused("index far past n", t); }
    { Table t = base; t.arg_event[5] = t.arg_event[4]; check_refused("equal arg_event", t); }
    { Table t = base; t.arg_event[5] = t.arg_event[3]; check_refused("decreasing arg_event", t); }
    {   // two separated defects: entries 5 and 7 name one event, entry 6 between them is lower.  Only
        // entry 6 fails its own check; checked and written entry by entry, 5 and 7 would both be accepted
        // and write that event, one's collection tag possibly beside the other's scalar bits
        Table t = base;
        t.arg_event[6] = t.arg_event[4] > 0 ? t.arg_event[4] - 1 : 0;
        t.arg_event[7] = t.arg_event[5];
        check_refused("non-adjacent duplicate arg_event", t);
    }
    {   // the same with the duplicate far apart and a collection on one side
        Table t = base;
        const uint32_t dup = t.arg_event[m - 1];
        t.arg_event[2] = dup;                                 // entries 2 and m-1 name one event; entry 3 < dup fails
        check_refused("duplicate arg_event across the table", t);
    }
    { Table t = base; t.arg_off[4] = t.arg_off[3] - 1; check_refused("decreasing arg_off", t); }
    { Table t = base; t.arg_off[4] = 0xFFFFFFF0u; check_refused("arg_off far past n_values", t); }
    {   // one event with slots + 1 values: its neighbour gives one up
        Table t = base;
        size_t j = 1;
        while (j + 1 < m && !(t.arg_off[j + 1] - t.arg_off[j] == t.slots && t.arg_off[j + 2] - t.arg_off[j + 1] >= 1)) j++;
        if (j + 1 >= m) fail("no event to widen");
        else { t.arg_off[j + 1] += 1; check_refused("span above arg_slots", t); }
    }
    { Table t = base; t.arg_off[m] -= 1; check_refused("arg_off[last] below n_values", t); }
    { Table t = base; t.tag.push_back(1); t.bits.push_back(1); t.elem_off.push_back(t.n_elems);
      check_refused("arg_off[last] != n_values", t); }
    {
        Table t = base;
        size_t v = 1;
        while (v < t.elem_off.size() && t.elem_off[v] == 0) v++;
        if (v + 2 >= t.elem_off.size()) fail("no element offset to lower");
        else { t.elem_off[v + 1] = t.elem_off[v] - 1; check_refused("decreasing elem_off", t); }
    }
    { Table t = base; t.elem_off.back() = t.n_elems - 1; check_refused("elem_off[last] below n_elems", t); }
    { Table t = base; t.elem_off.back() = t.n_elems + 1000; check_refused("elem_off[last] above n_elems", t); }
    { Table t = base; t.elem_off[t.elem_off.size() / 2] = 0xFFFFFFF0u; check_refused("elem_off far past n_elems", t); }
    { Table t = base; t.has_eoff = false; t.elem_off.clear(); t.n_elems = 0; check_refused("collection without elem_off", t); }
    // what the scalars alone tell
    { Table t = make(3, 0, 50, 2, unused); t.tag.pop_back(); t.bits.pop_back(); check_refused("shortcut with a short value array", t); }
    { Table t = base; t.slots = 0; check_refused("arg_slots 0", t); }
    { Table t = base; t.slots = SF_MAX_ARGS + 1; check_refused("arg_slots above SF_MAX_ARGS", t); }
    { Table t = base; t.has_event = false; t.force_nae = (long)m; check_refused("NULL arg_event with fewer listed events than n", t); }
    { Table t = base; t.force_nae = (long)t.n + 1; check_refused("more listed events than n", t); }

    std::printf("%u valid tables, 21 malformed, %ld failures\n", cases + 2, bad);
    return bad ? 1 : 0;
}
