// ParamFlow arguments of a packed batch (sf_packed_batch, sentinel_flow.h):
// the sparse tables a host sends -- the events that carry arguments, their
// values, the collections' element CSR -- expanded into the dense slot-major
// arrays the sort and decide phases read (DevBatch nargs / atag / abits,
// stride n), and the validation of every index before it is used.  One body
// for the device kernels (k_pk_args_check / k_pk_args, sf_packed.hip) and the host check
// (tests/packed_args_check.cpp): nothing here needs the HIP runtime.
//
// The dense arrays are zero-filled (nargs, atag) before the expansion, so an
// event that is not listed, and every event of a refused table, has no
// arguments.  A collection value carries its value index v: the copied
// elem_off is indexed by value (DevBatch::acsr, RsSinkFinal::put).
#pragma once
#include <stdint.h>

#include "../../include/sentinel_flow.h"

#ifndef SF_HD
#if defined(__HIPCC__)
#define SF_HD __host__ __device__ __forceinline__
#else
#define SF_HD inline
#endif
#endif

namespace sf {

struct PkArgIn {
    uint32_t n, n_arg_events, n_values, arg_slots, n_elems;
    const uint32_t* arg_event; const uint32_t* arg_off;
    const uint8_t* arg_tag; const uint64_t* arg_bits;
    const uint32_t* elem_off;
};
// nargs [n], atag / abits [arg_slots * n] slot-major; eoff [n_values + 1] (null without elem_off)
struct PkArgOut { uint8_t* nargs; uint8_t* atag; uint64_t* abits; uint32_t* eoff; };

// What the scalars alone tell (the caller checks them before any array is
// read): the slot count, and the lengths the two NULL shortcuts imply.
SF_HD bool pk_args_header_ok(const PkArgIn& in) {
    if (in.n_arg_events == 0 && in.n_values == 0) return true;    // no arguments: the rest is not read
    if (in.arg_slots < 1 || in.arg_slots > SF_MAX_ARGS) return false;
    if (in.n_arg_events > in.n) return false;
    if (!in.arg_event && in.n_arg_events != in.n) return false;
    if (!in.arg_off && (uint64_t)in.n_arg_events * in.arg_slots != in.n_values) return false;
    if ((uint64_t)in.n_values > (uint64_t)in.n_arg_events * in.arg_slots) return false;
    if (in.n_values && (!in.arg_tag || !in.arg_bits)) return false;
    return true;
}

// The verdict on a table is global: a defect anywhere refuses the whole table
// before anything dense is written.  Checked index by index the conditions are
// local (each entry against its neighbour), yet together they are the global
// ones: when every j passes, arg_event is strictly increasing as a whole, so
// no two listed entries name the same event and exactly one thread of the
// expansion writes an event's count, tags and bits.  A table with two
// separated defects (a non-adjacent duplicate) can therefore never leave a
// tag from one entry beside the bits of another.
//
// Pass 1, the j-th listed entry (j < n_arg_events): false when the table is
// malformed at j.  Reads only what the checks before it have bounded; writes
// nothing.
SF_HD bool pk_args_event_ok(const PkArgIn& in, uint32_t j) {
    uint32_t i = j;
    if (in.arg_event) {
        i = in.arg_event[j];
        if (j && in.arg_event[j - 1] >= i) return false;          // strictly increasing
    }
    if (i >= in.n) return false;
    uint32_t lo = j * in.arg_slots, hi = lo + in.arg_slots;       // (header: n_arg_events * arg_slots == n_values)
    if (in.arg_off) {
        lo = in.arg_off[j]; hi = in.arg_off[j + 1];
        if (hi < lo || hi - lo > in.arg_slots || hi > in.n_values) return false;
        if (j + 1 == in.n_arg_events && hi != in.n_values) return false;
    }
    if (!in.elem_off)                                             // a collection needs the CSR
        for (uint32_t v = lo; v < hi; v++)
            if (in.arg_tag[v] == SF_TAG_COLLECTION) return false;
    return true;
}

// Pass 2, only after every entry (and every elem_off entry) passed: the j-th
// listed event's count, tags and bits into the dense arrays.
SF_HD void pk_args_event_put(const PkArgIn& in, const PkArgOut& out, uint32_t j) {
    const uint32_t i = in.arg_event ? in.arg_event[j] : j;
    const uint32_t lo = in.arg_off ? in.arg_off[j] : j * in.arg_slots;
    const uint32_t na = in.arg_off ? in.arg_off[j + 1] - lo : in.arg_slots;
    out.nargs[i] = (uint8_t)na;
    for (uint32_t s = 0; s < na; s++) {
        const uint32_t v = lo + s;
        const uint8_t tg = in.arg_tag[v];
        out.atag[(size_t)s * in.n + i] = tg;
        out.abits[(size_t)s * in.n + i] = tg == SF_TAG_COLLECTION ? (uint64_t)v : in.arg_bits[v];
    }
}

// Pass 1, entry v (v <= n_values) of the element CSR into its copy.  The copy never
// points past n_elems, whatever the table holds, so the decide phase stays
// inside the element arrays it was handed; false: malformed at v.
SF_HD bool pk_args_elem_off(const PkArgIn& in, const PkArgOut& out, uint32_t v) {
    const uint32_t x = in.elem_off[v];
    bool ok = x <= in.n_elems;
    if (v && in.elem_off[v - 1] > x) ok = false;
    if (v == in.n_values && x != in.n_elems) ok = false;
    out.eoff[v] = ok ? x : in.n_elems;
    return ok;
}

}  // namespace sf
