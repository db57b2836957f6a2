// Host-side helpers that the multi-field utility entries (halo_fill, field_stats, level_stats, field_copy, vertical_remap,
// horizontal_interp, departure_interp, point_sample, horizontal_remap, line_solve, line_scan) share: where a field's origin item is, which bytes its box touches, the per-field argument check and
// the "no dst meets anything that is read" sweep.  What differs between the entries is DATA (BoxChecks, the arguments of
// check_box_field): a new entry states its differences here instead of copying a check function.  The messages are part of
// the library's behaviour (tests/test_refusal_messages.py holds them byte for byte).
//
// The PAIR entries (vertical_remap, horizontal_interp, departure_interp, point_sample, horizontal_remap, line_solve, line_scan) take (written, read) pairs, up to
// PAIR_MAX_FIELDS per launch, the descriptors passed by value, the kernel instantiated for 1, 4 and 8 entries.  Such an entry states
// its own args struct (`PairEntry e[PAIR_MAX_FIELDS]` first, then its SharedFields and scalars, and an `int nf`), its kernel
// template with NF as a parameter, its scalar checks and its BoxChecks.  From here it takes the checks above, shared_field for what
// every pair reads, next_pair_batch for the loop over the launches of a call, with_pair_entries for NF and with_item_type for
// float / double; it keeps one hipLaunchKernelGGL per kernel template and the GT4MI_HIP_CHECK after each batch.
#pragma once

#include <type_traits>

#include "common.hip.h"

namespace gt4mi {

// the item at the field's origin
inline char* origin_ptr(const gt4mi_field& f) {
    return static_cast<char*>(f.data) + f.origin[0] * f.stride[0] + f.origin[1] * f.stride[1] + f.origin[2] * f.stride[2];
}

// strides in ITEMS (the callers have checked that the byte strides are multiples of the item size); with an `order`, out[x] is the
// stride along axis order[x]
inline void item_strides(const gt4mi_field& f, int elem_size, int64_t out[3], const int* order = nullptr) {
    for (int x = 0; x < 3; ++x) out[x] = f.stride[order != nullptr ? order[x] : x] / elem_size;
}

// the byte range the box [origin, origin + extent) of a field touches; `grow` (null: none) widens the box by grow[0 / 2] points
// below and grow[1 / 3] above along I / J
inline ByteSpan box_span(const gt4mi_field& f, const int64_t extent[3], int elem_size, const int64_t* grow = nullptr) {
    int64_t lo = 0, hi = 0;
    for (int ax = 0; ax < 3; ++ax) {
        const int64_t below = grow != nullptr && ax < 2 ? grow[2 * ax] : 0, above = grow != nullptr && ax < 2 ? grow[2 * ax + 1] : 0;
        const int64_t x = (f.origin[ax] - below) * f.stride[ax], y = (f.origin[ax] + extent[ax] + above - 1) * f.stride[ax];
        lo += x < y ? x : y;
        hi += x < y ? y : x;
    }
    const uintptr_t base = reinterpret_cast<uintptr_t>(f.data);
    return ByteSpan{base + (uintptr_t)lo, base + (uintptr_t)(hi + elem_size)};
}

// what the messages and rules of check_box_field take from the entry
struct BoxChecks {
    const char* entry;      // the entry's name in front of every message
    const char* box;        // what the entry calls its box: "extent" or "domain"
    const char* hint;       // who may be broadcast, in the refusal of stride 0 on a field that may not
    bool free_needs_extent; // a stride-0 axis is free of the shape check only where the box is longer than 1 (the stats entries)
    bool reach;             // the bounds messages name a reach (horizontal_interp, also where it is 0)
};

// One field of a call: not null, aligned to its item size, strides multiples of it, no stride 0 on an extent above 1 for a
// field that must not be broadcast (`solid`: every written field), origin and box inside the shape.  `free_axes`: bit ax set =
// stride 0 along ax broadcasts one item to every index, and the axis has no shape to check.  `grow` as in box_span.
inline int check_box_field(const BoxChecks& c, const char* what, int n, const gt4mi_field& f, const int64_t extent[3], int elem_size,
                           bool solid, int free_axes = 0, const int64_t* grow = nullptr) {
    if (f.data == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: %s %d is null", c.entry, what, n);
    if (reinterpret_cast<uintptr_t>(f.data) % (uintptr_t)elem_size != 0)
        return fail(GT4MI_ERR_UNSUPPORTED, "%s: %s %d is not aligned to its item size", c.entry, what, n);
    for (int ax = 0; ax < 3; ++ax) {
        if (f.stride[ax] % elem_size != 0)
            return fail(GT4MI_ERR_UNSUPPORTED, "%s: %s %d: byte stride %lld along axis %d is not a multiple of the item size", c.entry,
                        what, n, (long long)f.stride[ax], ax);
        if (solid && f.stride[ax] == 0 && extent[ax] > 1)
            return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: %s %d has stride 0 along axis %d (%s)", c.entry, what, n, ax, c.hint);
        if ((free_axes >> ax & 1) && f.stride[ax] == 0 && (!c.free_needs_extent || extent[ax] > 1)) continue;
        const int64_t lo = grow != nullptr && ax < 2 ? grow[2 * ax] : 0, hi = grow != nullptr && ax < 2 ? grow[2 * ax + 1] : 0;
        if (f.origin[ax] < 0)
            return fail(GT4MI_ERR_OUT_OF_BOUNDS, "%s: %s %d: negative origin %lld along axis %d", c.entry, what, n,
                        (long long)f.origin[ax], ax);
        if (f.origin[ax] < lo)
            return fail(GT4MI_ERR_OUT_OF_BOUNDS, "%s: %s %d: origin %lld along axis %d leaves no room for a reach of %lld below the domain",
                        c.entry, what, n, (long long)f.origin[ax], ax, (long long)lo);
        if (f.origin[ax] + extent[ax] + hi > f.shape[ax]) {
            if (c.reach)
                return fail(GT4MI_ERR_OUT_OF_BOUNDS, "%s: %s %d: origin %lld + %s %lld + reach %lld along axis %d is outside the array (shape %lld)",
                            c.entry, what, n, (long long)f.origin[ax], c.box, (long long)extent[ax], (long long)hi, ax, (long long)f.shape[ax]);
            return fail(GT4MI_ERR_OUT_OF_BOUNDS, "%s: %s %d: origin %lld + %s %lld along axis %d is outside the array (shape %lld)", c.entry,
                        what, n, (long long)f.origin[ax], c.box, (long long)extent[ax], ax, (long long)f.shape[ax]);
        }
    }
    return GT4MI_OK;
}

// a field that every pair of a call reads (edges, positions), for check_pairs_disjoint
struct NamedSpan {
    const char* name;
    ByteSpan span;
};

// what check_pairs_disjoint takes from the entry where it differs from the default {"dst", "src", false}
struct PairRoles {
    const char* dst;  // what the messages call the written field of a pair ...
    const char* src;  // ... and the read one
    bool same_box;    // dst[n] may BE src[n]: the same first item and the same strides (an in-place call); any other meeting is refused
};

// No dst may meet a shared field, any src (its box grown by `src_grow`) or another dst: what makes one launch without ordering
// between its workgroups correct.
inline int check_pairs_disjoint(const char* entry, const gt4mi_field* dst, const gt4mi_field* src, int n, const int64_t dst_extent[3],
                                const int64_t src_extent[3], int dsize, int ssize, const int64_t* src_grow = nullptr,
                                const NamedSpan* shared = nullptr, int nshared = 0, const PairRoles* roles = nullptr) {
    const char* const dname = roles != nullptr ? roles->dst : "dst";
    const char* const sname = roles != nullptr ? roles->src : "src";
    for (int a = 0; a < n; ++a) {
        const ByteSpan d = box_span(dst[a], dst_extent, dsize);
        for (int s = 0; s < nshared; ++s)
            if (spans_overlap(d, shared[s].span))
                return fail(GT4MI_ERR_UNSUPPORTED, "%s: %s %d and %s overlap in memory", entry, dname, a, shared[s].name);
        for (int b = 0; b < n; ++b) {
            const bool same = roles != nullptr && roles->same_box && a == b && origin_ptr(dst[a]) == origin_ptr(src[a]) &&
                              dst[a].stride[0] == src[a].stride[0] && dst[a].stride[1] == src[a].stride[1] && dst[a].stride[2] == src[a].stride[2];
            if (!same && spans_overlap(d, box_span(src[b], src_extent, ssize, src_grow)))
                return fail(GT4MI_ERR_UNSUPPORTED, "%s: %s %d and %s %d overlap in memory", entry, dname, a, sname, b);
            if (b > a && spans_overlap(d, box_span(dst[b], dst_extent, dsize)))
                return fail(GT4MI_ERR_UNSUPPORTED, "%s: %s %d and %s %d overlap in memory", entry, dname, a, dname, b);
        }
    }
    return GT4MI_OK;
}

// ---- the launches of the pair entries ----------------------------------------------------------------------------------------------
constexpr int PAIR_MAX_FIELDS = 8;  // pairs of one launch (include/gt4py_amd.h and the Python wrappers say "per 8 pairs")

struct PairEntry {
    char* dst;           // first item of the written box
    const char* src;     // first item of the read box
    int64_t d[3], s[3];  // strides in ITEMS of dst / src
};

// a field that every pair of a launch reads (edges, positions, coefficients)
struct SharedField {
    const char* p;  // first item of the box
    int64_t s[3];   // strides in ITEMS; 0 broadcasts
};

inline SharedField shared_field(const gt4mi_field& f, int elem_size, const int* order = nullptr) {
    SharedField q{};
    q.p = origin_ptr(f);
    item_strides(f, elem_size, q.s, order);
    return q;
}

// The loop over the launches of a call: `int next = 0; while (next_pair_batch(a, dst, src, &next, ...)) { launch a; }`.  False when
// no pair is left; else pairs [*next, *next + a.nf) go to a.e[0 .. a.nf), the rest of a.e is zeroed (the kernel is handed the whole
// block) and *next moves on.  `order` as in item_strides.
template <typename Args>
inline bool next_pair_batch(Args& a, const gt4mi_field* dst, const gt4mi_field* src, int* next, int nfields, int elem_size,
                            const int* order = nullptr) {
    const int first = *next;
    if (first >= nfields) return false;
    a.nf = nfields - first < PAIR_MAX_FIELDS ? nfields - first : PAIR_MAX_FIELDS;
    for (int n = 0; n < PAIR_MAX_FIELDS; ++n) {
        PairEntry& e = a.e[n];
        e = PairEntry{};
        if (n >= a.nf) continue;
        e.dst = origin_ptr(dst[first + n]), e.src = origin_ptr(src[first + n]);
        item_strides(dst[first + n], elem_size, e.d, order), item_strides(src[first + n], elem_size, e.s, order);
    }
    *next = first + a.nf;
    return true;
}

// The entries a kernel is instantiated for, as a compile-time constant: f(std::integral_constant<int, NF>{}) with the smallest of
// 1, 4 and 8 that holds `nf`.
template <typename F>
inline void with_pair_entries(int nf, F&& f) {
    if (nf == 1) f(std::integral_constant<int, 1>{});
    else if (nf <= 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, PAIR_MAX_FIELDS>{});
}

// An item size the entry has checked to be 4 or 8 as a type: f(float{}) or f(double{}).
template <typename F>
inline void with_item_type(int elem_size, F&& f) {
    if (elem_size == 8) f(double{});
    else f(float{});
}

}  // namespace gt4mi
