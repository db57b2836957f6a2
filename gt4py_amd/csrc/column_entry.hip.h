// What the COLUMN entries (vertical_remap, vertical_interp) share: pair entries (field_args.hip.h) whose kernel gives one thread a
// whole column (i, j) of up to PAIR_MAX_FIELDS (dst, src) pairs and of two shared fields along K -- the coordinate of the source
// levels and of the target levels, an IJK field or a Field[K] broadcast to every column.
//
// What differs between the entries is DATA: a column entry states a ColumnEntry (its names in the messages, how many more items
// than levels a shared field has, the least ns, its dry-run bit, its BoxChecks), an args struct that derives from ColumnArgs and
// adds its own scalars, its scalar checks (method, ...) and its kernel.  From here it takes
//   column_call     the checks in front of its own scalar checks: null pointers, nfields, the level and extent bounds, the flags
//   column_fields   the checks behind them -- item sizes, every field's box, the empty extent, "no dst meets anything read", the
//                   block count, *launches, the dry run -- and the fill of the ColumnArgs; *blocks stays 0 where nothing is launched
// and it keeps the loop over next_pair_batch with one hipLaunchKernelGGL per kernel template, as every pair entry does.  The
// kernels' openings (the lane's column, the bases of its coordinate, src and dst columns) are NOT shared: every form of a common
// device function that was tried moved the kernels' register counts.
#pragma once

#include "common.hip.h"
#include "field_args.hip.h"

namespace gt4mi {

constexpr int COLUMN_TILE_I = 64, COLUMN_TILE_J = 4;  // a workgroup: 64 columns along I (one wave) by 4 along J
constexpr int COLUMN_SHARED_FREE_AXES = 3;  // a Field[K]: stride 0 along I / J, one item for every i / j, no shape to check

struct ColumnEntry {
    const char* name;       // the entry's name in front of every message
    const char* shared[2];  // what the messages call the shared field of the sources / of the targets
    const char* item;       // what the size message calls an item of them: "edge" or "coordinate"
    int surplus;            // items a shared field has along K beyond the levels: 1 for edges, 0 for coordinates
    int64_t least_ns;       // the fewest source levels
    const char* levels;     // how the refusal of ns / nd ends: what is needed
    int dry_run;            // the entry's GT4MI_*_DRY_RUN bit, the only known flag
    BoxChecks checks;
};

// the leading members of a column kernel's arguments; an entry's own scalars follow in its derived struct
struct ColumnArgs {
    PairEntry e[PAIR_MAX_FIELDS];
    SharedField zs, zd;  // item 0 of the box's first column; stride 0 along I / J broadcasts
    int ni, nj, ns, nd, nf;
    unsigned tiles_i;
};

inline int column_call(const ColumnEntry& c, const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* shared_src,
                       const gt4mi_field* shared_dst, const int64_t extent_ij[2], int64_t ns, int64_t nd, int flags, int* launches) {
    if (launches) *launches = 0;
    if (dst == nullptr || src == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: %s is null", c.name, dst == nullptr ? "dst" : "src");
    if (shared_src == nullptr || shared_dst == nullptr)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: %s is null", c.name, shared_src == nullptr ? c.shared[0] : c.shared[1]);
    if (extent_ij == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: extent_ij is null", c.name);
    if (nfields < 1) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: nfields = %d, at least one pair is needed", c.name, nfields);
    if (ns < c.least_ns || nd < 1 || ns >= INT32_MAX - 2 || nd >= INT32_MAX - 2)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: ns = %lld source and nd = %lld target levels, %s", c.name, (long long)ns, (long long)nd,
                    c.levels);
    for (int ax = 0; ax < 2; ++ax)
        if (extent_ij[ax] < 0 || extent_ij[ax] > INT32_MAX)
            return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: invalid extent %lld along axis %d", c.name, (long long)extent_ij[ax], ax);
    if (flags & ~c.dry_run) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: unknown bits in flags 0x%x", c.name, (unsigned)flags);
    return GT4MI_OK;
}

inline void column_args(ColumnArgs& a, const gt4mi_field& shared_src, const gt4mi_field& shared_dst, const int64_t extent_ij[2], int64_t ns,
                        int64_t nd, int shared_elem_size, int64_t tiles_i) {
    a.zs = shared_field(shared_src, shared_elem_size), a.zd = shared_field(shared_dst, shared_elem_size);
    a.ni = (int)extent_ij[0], a.nj = (int)extent_ij[1], a.ns = (int)ns, a.nd = (int)nd;
    a.tiles_i = (unsigned)tiles_i;
}

inline int column_fields(const ColumnEntry& c, ColumnArgs& a, int64_t* blocks, const gt4mi_field* dst, const gt4mi_field* src, int nfields,
                         const gt4mi_field* shared_src, const gt4mi_field* shared_dst, const int64_t extent_ij[2], int64_t ns, int64_t nd,
                         int elem_size, int shared_elem_size, int flags, int* launches) {
    *blocks = 0;
    if (elem_size != 4 && elem_size != 8)
        return fail(GT4MI_ERR_UNSUPPORTED, "%s: field item size %d is not supported (float32 or float64)", c.name, elem_size);
    if (shared_elem_size != 4 && shared_elem_size != 8)
        return fail(GT4MI_ERR_UNSUPPORTED, "%s: %s item size %d is not supported (float32 or float64)", c.name, c.item, shared_elem_size);
    const int64_t d_ext[3] = {extent_ij[0], extent_ij[1], nd}, s_ext[3] = {extent_ij[0], extent_ij[1], ns};
    const int64_t dz_ext[3] = {extent_ij[0], extent_ij[1], nd + c.surplus}, sz_ext[3] = {extent_ij[0], extent_ij[1], ns + c.surplus};
    for (int n = 0; n < nfields; ++n) {
        if (int rc = check_box_field(c.checks, "dst", n, dst[n], d_ext, elem_size, true)) return rc;
        if (int rc = check_box_field(c.checks, "src", n, src[n], s_ext, elem_size, false)) return rc;
    }
    if (int rc = check_box_field(c.checks, c.shared[0], 0, *shared_src, sz_ext, shared_elem_size, false, COLUMN_SHARED_FREE_AXES)) return rc;
    if (int rc = check_box_field(c.checks, c.shared[1], 0, *shared_dst, dz_ext, shared_elem_size, false, COLUMN_SHARED_FREE_AXES)) return rc;
    if (extent_ij[0] == 0 || extent_ij[1] == 0) return GT4MI_OK;
    const NamedSpan shared[2] = {{c.shared[0], box_span(*shared_src, sz_ext, shared_elem_size)},
                                 {c.shared[1], box_span(*shared_dst, dz_ext, shared_elem_size)}};
    if (int rc = check_pairs_disjoint(c.name, dst, src, nfields, d_ext, s_ext, elem_size, elem_size, nullptr, shared, 2)) return rc;
    const int64_t tiles_i = cdiv(extent_ij[0], COLUMN_TILE_I), n_blocks = tiles_i * cdiv(extent_ij[1], COLUMN_TILE_J);
    if (n_blocks > INT32_MAX) return fail(GT4MI_ERR_UNSUPPORTED, "%s: too many columns for one launch", c.name);
    if (launches) *launches = (int)cdiv(nfields, PAIR_MAX_FIELDS);
    if (flags & c.dry_run) return GT4MI_OK;
    column_args(a, *shared_src, *shared_dst, extent_ij, ns, nd, shared_elem_size, tiles_i);
    *blocks = n_blocks;
    return GT4MI_OK;
}

}  // namespace gt4mi
