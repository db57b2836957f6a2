// What the utilities that work along the lines of I, J or K (line_solve, line_stats, line_scan, line_find, line_filter) share: the rule that picks one of
// their three paths (TILES, LANES, ITEMS: each entry's header says what its kernels do there) from the strides, which line a lane
// owns, the tiles of the TILES path, and -- for the two pair entries -- the front of the host entry, the grid of lines and the
// launch.  A further line utility states its kernels and its own checks and takes its geometry from here.
#pragma once

#include <type_traits>

#include "common.hip.h"
#include "field_args.hip.h"

#pragma clang fp contract(off)

namespace gt4mi {

constexpr int LINE_TILE_LINES = 64;  // TILES: lines of a tile = lanes of the wave that owns it
constexpr int LINE_TILE_BYTES = 128; // TILES: the run along the line a tile covers

static_assert(GT4MI_LINE_STATS_PATH_LANES == GT4MI_LINE_PATH_LANES && GT4MI_SCAN_PATH_LANES == GT4MI_LINE_PATH_LANES &&
              GT4MI_LINE_STATS_PATH_TILES == GT4MI_LINE_PATH_TILES && GT4MI_SCAN_PATH_TILES == GT4MI_LINE_PATH_TILES &&
              GT4MI_LINE_STATS_PATH_ITEMS == GT4MI_LINE_PATH_ITEMS && GT4MI_SCAN_PATH_ITEMS == GT4MI_LINE_PATH_ITEMS,
              "LinePlan's paths are reported as they are by all four entries (line_find reports GT4MI_LINE_PATH_* itself)");

// ---- the path rule ------------------------------------------------------------------------------------------------------------
// The path of a call and its lane axis.  The entry feeds every field of the call, one at a time: `strict` a field that must have
// unit item stride along an axis for that axis to count, `loose` one (a coefficient, a weight, a second field; null: none) that
// may also be broadcast (stride 0) along an axis that is not the line axis.  unit[ax] = every field fed so far allows ax.
struct LinePlan {
    int axis, elem_size;
    bool unit[3] = {true, true, true};

    LinePlan(int axis_, int elem_size_) : axis(axis_), elem_size(elem_size_) {}

    void strict(const gt4mi_field& f) {
        for (int ax = 0; ax < 3; ++ax) unit[ax] = unit[ax] && f.stride[ax] == elem_size;
    }
    void loose(const gt4mi_field* f) {
        for (int ax = 0; f != nullptr && ax < 3; ++ax) unit[ax] = unit[ax] && (f->stride[ax] == elem_size || (ax != axis && f->stride[ax] == 0));
    }

    // TILES, then LANES (the lower of the two other axes first), then ITEMS; an axis of extent 1 selects nothing
    int path(const int64_t extent[3], int* lane_axis) const {
        const int other0 = axis == 0 ? 1 : 0, other1 = axis == 2 ? 1 : 2;
        *lane_axis = other0;
        if (unit[axis] && extent[axis] > 1) return GT4MI_LINE_PATH_TILES;
        for (int ax : {other0, other1})
            if (unit[ax] && extent[ax] > 1) {
                *lane_axis = ax;
                return GT4MI_LINE_PATH_LANES;
            }
        return GT4MI_LINE_PATH_ITEMS;
    }
};

// ---- which line a lane owns ---------------------------------------------------------------------------------------------------
// The lines of a call are numbered line = ia + na * ib over the two axes other than the line axis, ia along the lane axis.  Lane
// threadIdx.x of workgroup `group` (of `block` lanes) owns line group * block + threadIdx.x, if there is one (`ok`).  A march
// kernel returns at once in a lane without a line.  In a tile kernel every lane of the wave takes part in the moves: a lane
// without a line computes on line 0's addresses (mine(), ia() and ib() are 0 there) and neither loads nor stores.
struct LineLane {
    int64_t line;  // what the lane would own
    bool ok;       // line < lines
    int na;
    // (formed where they are asked for: in a march kernel behind the return, where only lanes with a line divide)
    __device__ __forceinline__ int64_t mine() const { return ok ? line : 0; }
    __device__ __forceinline__ int64_t ib() const { return mine() / na; }
    __device__ __forceinline__ int64_t ia() const { return mine() - ib() * na; }
};

__device__ __forceinline__ LineLane line_lane(int block, unsigned group, int na, int64_t lines) {
    LineLane l;
    l.line = (int64_t)group * block + threadIdx.x;
    l.ok = l.line < lines;
    l.na = na;
    return l;
}

// ---- TILES --------------------------------------------------------------------------------------------------------------------
// One wave = one workgroup = LINE_TILE_LINES consecutive lines.  tile[l][r]: line l of the wave, item r of the run.  The
// transposition and the padded pitch are field_copy.hip.h's: a row of R items plus one, lane l on bank (l + r) mod 32.
template <typename T>
struct LineTile {
    static constexpr int R = LINE_TILE_BYTES / (int)sizeof(T);   // items of a run: 32 (float) / 16 (double)
    static constexpr int PITCH = R + 1;                          // odd in items of 4 / 8 bytes: see above
    static constexpr int LINES_PER_PASS = LINE_TILE_LINES / R;   // lines one load / store instruction of the wave covers
    static constexpr int PASSES = R;                             // = LINE_TILE_LINES / LINES_PER_PASS
};

// Move the run [m0, m0 + R) of the wave's lines between global memory and a tile; `off` is THIS lane's line offset (items) in the
// field (the line axis has item stride 1 on this path), `ok` whether this lane's line exists.  Lane l moves item (l % R) of line
// (pass * LINES_PER_PASS + l / R): consecutive lanes on consecutive items.  Item `skip` of the line (-1: none) is not moved: a[0] and
// c[n-1], which line_solve's contract never reads, stay out of the tile (their slots are never used).  A load takes a pointer to const.
template <typename T, bool LOAD>
__device__ __forceinline__ void line_tile_move(T (*tile)[LineTile<T>::PITCH], std::conditional_t<LOAD, const T, T>* base, int64_t off, bool ok,
                                               int m0, int n, int skip = -1) {
    using L = LineTile<T>;
    const int lane = (int)threadIdx.x;
    const int r = lane % L::R, sub = lane / L::R;
    // (offsets as two 32-bit halves through the cross-lane read)
    const int off_lo = (int)(uint32_t)(uint64_t)off, off_hi = (int)(uint32_t)((uint64_t)off >> 32);
    // every load of the move is issued before the first LDS store (a wave is alone on its SIMD: nothing else hides the latency)
    T v[L::PASSES];
    uint32_t there = 0;
#pragma unroll
    for (int p = 0; p < L::PASSES; ++p) {
        const int l = p * L::LINES_PER_PASS + sub;
        const int64_t o = (int64_t)(((uint64_t)(uint32_t)__shfl(off_hi, l) << 32) | (uint64_t)(uint32_t)__shfl(off_lo, l));
        const bool here = __shfl((int)ok, l) != 0 && m0 + r < n && m0 + r != skip;
        there |= (uint32_t)here << p;
        if constexpr (LOAD) {
            v[p] = T(0);
            if (here) v[p] = base[o + (m0 + r)];
        } else {
            if (here) base[o + (m0 + r)] = tile[l][r];
        }
    }
    if constexpr (LOAD) {
#pragma unroll
        for (int p = 0; p < L::PASSES; ++p)
            if (there >> p & 1u) tile[p * L::LINES_PER_PASS + sub][r] = v[p];
    }
}

// ---- the host side of the pair entries (line_solve, line_scan) ------------------------------------------------------------------
// The front of the entry, every refusal in the order and the words it has always had: dst / src / extent not null (`missing`: the
// name of a shared field that is null and must not be, or null), at least one pair, the extent's range, the axis, `own_scalars()`
// (the entry's op and flags), the item size, `own_rules()` (what the entry asks of the box once those are known), then every
// pair's fields against the box.  Both callables return a status.  *free_axes: a 1-d shared field has stride 0 along the two
// axes other than the line axis and no shape to check there.
template <typename Scalars, typename Rules>
inline int line_front(const BoxChecks& c, const PairRoles& r, const gt4mi_field* dst, const gt4mi_field* src, int nfields, const char* missing,
                      const int64_t* extent, int axis, int elem_size, Scalars&& own_scalars, Rules&& own_rules, int* free_axes) {
    if (dst == nullptr || src == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: %s is null", c.entry, dst == nullptr ? r.dst : r.src);
    if (missing != nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: %s is null", c.entry, missing);
    if (extent == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: extent is null", c.entry);
    if (nfields < 1) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: nfields = %d, at least one pair is needed", c.entry, nfields);
    for (int ax = 0; ax < 3; ++ax)
        if (extent[ax] < 0 || extent[ax] > INT32_MAX)
            return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: invalid extent %lld along axis %d", c.entry, (long long)extent[ax], ax);
    if (axis < 0 || axis > 2) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: axis %d is not 0 (I), 1 (J) or 2 (K)", c.entry, axis);
    if (int rc = own_scalars()) return rc;
    if (elem_size != 4 && elem_size != 8)
        return fail(GT4MI_ERR_UNSUPPORTED, "%s: item size %d is not supported (float32 or float64)", c.entry, elem_size);
    if (int rc = own_rules()) return rc;
    for (int k = 0; k < nfields; ++k) {
        if (int rc = check_box_field(c, r.dst, k, dst[k], extent, elem_size, true)) return rc;
        if (int rc = check_box_field(c, r.src, k, src[k], extent, elem_size, false)) return rc;
    }
    *free_axes = 7 & ~(1 << axis);
    return GT4MI_OK;
}

// The lines of a call once its fields are fed to `plan`: the path, the axes as the kernels take them ([0] the line axis, [1] the
// lane axis A, [2] the remaining axis B) and the extents along A and B.  Refuses more lines than a grid of `block` lanes counts.
struct LineGrid {
    int path, order[3], na, nb;
    int64_t lines;
};

inline int line_grid(const char* entry, const LinePlan& plan, const int64_t extent[3], int block, LineGrid* g) {
    int lane_axis = 0;
    g->path = plan.path(extent, &lane_axis);
    g->order[0] = plan.axis, g->order[1] = lane_axis, g->order[2] = 3 - plan.axis - lane_axis;
    g->na = (int)extent[g->order[1]], g->nb = (int)extent[g->order[2]];
    g->lines = extent[g->order[1]] * extent[g->order[2]];
    if (g->lines > (int64_t)INT32_MAX - block) return fail(GT4MI_ERR_UNSUPPORTED, "%s: too many lines for one launch", entry);
    return GT4MI_OK;
}

// One launch over `lines` lines: the tile kernel (a wave per workgroup) on TILES, else a march kernel on workgroups of `block`
// lanes -- `lanes` with its look-ahead on LANES, `items` (AHEAD = 1) on ITEMS.
template <typename Args>
inline void line_launch(int path, int64_t lines, int block, void (*tile)(Args), void (*lanes)(Args), void (*items)(Args), const Args& a,
                        hipStream_t stream) {
    void (*const kernel)(Args) = path == GT4MI_LINE_PATH_TILES ? tile : path == GT4MI_LINE_PATH_LANES ? lanes : items;
    const int width = path == GT4MI_LINE_PATH_TILES ? LINE_TILE_LINES : block;
    hipLaunchKernelGGL(kernel, dim3((unsigned)cdiv(lines, width)), dim3(width), 0, stream, a);
}

}  // namespace gt4mi
