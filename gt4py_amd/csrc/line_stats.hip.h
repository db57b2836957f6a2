// Statistics along the lines of I, J or K: the eight slots of field_stats.hip.h and the mean for EVERY LINE of the domain along
// `axis`, for up to 8 entries per launch, the field read ONCE, the result BIT-REPRODUCIBLE and left on the device as (nB, nA)
// sections -- what a stencil takes as Field[JK] (axis I: the zonal mean), Field[IK] (axis J) or Field[IJ] (axis K) of float64.
//
// NEW component, no reference counterpart: GTScript has no reduction over I or J; gt4py.cartesian leaves `field.sum(axis=0)` to
// numpy / cupy on storages that ARE numpy / cupy arrays.
//
// Entries, x = a or a - b, the slots, the NaN and signed-zero rules and the all-double, no-FMA arithmetic are those of
// field_stats.hip.h, whose device functions (StatsAcc, stats_init, stats_item, stats_load, stats_wave_values, stats_min / stats_max
// / stats_combine) do the work here too.
//
// THE ORDER OF THE ADDITIONS OF A LINE is a function of its length n alone -- not of the axis, the layout, the path, pointers,
// strides, the number of entries in the call, the grid or the arrival order of workgroups:
//   segments  G = GT4MI_LINE_STATS_SEGMENT items; S = ceil(n / G); segment s is the items m in [s G, min(n, (s + 1) G)).
//   inside    four accumulator sets: set p takes the items with m mod 4 == p in increasing m (sums start at +0.0, min at +inf,
//             max at -inf, counts at 0); a set whose sum |x| ended NaN sets min = max = NaN; the segment's value is
//             (A0 (+) A1) (+) (A2 (+) A3) -- all four sets take part, also one that owned no item.
//   across    the halving tree of level_stats_finish_kernel over the S segment values: new[i] = old[2i] (+) old[2i + 1], an odd
//             last one carried up unchanged, until one is left.  (Evaluated here as a binary counter: segment s is merged with the
//             finished subtrees of equal size to its left -- the same tree, node for node -- so S needs no bound in registers.)
//   mean      SUM / COUNT, one IEEE division (COUNT = n: exact in float64 whatever the order).
//   (+) as in field_stats.hip.h.  tests/line_stats_ref.py restates this order in plain Python and in numpy.
// A lane owns one (line, segment) pair from its first load to its store: nothing is shared between lanes but the staging tiles of
// the TILES path.  The segment values cross ONE launch boundary through the workspace,
//   partial[((entry * S + s) * 8 + slot) * lines + w],  w = x + nx * y  (x along the lane axis, y along the remaining axis),
// written with plain vector stores; a finish kernel on the same stream halves them.  With S == 1 the segment IS the line and the
// pass kernel stores the nine rows itself (the tree of one value is that value: the same bits, one launch fewer).
// No float atomics, no ticket, flag or spin, no workgroup waits for another, no scratch, and no address or loop bound depends on
// field data: every loop counts to n, G or the items of a tile, which the host has checked against every field's shape.
//
// THREE PATHS, chosen by the host from the strides (line_geometry.hip.h: LinePlan; reported as GT4MI_LINE_STATS_PATH_*), THE SAME ADDITIONS:
//   LANES  an axis OTHER than the line axis has unit stride in every field of the call (0 is allowed in an `other`): lanes run
//          along it, a thread marches over the at most G items of its pair, every step a coalesced row segment; the loads of
//          STATS_BATCH groups of 4 steps are issued before their adds.  On I-contiguous storage: axis J and K.
//   TILES  the LINE axis has unit stride: a workgroup IS one wave and takes 64 lines of ONE segment; tiles of 64 lines x one
//          128-byte run go through LDS with line_geometry.hip.h's transposition and padded pitch (LineTile, line_tile_move: item
//          loads, so any origin alignment works, and a run that ends inside a tile is masked), global access coalesced along the
//          line; the lane adds its run from LDS in m order.  `a` and `b` each have a tile; the tiles are private to the wave and
//          the barriers are wave barriers.  On I-contiguous storage: axis I.
//   ITEMS  anything else: the LANES kernel on whatever strides there are, uncoalesced: slow.
// RESULT: result[((entry * 9 + row) * nB + b) * nA + a], A < B the two remaining axes in I, J, K order: every (entry, row) is one
// contiguous section, and where the lane axis is A (always on I-contiguous storage) the stores are coalesced.
#pragma once

#include "field_stats.hip.h"
#include "line_geometry.hip.h"

namespace gt4mi {

constexpr int LINE_STATS_SEGMENT = GT4MI_LINE_STATS_SEGMENT;  // G: part of the bit contract
constexpr int LINE_STATS_ROWS = GT4MI_LINE_STATS_ROWS;
constexpr int LINE_STATS_SETS = 4;
constexpr int LINE_STATS_BLOCK = 256;
constexpr int LINE_STATS_LEVELS = 26;                          // of the finish kernel's counter: S <= ceil(2^31 / 64) = 2^25
constexpr int64_t LINE_STATS_MAX_PAIRS = (int64_t)1 << 30;     // (line, segment) pairs of a call: the grids count in 32 bits
constexpr int LINE_STATS_MAX_FIELDS = 65535;                   // the finish kernel's grid.z
static_assert(LINE_STATS_SEGMENT >= 64 && LINE_STATS_SEGMENT % 32 == 0, "G is a multiple of a float tile's run (and so of 4)");
static_assert(LINE_STATS_ROWS == STATS_SLOTS + 1 && GT4MI_LINE_STATS_MEAN == STATS_SLOTS, "row 8 is the mean");
static_assert(LINE_STATS_SETS == STATS_GROUP, "stats_load fetches one item per set");

// Every stride (ITEMS) is permuted by the host: l along the line axis, x along the lane axis X, y along the remaining axis Y.
// (Scalars, not arrays: the selection below then stays in registers.)
struct LineStatsEntry {
    const char* a;  // address of the first compute-domain point
    const char* b;  // nullptr: no second field
    int64_t al, ax, ay, bl, bx, by;
};

struct LineStatsArgs {
    LineStatsEntry e[STATS_MAX_ENTRIES];
    double* partials;  // of the launch's first entry (not touched when segments == 1)
    double* result;    // of the launch's first entry
    int64_t lines;     // nx * ny
    int n, nx, ny, segments;
    int swap;          // the lane axis X is B, not A: result index a = y, b = x
};

// (selected member by member with scalar moves: indexing the by-value argument block with blockIdx.y, or copying a whole entry under
// a condition, makes the compiler copy the block to scratch)
__device__ __forceinline__ LineStatsEntry line_stats_entry(const LineStatsArgs& g) {
    LineStatsEntry f = g.e[0];
#pragma unroll
    for (int k = 1; k < STATS_MAX_ENTRIES; ++k) {
        const bool mine = blockIdx.y == (unsigned)k;
        f.a = mine ? g.e[k].a : f.a, f.b = mine ? g.e[k].b : f.b;
        f.al = mine ? g.e[k].al : f.al, f.ax = mine ? g.e[k].ax : f.ax, f.ay = mine ? g.e[k].ay : f.ay;
        f.bl = mine ? g.e[k].bl : f.bl, f.bx = mine ? g.e[k].bx : f.bx, f.by = mine ? g.e[k].by : f.by;
    }
    return f;
}

__device__ __forceinline__ void line_stats_init(StatsAcc (&acc)[LINE_STATS_SETS]) {
#pragma unroll
    for (int p = 0; p < LINE_STATS_SETS; ++p) stats_init(acc[p]);
}

// where line w = x + nx * y stands in a section
__device__ __forceinline__ int64_t line_stats_section_index(int64_t w, int nx, int ny, int swap) {
    if (!swap) return w;
    const int64_t y = w / nx, x = w - y * nx;
    return y + (int64_t)ny * x;
}

// one row of one line; the thread that stores SUM stores the mean too
__device__ __forceinline__ void line_stats_store_row(double* result, unsigned entry, int slot, int64_t at, int64_t lines, int n, double v) {
    double* const r = result + (size_t)entry * LINE_STATS_ROWS * lines + at;
    r[(size_t)slot * lines] = v;
    if (slot == STATS_SUM) r[(size_t)GT4MI_LINE_STATS_MEAN * lines] = v / (double)n;
}

// The end of a pair: the NaN rule per set, (A0 (+) A1) (+) (A2 (+) A3), then the 8 values to the workspace -- or, where the
// segment is the whole line, to the result.
__device__ __forceinline__ void line_stats_put(const LineStatsArgs& g, StatsAcc (&acc)[LINE_STATS_SETS], int64_t w, int s) {
    double q[LINE_STATS_SETS][STATS_SLOTS];
#pragma unroll
    for (int p = 0; p < LINE_STATS_SETS; ++p) {
        if (acc[p].sum_abs != acc[p].sum_abs) acc[p].mn = acc[p].mx = __builtin_nan("");
        stats_wave_values(acc[p], q[p]);
    }
    const int64_t at = g.segments == 1 ? line_stats_section_index(w, g.nx, g.ny, g.swap) : 0;
    double* const p = g.partials + ((size_t)blockIdx.y * g.segments + s) * STATS_SLOTS * g.lines + w;
#pragma unroll
    for (int slot = 0; slot < STATS_SLOTS; ++slot) {
        const double v = stats_combine(slot, stats_combine(slot, q[0][slot], q[1][slot]), stats_combine(slot, q[2][slot], q[3][slot]));
        if (g.segments == 1) line_stats_store_row(g.result, blockIdx.y, slot, at, g.lines, g.n, v);
        else p[(size_t)slot * g.lines] = v;
    }
}

// LANES / ITEMS: the `count` items of pair (w, s) from `a` (and `b`), `sa` (`sb`) items apart, first item m0 (a multiple of 4).
// (The accumulators live in ONE instantiation from their start to the store: sharing them between the PAIR and the single-field
// code sends them to scratch.)
template <typename T, bool PAIR>
__device__ __forceinline__ void line_stats_march(const LineStatsArgs& g, const T* a, int64_t sa, const T* b, int64_t sb, int m0, int count,
                                                 int64_t w, int s) {
    StatsAcc acc[LINE_STATS_SETS];
    line_stats_init(acc);
    for (int r0 = 0; r0 < count; r0 += STATS_BATCH * STATS_GROUP) {
        T va[STATS_BATCH][STATS_GROUP], vb[STATS_BATCH][STATS_GROUP];
        int nvalid[STATS_BATCH];
#pragma unroll
        for (int u = 0; u < STATS_BATCH; ++u) {
            const int left = count - (r0 + u * STATS_GROUP);
            nvalid[u] = left < 0 ? 0 : (left > STATS_GROUP ? STATS_GROUP : left);
            const int first = nvalid[u] > 0 ? m0 + r0 + u * STATS_GROUP : 0;
            stats_load<T>(a, sa, false, first, nvalid[u], va[u]);
            if constexpr (PAIR) stats_load<T>(b, sb, false, first, nvalid[u], vb[u]);
        }
#pragma unroll
        for (int u = 0; u < STATS_BATCH; ++u) {
#pragma unroll
            for (int e = 0; e < STATS_GROUP; ++e)  // item m0 + r0 + 4 u + e: set e
                if (e < nvalid[u]) stats_item<PAIR>(acc[e], (double)va[u][e], PAIR ? (double)vb[u][e] : 0.0);
        }
    }
    line_stats_put(g, acc, w, s);
}

template <typename T>
__global__ void __launch_bounds__(LINE_STATS_BLOCK)
line_stats_march_kernel(const LineStatsArgs g) {
    const LineStatsEntry f = line_stats_entry(g);
    const int64_t id = (int64_t)blockIdx.x * LINE_STATS_BLOCK + threadIdx.x;  // w + lines * s
    if (id >= g.lines * g.segments) return;
    const int s = (int)(id / g.lines);
    const int64_t w = id - (int64_t)s * g.lines;
    const int64_t y = w / g.nx, x = w - y * g.nx;
    const int m0 = s * LINE_STATS_SEGMENT;  // < n
    const int rest = g.n - m0;
    const int count = rest < LINE_STATS_SEGMENT ? rest : LINE_STATS_SEGMENT;
    const T* const a = reinterpret_cast<const T*>(f.a) + x * f.ax + y * f.ay;
    if (f.b != nullptr)
        line_stats_march<T, true>(g, a, f.al, reinterpret_cast<const T*>(f.b) + x * f.bx + y * f.by, f.bl, m0, count, w, s);
    else
        line_stats_march<T, false>(g, a, f.al, nullptr, 0, m0, count, w, s);
}

// TILES: the `count` items (the same in every lane) of the wave's 64 pairs, tile by tile; this lane's pair is (w, s) if `ok`.
// Item r of a run goes to set r mod 4 (a run starts at a multiple of 4).  Every lane of the wave takes part in the moves.
template <typename T, bool PAIR>
__device__ __forceinline__ void line_stats_tiles(const LineStatsArgs& g, T (*ta)[LineTile<T>::PITCH], T (*tb)[LineTile<T>::PITCH], const T* a,
                                                 int64_t oa, const T* b, int64_t ob, bool ok, int count, int64_t w, int s) {
    constexpr int R = LineTile<T>::R;
    const int lane = (int)threadIdx.x;
    StatsAcc acc[LINE_STATS_SETS];
    line_stats_init(acc);
    for (int r0 = 0; r0 < count; r0 += R) {
        __syncthreads();  // (the adds of the tile before are done with the tiles)
        line_tile_move<T, true>(ta, a, oa, ok, r0, count);
        if constexpr (PAIR) line_tile_move<T, true>(tb, b, ob, ok, r0, count);
        __syncthreads();
        if (ok) {
            const int left = count - r0;
            if (left >= R) {
#pragma unroll
                for (int r = 0; r < R; ++r) stats_item<PAIR>(acc[r % LINE_STATS_SETS], (double)ta[lane][r], PAIR ? (double)tb[lane][r] : 0.0);
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (r < left) stats_item<PAIR>(acc[r % LINE_STATS_SETS], (double)ta[lane][r], PAIR ? (double)tb[lane][r] : 0.0);
            }
        }
    }
    if (ok) line_stats_put(g, acc, w, s);
}

// One wave = one workgroup = LINE_TILE_LINES consecutive lines of ONE segment.  SECOND: an entry of the launch has a second field
// (a launch without one keeps no tile for it).
template <typename T, bool SECOND>
__global__ void __launch_bounds__(LINE_TILE_LINES)
line_stats_tile_kernel(const LineStatsArgs g) {
    using L = LineTile<T>;
    __shared__ T ta[LINE_TILE_LINES][L::PITCH];
    __shared__ T tb[SECOND ? LINE_TILE_LINES : 1][L::PITCH];
    const LineStatsEntry f = line_stats_entry(g);
    const unsigned waves = (unsigned)((g.lines + LINE_TILE_LINES - 1) / LINE_TILE_LINES);  // per segment
    const int s = (int)(blockIdx.x / waves);
    const LineLane l = line_lane(LINE_TILE_LINES, blockIdx.x - (unsigned)s * waves, g.nx, g.lines);
    const bool ok = l.ok;
    const int64_t w = l.line, x = l.ia(), y = l.ib();
    const int m0 = s * LINE_STATS_SEGMENT;
    const int rest = g.n - m0;
    const int count = rest < LINE_STATS_SEGMENT ? rest : LINE_STATS_SEGMENT;
    // the offsets of this lane's segment (the line axis has item stride 1 on this path)
    const int64_t oa = x * f.ax + y * f.ay + m0, ob = x * f.bx + y * f.by + m0;
    const T* const a = reinterpret_cast<const T*>(f.a);
    if (SECOND && f.b != nullptr) line_stats_tiles<T, true>(g, ta, tb, a, oa, reinterpret_cast<const T*>(f.b), ob, ok, count, w, s);
    else line_stats_tiles<T, false>(g, ta, tb, a, oa, nullptr, 0, ok, count, w, s);
}

// One thread per (line, slot, entry): the S values of its line, LINE_STATS_AHEAD loads issued before they are merged.  level[l]
// holds the finished subtree of 2^l segments that waits for its right sibling: bit l of the number of segments merged so far.
constexpr int LINE_STATS_AHEAD = 8;

__global__ void __launch_bounds__(LINE_STATS_BLOCK)
line_stats_finish_kernel(const double* __restrict__ partials, double* __restrict__ result, int64_t lines, int segments, int n, int nx,
                         int ny, int swap) {
    const int64_t w = (int64_t)blockIdx.x * LINE_STATS_BLOCK + threadIdx.x;
    if (w >= lines) return;
    const int slot = (int)blockIdx.y;
    const double* const p = partials + ((size_t)blockIdx.z * segments * STATS_SLOTS + slot) * lines + w;
    const size_t step = (size_t)STATS_SLOTS * lines;
    double level[LINE_STATS_LEVELS];
#pragma unroll
    for (int l = 0; l < LINE_STATS_LEVELS; ++l) level[l] = 0.0;
    for (int s0 = 0; s0 < segments; s0 += LINE_STATS_AHEAD) {
        double v[LINE_STATS_AHEAD];
#pragma unroll
        for (int u = 0; u < LINE_STATS_AHEAD; ++u) v[u] = s0 + u < segments ? p[(size_t)(s0 + u) * step] : 0.0;
#pragma unroll
        for (int u = 0; u < LINE_STATS_AHEAD; ++u) {
            const int s = s0 + u;
            if (s < segments) {
                double x = v[u];
                bool placed = false;
#pragma unroll
                for (int l = 0; l < LINE_STATS_LEVELS; ++l) {
                    if (!placed) {
                        if (s >> l & 1) x = stats_combine(slot, level[l], x);  // its left sibling is finished: one node up
                        else level[l] = x, placed = true;
                    }
                }
            }
        }
    }
    // what is left are the odd last ones of their levels, carried up until they meet the subtree to their left
    double x = 0.0;
    bool have = false;
#pragma unroll
    for (int l = 0; l < LINE_STATS_LEVELS; ++l) {
        if (segments >> l & 1) {
            x = have ? stats_combine(slot, level[l], x) : level[l];
            have = true;
        }
    }
    line_stats_store_row(result, blockIdx.z, slot, line_stats_section_index(w, nx, ny, swap), lines, n, x);
}

template <typename T>
inline void line_stats_launch(const LineStatsArgs& a, int nf, int path, bool second, hipStream_t stream) {
    if (path == GT4MI_LINE_STATS_PATH_TILES) {
        const dim3 grid((unsigned)(cdiv(a.lines, LINE_TILE_LINES) * a.segments), (unsigned)nf);
        if (second) hipLaunchKernelGGL((line_stats_tile_kernel<T, true>), grid, dim3(LINE_TILE_LINES), 0, stream, a);
        else hipLaunchKernelGGL((line_stats_tile_kernel<T, false>), grid, dim3(LINE_TILE_LINES), 0, stream, a);
    } else {
        const dim3 grid((unsigned)cdiv(a.lines * a.segments, LINE_STATS_BLOCK), (unsigned)nf);
        hipLaunchKernelGGL((line_stats_march_kernel<T>), grid, dim3(LINE_STATS_BLOCK), 0, stream, a);
    }
}

// every check, then (unless `flags` carries GT4MI_STATS_DRY_RUN) the launches; *launches = kernels the call enqueues
inline int line_stats(const gt4mi_field* fields, const gt4mi_field* others, int nfields, const int64_t domain[3], int axis, int elem_size,
                      void* workspace, int64_t workspace_bytes, double* result, int flags, hipStream_t stream, int64_t* workspace_needed,
                      int* launches, int* path) {
    if (launches) *launches = 0;
    if (workspace_needed) *workspace_needed = 0;
    if (path) *path = -1;
    if (fields == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "line_stats: fields is null");
    if (nfields < 1) return fail(GT4MI_ERR_INVALID_ARGUMENT, "line_stats: nfields = %d, at least one field is needed", nfields);
    if (nfields > LINE_STATS_MAX_FIELDS)
        return fail(GT4MI_ERR_UNSUPPORTED, "line_stats: nfields = %d, more than %d fields in one call", nfields, LINE_STATS_MAX_FIELDS);
    if (int rc = check_domain(domain)) return rc;
    if (axis < 0 || axis > 2) return fail(GT4MI_ERR_INVALID_ARGUMENT, "line_stats: axis %d is not 0 (I), 1 (J) or 2 (K)", axis);
    for (int ax = 0; ax < 3; ++ax)
        if (domain[ax] < 1) return fail(GT4MI_ERR_INVALID_ARGUMENT, "line_stats: empty domain (%lld along axis %d)", (long long)domain[ax], ax);
    if (elem_size != 4 && elem_size != 8)
        return fail(GT4MI_ERR_UNSUPPORTED, "line_stats: item size %d is not supported (float32 or float64 fields)", elem_size);
    if (flags & ~GT4MI_STATS_DRY_RUN) return fail(GT4MI_ERR_INVALID_ARGUMENT, "line_stats: unknown bits in flags 0x%x", (unsigned)flags);
    const bool dry = (flags & GT4MI_STATS_DRY_RUN) != 0;
    if (int rc = stats_check_fields("line_stats", fields, others, nfields, domain, elem_size)) return rc;
    LinePlan plan(axis, elem_size);  // (every entry of the call, not only those of the first launch)
    for (int k = 0; k < nfields; ++k) plan.strict(fields[k]), plan.loose(stats_other(others, k));
    int lane_axis = 0;
    const int which = plan.path(domain, &lane_axis);
    const int order[3] = {axis, lane_axis, 3 - axis - lane_axis};
    const int64_t n = domain[axis], lines = domain[order[1]] * domain[order[2]], segments = cdiv(n, LINE_STATS_SEGMENT);
    if ((double)lines * (double)segments > (double)LINE_STATS_MAX_PAIRS)
        return fail(GT4MI_ERR_UNSUPPORTED, "line_stats: %lld lines of %lld segments are more than 2^30 (line, segment) pairs", (long long)lines,
                    (long long)segments);
    const int64_t needed = (int64_t)nfields * lines * segments * STATS_SLOTS * (int64_t)sizeof(double);
    const int64_t result_bytes = (int64_t)nfields * LINE_STATS_ROWS * lines * (int64_t)sizeof(double);
    if (workspace_needed) *workspace_needed = needed;
    if (path) *path = which;
    if (int rc = stats_check_buffers("line_stats", fields, others, nfields, domain, elem_size, workspace, workspace_bytes, needed, result,
                                     result_bytes, dry))
        return rc;
    if (launches) *launches = (int)cdiv(nfields, STATS_MAX_ENTRIES) + (segments > 1 ? 1 : 0);
    if (dry) return GT4MI_OK;
    LineStatsArgs a{};
    a.lines = lines;
    a.n = (int)n, a.nx = (int)domain[order[1]], a.ny = (int)domain[order[2]], a.segments = (int)segments;
    a.swap = order[1] > order[2];
    for (int first = 0; first < nfields; first += STATS_MAX_ENTRIES) {
        const int nf = nfields - first < STATS_MAX_ENTRIES ? nfields - first : STATS_MAX_ENTRIES;
        bool second = false;
        for (int k = 0; k < STATS_MAX_ENTRIES; ++k) {
            LineStatsEntry& e = a.e[k];
            e = LineStatsEntry{};
            if (k >= nf) continue;
            int64_t strides[3];
            e.a = origin_ptr(fields[first + k]);
            item_strides(fields[first + k], elem_size, strides, order);
            e.al = strides[0], e.ax = strides[1], e.ay = strides[2];
            if (const gt4mi_field* o = stats_other(others, first + k)) {
                e.b = origin_ptr(*o);
                item_strides(*o, elem_size, strides, order);
                e.bl = strides[0], e.bx = strides[1], e.by = strides[2];
                second = true;
            }
        }
        a.partials = static_cast<double*>(workspace) + (size_t)first * segments * STATS_SLOTS * lines;
        a.result = result + (size_t)first * LINE_STATS_ROWS * lines;
        with_item_type(elem_size, [&](auto t) { line_stats_launch<decltype(t)>(a, nf, which, second, stream); });
        GT4MI_HIP_CHECK(hipGetLastError());
    }
    if (segments > 1) {
        const dim3 grid((unsigned)cdiv(lines, LINE_STATS_BLOCK), STATS_SLOTS, (unsigned)nfields);
        hipLaunchKernelGGL(line_stats_finish_kernel, grid, dim3(LINE_STATS_BLOCK), 0, stream, static_cast<const double*>(workspace), result,
                           lines, a.segments, a.n, a.nx, a.ny, a.swap);
        GT4MI_HIP_CHECK(hipGetLastError());
    }
    return GT4MI_OK;
}

}  // namespace gt4mi
