// Searches along I, J or K: for every line of the box along `axis`, WHERE it first crosses a level (a fractional position, the
// coordinate there and the number of crossings) or WHERE its maximum / minimum lies (the index, the coordinate and the value
// there), for up to 8 fields per launch that share the axis, the mode and optionally one coordinate field.
//
// NEW component.  The reference has no search: its users write a FORWARD stencil with a carried flag, one field per call and along K
// only, or chain cupy passes (a compare, `argmax` of the mask, two gathers, the arithmetic), each with fresh arrays.
//
// THE CONTRACT (include/gt4py_amd.h states it, tests/line_find_ref.py restates it in plain Python and in numpy).  All comparisons
// and arithmetic are IEEE float64 on the items converted exactly, one rounding per operation, no FMA.  y[q] is the line in scan
// order (GT4MI_FIND_REVERSE: from the far end), zc[q] the coord's item at the same place, idx(q) = q (reverse: n-1-q).
//   ARGMAX  the candidate starts as item 0; item q replaces it if the candidate is not a NaN and y[q] is a NaN or y[q] > candidate:
//           the first NaN met wins and stays, the first of equal items stays (-0.0 == +0.0): numpy.argmax of y.
//           position = double(idx(q*)), coord = zc[q*] (no coord: position), value = double(y[q*]).
//   ARGMIN  the same with <.
//   CROSSING of L: pair q in [0, n-1) rises if y[q] < L && y[q+1] >= L and falls if y[q] > L && y[q+1] <= L; `direction` selects
//           rising, falling or either; y[0] == L counts as found at q = 0 with t = 0 for every direction (position = double(idx(0)),
//           coord = zc[0]).  A comparison with a NaN is false.  crossings = the selected pairs of the whole line (+ 1 if y[0] == L).
//           At the first found pair t = (L - y[q]) / (y[q+1] - y[q]), position = double(q) + t (reverse: double(n-1-q) - t),
//           coord = zc[q] + t * (zc[q+1] - zc[q]) (no coord: position).  None: position = coord = missing, crossings = 0.
// A line's three result items depend on that line alone: not on layout, axis, path, the other fields of the call or the device.
//
// WHY IT ENDS AND STAYS IN ITS BOX WHATEVER THE DATA HOLDS: every loop counts to n (or to the items of a tile), which the host has
// checked against every field's shape; no loop bound and no address depends on field data, and there is no early exit (the count of
// crossings needs the whole line).  A lane owns its line from the first load to its three stores per field.
//
// THREE PATHS, chosen by the family's rule (line_geometry.hip.h: LinePlan; the fields strict, the coord loose) and reported as
// GT4MI_LINE_PATH_*:
//   LANES  lanes run along a unit-stride axis other than the line axis, a lane owns a line, every step is a coalesced row segment;
//          the loads of the NEXT FIND_AHEAD steps are issued before the compares of the steps in hand, the field loop sits inside
//          the step.  Carried per field: the item before (or the candidate), the found flag, position, coord, the count (or the
//          candidate's place); per lane: the coord's item before.
//   TILES  the LINE axis has unit stride: a workgroup IS one wave and moves tiles of 64 lines x one 128-byte run through LDS
//          (line_tile_move, the padded pitch); a lane scans its row of the tile (FIND_BURST items are read from LDS before the
//          first of them is compared), the carries cross the runs in registers, the coord's run is staged once per run for all
//          fields; a reverse search walks the runs from the far end.
//   ITEMS  anything else: the LANES kernel with one step in hand, uncoalesced: correct and slow.
// WHAT IS A TEMPLATE PARAMETER: T, the entries NF (1, 4, 8) and the look-ahead.  what, direction, reverse and the coord are UNIFORM
// branches.  Every field item is read once; the three float64 results per line and field are written once with plain vector
// stores.  No scratch, no atomics, no ordering between workgroups, no host synchronisation, no workspace.
// RESULT: result[((field * 3 + row) * nB + b) * nA + a], A < B the two other axes: the layout of line_stats' result.
#pragma once

#include "line_geometry.hip.h"

#pragma clang fp contract(off)

namespace gt4mi {

constexpr int FIND_BLOCK = 64;  // lanes (= lines) of a workgroup on the LANES / ITEMS paths: one wave, so that few lines still spread over the CUs
constexpr int FIND_AHEAD = 4;   // steps of one register buffer on the LANES path (two buffers)
constexpr int FIND_BURST = 8;   // items of a tile row that a lane reads from LDS in one go on the TILES path
constexpr int FIND_ROWS = GT4MI_FIND_ROWS;

// Every stride (ITEMS) is permuted by the host: [0] the line axis, [1] the lane axis, [2] the remaining axis.
struct FindArgs {
    SharedField e[PAIR_MAX_FIELDS];
    SharedField z;  // the coord (p == nullptr: none); stride 0 along the two other axes broadcasts a 1-d coord
    double level[PAIR_MAX_FIELDS];
    double missing;
    double* result;  // of the launch's first field
    int n, na, nb, nf, what, direction, reverse;
    int swap;        // the lane axis is B, not A: a line's place in a section is ib + nb * ia
};

// what a lane carries along its line for one field
template <typename T>
struct FindCarry {
    T keep;           // CROSSING: the item before; extrema: the candidate
    double pos, crd;  // CROSSING: of the first found pair; extrema: crd = the coord at the candidate
    int k;            // CROSSING: the crossings so far; extrema: the candidate's scan position
    bool found;
};

template <typename T>
__device__ __forceinline__ void find_init(FindCarry<T>& c) {
    c.keep = T(0), c.pos = 0.0, c.crd = 0.0, c.k = 0, c.found = false;
}

// One step of the contract: scan position q holds item y and coord z; zp is the coord at q - 1.
template <typename T>
__device__ __forceinline__ void find_step(FindCarry<T>& c, int q, T y, T z, T zp, const FindArgs& a, double level) {
    if (a.what != GT4MI_FIND_CROSSING) {
        const bool beyond = a.what == GT4MI_FIND_ARGMAX ? y > c.keep : y < c.keep;
        const bool take = q == 0 || (!(c.keep != c.keep) && (y != y || beyond));
        c.keep = take ? y : c.keep, c.k = take ? q : c.k, c.crd = take ? (double)z : c.crd;
        return;
    }
    const double before = (double)c.keep, here = (double)y;
    if (q == 0) {
        if (here == level) c.found = true, c.k = 1, c.pos = (double)(a.reverse ? a.n - 1 : 0), c.crd = (double)z;
    } else {
        const bool rise = before < level && here >= level, fall = before > level && here <= level;
        const bool hit = a.direction == GT4MI_FIND_ANY ? (rise || fall) : a.direction == GT4MI_FIND_RISING ? rise : fall;
        c.k += hit ? 1 : 0;
        if (hit && !c.found) {
            const double t = (level - before) / (here - before);
            c.found = true;
            c.pos = a.reverse ? (double)(a.n - q) - t : (double)(q - 1) + t;  // pair q - 1
            c.crd = (double)zp + t * ((double)z - (double)zp);
        }
    }
    c.keep = y;
}

// the three rows of one line and field: position, coord, extra
template <typename T>
__device__ __forceinline__ void find_store(const FindArgs& a, const FindCarry<T>& c, int f, int64_t at, int64_t lines) {
    const bool coord = a.z.p != nullptr;
    double pos, extra;
    bool have = true;
    if (a.what != GT4MI_FIND_CROSSING) pos = (double)(a.reverse ? a.n - 1 - c.k : c.k), extra = (double)c.keep;
    else pos = c.found ? c.pos : a.missing, extra = (double)c.k, have = c.found;
    double* const r = a.result + (size_t)f * FIND_ROWS * lines + at;
    r[0] = pos;
    r[(size_t)lines] = !have ? a.missing : coord ? c.crd : pos;
    r[(size_t)2 * lines] = extra;
}

// LANES (AHEAD = FIND_AHEAD) and ITEMS (AHEAD = 1).  NF: entries the kernel has registers for (a.nf <= NF).
template <typename T, int NF, int AHEAD>
__global__ void __launch_bounds__(FIND_BLOCK)
line_find_march_kernel(const FindArgs a) {
    const int64_t lines = (int64_t)a.na * a.nb;
    const LineLane l = line_lane(FIND_BLOCK, blockIdx.x, a.na, lines);
    if (!l.ok) return;
    const int64_t ia = l.ia(), ib = l.ib();
    const int n = a.n, nf = a.nf;
    const bool coord = a.z.p != nullptr;
    // scan position q is item first + dir * q of the line
    const int64_t first = a.reverse ? n - 1 : 0, dir = a.reverse ? -1 : 1;
    const T* const pz = coord ? reinterpret_cast<const T*>(a.z.p) + ia * a.z.s[1] + ib * a.z.s[2] + first * a.z.s[0] : nullptr;
    const int64_t sz = dir * a.z.s[0];
    const T* src[NF];
    int64_t ss[NF];
    FindCarry<T> carry[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        src[f] = nullptr, ss[f] = 0;
        find_init(carry[f]);
        if (f < nf) {
            src[f] = reinterpret_cast<const T*>(a.e[f].p) + ia * a.e[f].s[1] + ib * a.e[f].s[2] + first * a.e[f].s[0];
            ss[f] = dir * a.e[f].s[0];
        }
    }
    T vx[NF][AHEAD], vz[AHEAD], nx[NF][AHEAD], nz[AHEAD];
    auto load = [&](T (&x)[NF][AHEAD], T (&z)[AHEAD], int q0) {
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const int q = q0 + u;
            z[u] = T(0);
            if (coord && q < n) z[u] = pz[(int64_t)q * sz];
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                x[f][u] = T(0);
                if (f < nf && q < n) x[f][u] = src[f][(int64_t)q * ss[f]];
            }
        }
    };
    T zp = T(0);
    load(vx, vz, 0);
    for (int q0 = 0; q0 < n; q0 += AHEAD) {
        if (AHEAD > 1) load(nx, nz, q0 + AHEAD);
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const int q = q0 + u;
            if (q < n) {
#pragma unroll
                for (int f = 0; f < NF; ++f)
                    if (f < nf) find_step(carry[f], q, vx[f][u], vz[u], zp, a, a.level[f]);
                zp = vz[u];
            }
        }
        if (AHEAD > 1) {
#pragma unroll
            for (int u = 0; u < AHEAD; ++u) {
                vz[u] = nz[u];
#pragma unroll
                for (int f = 0; f < NF; ++f) vx[f][u] = nx[f][u];
            }
        } else {
            load(vx, vz, q0 + AHEAD);
        }
    }
    const int64_t at = a.swap ? ib + (int64_t)a.nb * ia : l.line;
#pragma unroll
    for (int f = 0; f < NF; ++f)
        if (f < nf) find_store(a, carry[f], f, at, lines);
}

// TILES: one wave = one workgroup = LINE_TILE_LINES consecutive lines; tile[l][r]: line l of the wave, item r of the run.
template <typename T, int NF>
__global__ void __launch_bounds__(LINE_TILE_LINES)
line_find_tile_kernel(const FindArgs a) {
    using L = LineTile<T>;
    constexpr int R = L::R;
    __shared__ T tz[LINE_TILE_LINES][L::PITCH];  // the coord's run
    __shared__ T tf[LINE_TILE_LINES][L::PITCH];  // the field in hand
    const int lane = (int)threadIdx.x;
    const int64_t lines = (int64_t)a.na * a.nb;
    const LineLane l = line_lane(LINE_TILE_LINES, blockIdx.x, a.na, lines);
    const bool ok = l.ok;
    const int64_t ia = l.ia(), ib = l.ib();
    const int n = a.n, nf = a.nf;
    const bool coord = a.z.p != nullptr, reverse = a.reverse != 0;
    const int64_t oz = ia * a.z.s[1] + ib * a.z.s[2];
    int64_t osrc[NF];
    FindCarry<T> carry[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        osrc[f] = 0;
        find_init(carry[f]);
        if (f < nf) osrc[f] = ia * a.e[f].s[1] + ib * a.e[f].s[2];
    }
    const int tiles = (n + R - 1) / R;
    T zrun = T(0);  // the coord's item in front of this run, in scan order
    for (int tt = 0; tt < tiles; ++tt) {
        const int t = reverse ? tiles - 1 - tt : tt;
        const int m0 = t * R;
        const int count = n - m0 < R ? n - m0 : R;  // items of this run
        if (coord) {
            __syncthreads();  // (the searches of the run before are done with tz)
            line_tile_move<T, true>(tz, reinterpret_cast<const T*>(a.z.p), oz, ok, m0, n);
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            if (f < nf) {
                __syncthreads();  // (tf is free: the search of the field before has read it)
                line_tile_move<T, true>(tf, reinterpret_cast<const T*>(a.e[f].p), osrc[f], ok, m0, n);
                __syncthreads();
                if (ok) {
                    // FIND_BURST items of the row, in scan order, are read from LDS before the first of them is compared
                    T zp = zrun;
                    const int q0 = reverse ? n - m0 - count : m0;  // the scan position of the run's first item in scan order
                    for (int i0 = 0; i0 < count; i0 += FIND_BURST) {
                        T y[FIND_BURST], z[FIND_BURST];
#pragma unroll
                        for (int u = 0; u < FIND_BURST; ++u) {
                            const int i = i0 + u < count ? i0 + u : count - 1;
                            const int r = reverse ? count - 1 - i : i;
                            y[u] = tf[lane][r];
                            z[u] = coord ? tz[lane][r] : T(0);
                        }
#pragma unroll
                        for (int u = 0; u < FIND_BURST; ++u) {
                            if (i0 + u < count) {
                                find_step(carry[f], q0 + i0 + u, y[u], z[u], zp, a, a.level[f]);
                                zp = z[u];
                            }
                        }
                    }
                }
            }
        }
        if (coord && ok) zrun = tz[lane][reverse ? 0 : count - 1];
    }
    if (!ok) return;
    const int64_t at = a.swap ? ib + (int64_t)a.nb * ia : l.line;
#pragma unroll
    for (int f = 0; f < NF; ++f)
        if (f < nf) find_store(a, carry[f], f, at, lines);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
const BoxChecks FIND_CHECKS = {"line_find", "extent", "only the coord may be broadcast", false, false};

template <typename T>
inline void find_launch(const FindArgs& a, const LineGrid& g, hipStream_t stream) {
    with_pair_entries(a.nf, [&](auto nf) {
        constexpr int NF = decltype(nf)::value;
        line_launch(g.path, g.lines, FIND_BLOCK, line_find_tile_kernel<T, NF>, line_find_march_kernel<T, NF, FIND_AHEAD>,
                    line_find_march_kernel<T, NF, 1>, a, stream);
    });
}

// every check, then (unless `flags` carries GT4MI_FIND_DRY_RUN) the launches
inline int line_find(const gt4mi_field* fields, int nfields, const gt4mi_field* coord, const int64_t extent[3], int axis, int elem_size, int what,
                     int direction, const double* level, double missing, double* result, int flags, hipStream_t stream, int* path,
                     int* launches) {
    if (launches) *launches = 0;
    if (path) *path = -1;
    const char* const entry = FIND_CHECKS.entry;
    if (fields == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: fields is null", entry);
    if (extent == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: extent is null", entry);
    if (nfields < 1) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: nfields = %d, at least one field is needed", entry, nfields);
    for (int ax = 0; ax < 3; ++ax)
        if (extent[ax] < 0 || extent[ax] > INT32_MAX)
            return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: invalid extent %lld along axis %d", entry, (long long)extent[ax], ax);
    if (axis < 0 || axis > 2) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: axis %d is not 0 (I), 1 (J) or 2 (K)", entry, axis);
    if (what != GT4MI_FIND_CROSSING && what != GT4MI_FIND_ARGMAX && what != GT4MI_FIND_ARGMIN)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: what %d is not GT4MI_FIND_CROSSING, GT4MI_FIND_ARGMAX or GT4MI_FIND_ARGMIN", entry, what);
    if (direction != GT4MI_FIND_ANY && direction != GT4MI_FIND_RISING && direction != GT4MI_FIND_FALLING)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: direction %d is not GT4MI_FIND_ANY, GT4MI_FIND_RISING or GT4MI_FIND_FALLING", entry, direction);
    if (flags & ~(GT4MI_FIND_REVERSE | GT4MI_FIND_DRY_RUN))
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: unknown bits in flags 0x%x", entry, (unsigned)flags);
    if (what != GT4MI_FIND_CROSSING && (level != nullptr || direction != GT4MI_FIND_ANY))
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: a level and a direction go with GT4MI_FIND_CROSSING only, what is %d", entry, what);
    if (what == GT4MI_FIND_CROSSING && level == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: level is null", entry);
    if (elem_size != 4 && elem_size != 8)
        return fail(GT4MI_ERR_UNSUPPORTED, "%s: item size %d is not supported (float32 or float64)", entry, elem_size);
    for (int k = 0; k < nfields; ++k)
        if (int rc = check_box_field(FIND_CHECKS, "field", k, fields[k], extent, elem_size, true)) return rc;
    if (coord != nullptr)  // a 1-d coord has stride 0 along the two other axes and no shape to check there
        if (int rc = check_box_field(FIND_CHECKS, "coord", 0, *coord, extent, elem_size, false, 7 & ~(1 << axis))) return rc;
    const bool dry = (flags & GT4MI_FIND_DRY_RUN) != 0;
    if (extent[0] == 0 || extent[1] == 0 || extent[2] == 0) return GT4MI_OK;
    LinePlan plan(axis, elem_size);  // (every field of the call, not only those of the first launch)
    for (int k = 0; k < nfields; ++k) plan.strict(fields[k]);
    plan.loose(coord);
    LineGrid g;
    if (int rc = line_grid(entry, plan, extent, LINE_TILE_LINES, &g)) return rc;
    // the result: there unless the call is a dry run, aligned to 8 bytes, clear of everything that is read
    if (!dry && result == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: result is null", entry);
    if (result != nullptr) {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(result);
        const ByteSpan span{lo, lo + (uintptr_t)nfields * FIND_ROWS * (uintptr_t)g.lines * sizeof(double)};
        if (lo % 8 != 0) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: result is not aligned to 8 bytes", entry);
        for (int k = 0; k < nfields; ++k)
            if (spans_overlap(span, box_span(fields[k], extent, elem_size)))
                return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: result overlaps field %d", entry, k);
        if (coord != nullptr && spans_overlap(span, box_span(*coord, extent, elem_size)))
            return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: result overlaps coord", entry);
    }
    if (path) *path = g.path;
    if (launches) *launches = (int)cdiv(nfields, PAIR_MAX_FIELDS);
    if (dry) return GT4MI_OK;
    FindArgs a{};
    if (coord != nullptr) a.z = shared_field(*coord, elem_size, g.order);
    a.n = (int)extent[axis], a.na = g.na, a.nb = g.nb;
    a.what = what, a.direction = direction, a.reverse = (flags & GT4MI_FIND_REVERSE) != 0, a.missing = missing;
    a.swap = g.order[1] > g.order[2];
    for (int first = 0; first < nfields; first += PAIR_MAX_FIELDS) {
        a.nf = nfields - first < PAIR_MAX_FIELDS ? nfields - first : PAIR_MAX_FIELDS;
        for (int k = 0; k < PAIR_MAX_FIELDS; ++k) {
            a.e[k] = k < a.nf ? shared_field(fields[first + k], elem_size, g.order) : SharedField{};
            a.level[k] = k < a.nf && level != nullptr ? level[first + k] : 0.0;
        }
        a.result = result + (size_t)first * FIND_ROWS * g.lines;
        with_item_type(elem_size, [&](auto t) { find_launch<decltype(t)>(a, g, stream); });
        GT4MI_HIP_CHECK(hipGetLastError());
    }
    return GT4MI_OK;
}

}  // namespace gt4mi
