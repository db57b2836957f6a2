// Prefix scans along I, J or K: for every line of the box along `axis`, the running sum (optionally of src * weight), maximum or
// minimum of the line so far, at every point of the line, for up to 8 (dst, src) pairs per launch.
//
// NEW component.  The reference has no scan: its users slice a storage and call numpy / cupy `cumsum` (`maximum.accumulate`) on the
// slice, one call and one fresh array per field, or write a FORWARD / BACKWARD stencil, which exists along K only and takes one field.
//
// THE ARITHMETIC CONTRACT (include/gt4py_amd.h states it, tests/line_scan_ref.py restates it in plain Python and in numpy).  T is the
// fields' type, A is double where GT4MI_SCAN_WIDE is set, op is SUM and T is float, else T.  x[0 .. n) is the line in scan order
// (GT4MI_SCAN_REVERSE: from the far end), w the weight in the same order.
//   SUM  t[m] = A(x[m]), or A(x[m]) * A(w[m]) rounded once in A;  s[0] = t[0] (NOT 0 + t[0]: a leading -0.0 stays -0.0);
//        s[m] = s[m-1] + t[m], rounded once in A, no FMA, strictly in this order.
//   MAX  s[0] = x[0];  s[m] = s[m-1] if (s[m-1] != s[m-1] or s[m-1] > x[m]) else x[m]: a NaN, once met, stays; on a tie (signed zeros
//        included) the newer item is taken; a select: bit patterns (NaN payloads) are moved, not computed.  Not fmax, which drops NaNs.
//   MIN  the same with <.
//   dst[m] = T(s[m]);  with GT4MI_SCAN_EXCLUSIVE dst[0] = the identity (+0.0, -inf, +inf) and dst[m] = T(s[m-1]).
// dst is written at the item's own index.  A line's bits depend on neither layout, axis, path, position in the call nor device; the
// float sum is numpy.cumsum along that axis bit for bit.
//
// WHY IT ENDS AND STAYS IN ITS BOX WHATEVER THE DATA HOLDS: every loop counts to n (or to the items of a tile), which the host has
// checked against every field's shape; no loop bound and no address depends on field data.  A lane owns its line from the first
// load to the last store, which is why dst[n] may BE src[n] (the same box): an item is stored after it was loaded, by the same lane.
//
// THREE PATHS, chosen by the family's rule (line_geometry.hip.h: LinePlan) and reported as GT4MI_SCAN_PATH_*:
//   LANES  an axis OTHER than the line axis has unit stride in every field (0 = broadcast in the weight): lanes run along it, a lane
//          owns a line, every step is a coalesced row segment.  The carries stay in registers, the field loop sits inside the step.
//          The loads of the NEXT SCAN_AHEAD steps are issued before the arithmetic and the stores of the SCAN_AHEAD steps in hand
//          (two register buffers): up to 2 x SCAN_AHEAD rows per field are in flight per lane.  Read once, written once.
//   TILES  the LINE axis has unit stride in every field: a workgroup IS one wave and moves tiles of 64 lines x one 128-byte run along
//          the line through LDS (line_geometry.hip.h's line_tile_move, field_copy.hip.h's padded pitch); a lane scans its run of the
//          tile sequentially, the carry stays in a register from tile to tile; a reverse scan walks the tiles from the far end.  The
//          tiles are private to the wave: the barriers are wave barriers.
//   ITEMS  anything else: one lane per line, item by item, uncoalesced: correct and slow (the LANES kernel, one step in hand).
// WHAT IS A TEMPLATE PARAMETER: T, the entries NF (1, 4, 8), the look-ahead, and A -- which differs from T only for float fields with
// WIDE and SUM.  op, exclusive, reverse and the weight are UNIFORM branches (every lane of a launch takes the same side): 27 kernels
// instead of 12 times as many.  No scratch, no atomics, no ordering between workgroups, no host synchronisation, no workspace.
#pragma once

#include <type_traits>

#include "line_geometry.hip.h"

#pragma clang fp contract(off)

namespace gt4mi {

constexpr int SCAN_BLOCK = 64;  // lanes (= lines) of a workgroup on the LANES / ITEMS paths: one wave, so that few lines still spread over the CUs
constexpr int SCAN_AHEAD = 4;   // steps of one register buffer on the LANES path (two buffers)

// Every stride (ITEMS) is permuted by the host: [0] the line axis, [1] the lane axis A, [2] the remaining axis B.
struct ScanArgs {
    PairEntry e[PAIR_MAX_FIELDS];
    SharedField w;  // the weight (p == nullptr: none); stride 0 along A / B broadcasts a 1-d weight
    int n, na, nb, nf, op, exclusive, reverse;
};

// `c ? a : b` on the bit patterns: a NaN's payload and a zero's sign are moved, never computed
template <typename T>
__device__ __forceinline__ T scan_pick(bool c, T a, T b) {
    using U = std::conditional_t<sizeof(T) == 8, uint64_t, uint32_t>;
    return __builtin_bit_cast(T, c ? __builtin_bit_cast(U, a) : __builtin_bit_cast(U, b));
}

template <typename A>
__device__ __forceinline__ A scan_identity(int op) {
    return op == GT4MI_SCAN_SUM ? A(0) : op == GT4MI_SCAN_MAX ? -__builtin_inf() : __builtin_inf();
}

// One step of the contract: the carry `s` takes item x (weight w where `weighted`); returns what dst gets.
template <typename T, typename A>
__device__ __forceinline__ T scan_step(A& s, T x, T w, bool first, int op, bool weighted, bool exclusive) {
    const A before = s;
    if (op == GT4MI_SCAN_SUM) {
        A t = A(x);
        if (weighted) t = t * A(w);
        s = first ? t : s + t;
    } else if constexpr (std::is_same_v<A, T>) {  // (a wide launch is a sum)
        const bool keep = !first && (s != s || (op == GT4MI_SCAN_MAX ? s > x : s < x));
        s = scan_pick(keep, s, x);
    }
    return T(exclusive ? before : s);
}

// LANES (AHEAD = SCAN_AHEAD) and ITEMS (AHEAD = 1).  NF: entries the kernel has registers for (a.nf <= NF).
template <typename T, typename A, int NF, int AHEAD>
__global__ void __launch_bounds__(SCAN_BLOCK)
line_scan_march_kernel(const ScanArgs a) {
    const LineLane l = line_lane(SCAN_BLOCK, blockIdx.x, a.na, (int64_t)a.na * a.nb);
    if (!l.ok) return;
    const int64_t ia = l.ia(), ib = l.ib();
    const int n = a.n, nf = a.nf, op = a.op;
    const bool weighted = a.w.p != nullptr, exclusive = a.exclusive != 0;
    // scan position m is item first + dir * m of the line
    const int64_t first = a.reverse ? n - 1 : 0, dir = a.reverse ? -1 : 1;
    const T* const pw = weighted ? reinterpret_cast<const T*>(a.w.p) + ia * a.w.s[1] + ib * a.w.s[2] + first * a.w.s[0] : nullptr;
    const int64_t sw = dir * a.w.s[0];
    const T* src[NF];
    T* dst[NF];
    int64_t ss[NF], sd[NF];
    A carry[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        src[f] = nullptr, dst[f] = nullptr, ss[f] = sd[f] = 0, carry[f] = scan_identity<A>(op);
        if (f < nf) {
            src[f] = reinterpret_cast<const T*>(a.e[f].src) + ia * a.e[f].s[1] + ib * a.e[f].s[2] + first * a.e[f].s[0];
            dst[f] = reinterpret_cast<T*>(a.e[f].dst) + ia * a.e[f].d[1] + ib * a.e[f].d[2] + first * a.e[f].d[0];
            ss[f] = dir * a.e[f].s[0], sd[f] = dir * a.e[f].d[0];
        }
    }
    T vx[NF][AHEAD], vw[AHEAD], nx[NF][AHEAD], nw[AHEAD];
    auto load = [&](T (&x)[NF][AHEAD], T (&w)[AHEAD], int m0) {
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const int m = m0 + u;
            w[u] = T(1);
            if (weighted && m < n) w[u] = pw[(int64_t)m * sw];
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                x[f][u] = T(0);
                if (f < nf && m < n) x[f][u] = src[f][(int64_t)m * ss[f]];
            }
        }
    };
    load(vx, vw, 0);
    for (int m0 = 0; m0 < n; m0 += AHEAD) {
        // the rows of the steps after these first: they lie beyond every item stored so far, also where dst is src
        if (AHEAD > 1) load(nx, nw, m0 + AHEAD);
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const int m = m0 + u;
            if (m < n) {
#pragma unroll
                for (int f = 0; f < NF; ++f)
                    if (f < nf) dst[f][(int64_t)m * sd[f]] = scan_step<T, A>(carry[f], vx[f][u], vw[u], m == 0, op, weighted, exclusive);
            }
        }
        if (AHEAD > 1) {
#pragma unroll
            for (int u = 0; u < AHEAD; ++u) {
                vw[u] = nw[u];
#pragma unroll
                for (int f = 0; f < NF; ++f) vx[f][u] = nx[f][u];
            }
        } else {
            load(vx, vw, m0 + AHEAD);
        }
    }
}

// TILES: one wave = one workgroup = LINE_TILE_LINES consecutive lines; tile[l][r]: line l of the wave, item r of the run.
template <typename T, typename A, int NF>
__global__ void __launch_bounds__(LINE_TILE_LINES)
line_scan_tile_kernel(const ScanArgs a) {
    using L = LineTile<T>;
    constexpr int R = L::R;
    __shared__ T tw[LINE_TILE_LINES][L::PITCH];  // the weight's run
    __shared__ T tf[LINE_TILE_LINES][L::PITCH];  // the field in hand
    const int lane = (int)threadIdx.x;
    const LineLane l = line_lane(LINE_TILE_LINES, blockIdx.x, a.na, (int64_t)a.na * a.nb);
    const bool ok = l.ok;
    const int64_t ia = l.ia(), ib = l.ib();
    const int n = a.n, nf = a.nf, op = a.op;
    const bool weighted = a.w.p != nullptr, exclusive = a.exclusive != 0, reverse = a.reverse != 0;
    const int64_t ow = ia * a.w.s[1] + ib * a.w.s[2];
    int64_t osrc[NF], odst[NF];
    A carry[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        osrc[f] = odst[f] = 0, carry[f] = scan_identity<A>(op);
        if (f < nf) osrc[f] = ia * a.e[f].s[1] + ib * a.e[f].s[2], odst[f] = ia * a.e[f].d[1] + ib * a.e[f].d[2];
    }
    const int tiles = (n + R - 1) / R;
    const int start = reverse ? n - 1 : 0;  // the item that is scan position 0
    for (int tt = 0; tt < tiles; ++tt) {
        const int t = reverse ? tiles - 1 - tt : tt;
        const int m0 = t * R;
        const int count = n - m0 < R ? n - m0 : R;  // items of this run
        if (weighted) {
            __syncthreads();  // (the scans of the tile before are done with tw)
            line_tile_move<T, true>(tw, reinterpret_cast<const T*>(a.w.p), ow, ok, m0, n);
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            if (f < nf) {
                __syncthreads();  // (tf is free: the stores of the field before have read it)
                line_tile_move<T, true>(tf, reinterpret_cast<const T*>(a.e[f].src), osrc[f], ok, m0, n);
                __syncthreads();
                if (ok) {
                    for (int q = 0; q < count; ++q) {
                        const int r = reverse ? count - 1 - q : q;
                        const T w = weighted ? tw[lane][r] : T(1);
                        tf[lane][r] = scan_step<T, A>(carry[f], tf[lane][r], w, m0 + r == start, op, weighted, exclusive);
                    }
                }
                __syncthreads();
                line_tile_move<T, false>(tf, reinterpret_cast<T*>(a.e[f].dst), odst[f], ok, m0, n);
            }
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
const BoxChecks SCAN_CHECKS = {"line_scan", "extent", "only a src or the weight may be broadcast", false, false};
const PairRoles SCAN_ROLES = {"dst", "src", true};  // a dst may BE its own src (the same box), and meet nothing else

template <typename T, typename A>
inline void scan_launch(const ScanArgs& a, const LineGrid& g, hipStream_t stream) {
    with_pair_entries(a.nf, [&](auto nf) {
        constexpr int NF = decltype(nf)::value;
        line_launch(g.path, g.lines, SCAN_BLOCK, line_scan_tile_kernel<T, A, NF>, line_scan_march_kernel<T, A, NF, SCAN_AHEAD>,
                    line_scan_march_kernel<T, A, NF, 1>, a, stream);
    });
}

// every check, then (unless `flags` carries GT4MI_SCAN_DRY_RUN) the launches
inline int line_scan(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* weight, const int64_t extent[3], int axis,
                     int elem_size, int op, int flags, hipStream_t stream, int* path, int* launches) {
    if (launches) *launches = 0;
    if (path) *path = -1;
    int weight_free = 0;  // a 1-d weight
    if (int rc = line_front(
            SCAN_CHECKS, SCAN_ROLES, dst, src, nfields, nullptr, extent, axis, elem_size,
            [&]() -> int {
                if (op != GT4MI_SCAN_SUM && op != GT4MI_SCAN_MAX && op != GT4MI_SCAN_MIN)
                    return fail(GT4MI_ERR_INVALID_ARGUMENT, "line_scan: op %d is not GT4MI_SCAN_SUM, GT4MI_SCAN_MAX or GT4MI_SCAN_MIN", op);
                const bool unknown = (flags & ~(GT4MI_SCAN_EXCLUSIVE | GT4MI_SCAN_REVERSE | GT4MI_SCAN_WIDE | GT4MI_SCAN_DRY_RUN)) != 0;
                return unknown ? fail(GT4MI_ERR_INVALID_ARGUMENT, "line_scan: unknown bits in flags 0x%x", (unsigned)flags) : GT4MI_OK;
            },
            [&]() -> int {
                if (weight == nullptr || op == GT4MI_SCAN_SUM) return GT4MI_OK;
                return fail(GT4MI_ERR_INVALID_ARGUMENT, "line_scan: a weight goes with GT4MI_SCAN_SUM only, op is %d", op);
            },
            &weight_free))
        return rc;
    const bool dry = (flags & GT4MI_SCAN_DRY_RUN) != 0;
    const bool wide = (flags & GT4MI_SCAN_WIDE) != 0 && op == GT4MI_SCAN_SUM && elem_size == 4;
    if (weight != nullptr)
        if (int rc = check_box_field(SCAN_CHECKS, "weight", 0, *weight, extent, elem_size, false, weight_free)) return rc;
    if (extent[0] == 0 || extent[1] == 0 || extent[2] == 0) return GT4MI_OK;
    NamedSpan shared[1] = {};
    if (weight != nullptr) shared[0] = NamedSpan{"weight", box_span(*weight, extent, elem_size)};
    if (int rc = check_pairs_disjoint("line_scan", dst, src, nfields, extent, extent, elem_size, elem_size, nullptr, shared, weight != nullptr ? 1 : 0,
                                      &SCAN_ROLES))
        return rc;
    LinePlan plan(axis, elem_size);
    for (int k = 0; k < nfields; ++k) plan.strict(dst[k]), plan.strict(src[k]);
    plan.loose(weight);
    LineGrid g;
    if (int rc = line_grid("line_scan", plan, extent, LINE_TILE_LINES, &g)) return rc;
    if (path) *path = g.path;
    if (launches) *launches = (int)cdiv(nfields, PAIR_MAX_FIELDS);
    if (dry) return GT4MI_OK;
    ScanArgs a{};
    if (weight != nullptr) a.w = shared_field(*weight, elem_size, g.order);
    a.n = (int)extent[axis], a.na = g.na, a.nb = g.nb;
    a.op = op, a.exclusive = (flags & GT4MI_SCAN_EXCLUSIVE) != 0, a.reverse = (flags & GT4MI_SCAN_REVERSE) != 0;
    int next = 0;
    while (next_pair_batch(a, dst, src, &next, nfields, elem_size, g.order)) {
        if (wide) scan_launch<float, double>(a, g, stream);
        else with_item_type(elem_size, [&](auto t) { scan_launch<decltype(t), decltype(t)>(a, g, stream); });
        GT4MI_HIP_CHECK(hipGetLastError());
    }
    return GT4MI_OK;
}

}  // namespace gt4mi
