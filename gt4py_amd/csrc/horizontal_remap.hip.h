// Conservative horizontal remapping between rectilinear grids: the cell means of up to 8 fields on one horizontal grid become cell
// means on another (coarser, finer or shifted), level by level, ONE launch; the geometry is two per-axis overlap tables that the
// host computes once (overlap_table below, no GPU) and every level of every field reads.
//
// NEW component, no reference counterpart: a GTScript destination point (i, j) reads sources at compile-time constant offsets
// from (i, j) only -- not 2*i, not a run-time range of source cells, not a source field of another horizontal shape.
//
// THE TABLE (include/gt4py_amd.h states it, tests/horizontal_remap_ref.py restates it in plain Python) is vertical_remap.hip.h's
// overlap loop per axis, float64, one rounding per operation, no FMA (-ffp-contract=off covers the host side too).  Source edges
// xs[0..ns], destination edges xd[0..nd], finite and strictly increasing (the host refuses anything else); the first source cell
// reaches to -inf, the last to +inf.  A source index k is kept across the destination cells and only grows.  For destination
// cell m, lo = xd[m], hi = xd[m+1], d = hi - lo:
//   advance   while k < ns-1 and not (xs[k+1] > lo): k += 1
//   terms     l = lo if k == 0 else (xs[k] if xs[k] > lo else lo);  r = hi if k == ns-1 else (xs[k+1] if xs[k+1] < hi else hi)
//             cell = k;  w = (r - l) / d;  h = xs[k+1] - xs[k];  xl = (l - xs[k]) / h;  xr = (r - xs[k]) / h;  c = 0.5 * (xl + xr) - 0.5
//             den = 0.5 h[k-1] + h[k] + 0.5 h[k+1] (left to right), 1.0 in the two end cells
//             stop after the term with k == ns-1 or xs[k+1] >= hi, else k += 1
//   ptr[m] .. ptr[m+1] are the terms of cell m; nd <= nnz <= ns + nd - 1.
//
// THE VALUES.  Everything is float64, items are widened exactly on load, the result is rounded once on store, each product is
// rounded before its addition.  For a destination point the outer loop runs over the J terms b in table order, the inner loop
// over the I terms a in table order, q[a, b] the item of the level at source cell (cell_i[a], cell_j[b]):
//   pcm   row_b = sum_a wi_a * q[a, b];  out = sum_b wj_b * row_b; the first term of each sum IS the accumulator (identical grids
//         return q bit for bit, -0.0 included)
//   plm   the same two sums over v = (q[a, b] + si * ci_a) + sj * cj_b; si / sj the limited centred slopes of source cell (a, b)
//         along I / J (remap_slope_den of vertical_remap.hip.h: g = (q+ - q-) / den * h, limited to 2|dl| and 2|dr|, 0 at
//         extrema), 0 when the cell is the first or last of that axis of the source box: nothing outside the box is read.  The
//         limiter acts per axis: conservative, exact for fields linear in x and y away from the end cells, not strictly monotone
//         in 2-d.
//
// NO ADDRESS DEPENDS ON FIELD DATA.  The only data that reaches an address are table integers: each ptr value is clamped to
// [0, nnz], a non-increasing pair is zero terms, every cell and cell +- 1 is clamped to the source box the host has checked; every
// store is at the thread's own (i, j, k) < extent.  A corrupt table gives unspecified values, never an address outside the boxes.
// Every loop counts table integers (clamped) or levels: none depends on field data, all end.
//
// ONE THREAD PER DESTINATION POINT, lanes along the destination I, a workgroup is 64 along I by 4 along J, every thread walks a
// chunk of HREMAP_CHUNK_K levels; tiles are flattened into blockIdx.x, descriptors are passed by value.  A wave is one
// destination row: its J terms are wave-uniform (the row index goes through readfirstlane, their loads are scalar), its I
// terms are per lane.  For an n:1 coarsening lane x reads source items n*x ... n*x + n - 1: the wave's loads of one I term have
// stride n, and its n terms together use every byte of the lines they touch.  The field loop is INSIDE the term loop: a term's
// cell, w, c, h, den are read once for all entries.  The kernel is instantiated for 1, 4 and 8 entries (NF): the field loop is
// unrolled NF times so that the descriptors are read at constant offsets of the argument block; the bits do not depend on NF.
// No LDS, no workspace, no scratch, no atomics, no ordering between workgroups: the host refuses a call in which a dst box meets
// a src box, a table array or another dst box, so nothing a launch reads is written by it.
#pragma once

#include <cmath>

#include "common.hip.h"
#include "field_args.hip.h"
#include "vertical_remap.hip.h"

namespace gt4mi {

// ---- the host-side table --------------------------------------------------------------------------------------------------------
inline int overlap_table(const double* xs, int ns, const double* xd, int nd, int32_t* ptr, int32_t* cell, double* w, double* h, double* c,
                         double* den, int capacity, int* nnz) {
    if (nnz) *nnz = 0;
    if (xs == nullptr || xd == nullptr)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "overlap_table: %s is null", xs == nullptr ? "src_edges" : "dst_edges");
    if (ptr == nullptr || cell == nullptr || w == nullptr || nnz == nullptr)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "overlap_table: %s is null", ptr == nullptr ? "ptr" : cell == nullptr ? "cell" : w == nullptr ? "w" : "nnz");
    const bool plm = h != nullptr || c != nullptr || den != nullptr;
    if (plm && (h == nullptr || c == nullptr || den == nullptr))
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "overlap_table: %s is null (h, c and den go together)", h == nullptr ? "h" : c == nullptr ? "c" : "den");
    if (ns < 1 || nd < 1 || (int64_t)ns + nd - 1 > INT32_MAX)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "overlap_table: ns = %d source and nd = %d destination cells, at least one each is needed", ns, nd);
    for (int side = 0; side < 2; ++side) {
        const double* x = side == 0 ? xs : xd;
        const int n = side == 0 ? ns : nd;
        for (int e = 0; e <= n; ++e) {
            if (!std::isfinite(x[e]))
                return fail(GT4MI_ERR_INVALID_ARGUMENT, "overlap_table: %s[%d] is not finite", side == 0 ? "src_edges" : "dst_edges", e);
            if (e > 0 && !(x[e] > x[e - 1]))
                return fail(GT4MI_ERR_INVALID_ARGUMENT, "overlap_table: %s are not strictly increasing at [%d]", side == 0 ? "src_edges" : "dst_edges", e);
        }
    }
    int k = 0, t = 0;
    for (int m = 0; m < nd; ++m) {
        const double lo = xd[m], hi = xd[m + 1];
        const double d = hi - lo;
        ptr[m] = t;
        while (k < ns - 1 && !(xs[k + 1] > lo)) ++k;
        for (;;) {
            if (t >= capacity)
                return fail(GT4MI_ERR_OUT_OF_BOUNDS, "overlap_table: capacity %d is too small (ns + nd - 1 = %d is always enough)", capacity, ns + nd - 1);
            const double l = k == 0 ? lo : (xs[k] > lo ? xs[k] : lo);
            const double r = k == ns - 1 ? hi : (xs[k + 1] < hi ? xs[k + 1] : hi);
            cell[t] = k;
            w[t] = (r - l) / d;
            if (plm) {
                const double hk = xs[k + 1] - xs[k];
                const double xl = (l - xs[k]) / hk, xr = (r - xs[k]) / hk;
                h[t] = hk;
                c[t] = 0.5 * (xl + xr) - 0.5;
                den[t] = k == 0 || k == ns - 1 ? 1.0 : 0.5 * (xs[k] - xs[k - 1]) + hk + 0.5 * (xs[k + 2] - xs[k + 1]);
            }
            ++t;
            if (k == ns - 1 || xs[k + 1] >= hi) break;
            ++k;
        }
    }
    ptr[nd] = t;
    *nnz = t;
    return GT4MI_OK;
}

// ---- the kernel -----------------------------------------------------------------------------------------------------------------
constexpr int HREMAP_TILE_I = 64, HREMAP_TILE_J = 4, HREMAP_CHUNK_K = 8;

struct HRemapArgs {
    PairEntry e[PAIR_MAX_FIELDS];
    gt4mi_overlap_axis ai, aj;  // (device pointers)
    int nk, nf;
    unsigned tiles_i, tiles_j;
};

__device__ __forceinline__ int hremap_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the terms [t0, t1) of destination cell m: table integers, clamped
__device__ __forceinline__ void hremap_terms(const gt4mi_overlap_axis& x, int m, int& t0, int& t1) {
    t0 = hremap_clamp(x.ptr[m], 0, x.nnz);
    t1 = hremap_clamp(x.ptr[m + 1], 0, x.nnz);
    if (t1 < t0) t1 = t0;
}

// T: item type of the fields, METHOD: GT4MI_HREMAP_*, NF: entries the field loop is unrolled for (a.nf <= NF)
template <typename T, int METHOD, int NF>
__global__ void __launch_bounds__(HREMAP_TILE_I * HREMAP_TILE_J)
horizontal_remap_kernel(const HRemapArgs a) {
    constexpr bool PLM = METHOD == GT4MI_HREMAP_PLM;
    unsigned tile = blockIdx.x;
    const unsigned ti = tile % a.tiles_i;
    tile /= a.tiles_i;
    const unsigned tj = tile % a.tiles_j, tk = tile / a.tiles_j;
    // (a wave is 64 lanes along I: its row is the same in every lane, and provably so for the compiler)
    const int row = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = (int)(ti * HREMAP_TILE_I + (threadIdx.x & 63u)), j = (int)(tj * HREMAP_TILE_J) + row;
    if (i >= a.ai.nd || j >= a.aj.nd) return;
    const int k0 = (int)tk * HREMAP_CHUNK_K, k1 = k0 + HREMAP_CHUNK_K < a.nk ? k0 + HREMAP_CHUNK_K : a.nk;
    const int nf = a.nf, last_i = a.ai.ns - 1, last_j = a.aj.ns - 1;
    int ta0, ta1, tb0, tb1;
    hremap_terms(a.ai, i, ta0, ta1);
    hremap_terms(a.aj, j, tb0, tb1);
    for (int k = k0; k < k1; ++k) {
        double out[NF];
#pragma unroll
        for (int n = 0; n < NF; ++n) out[n] = 0.0;
        for (int tb = tb0; tb < tb1; ++tb) {
            const int cb = hremap_clamp(a.aj.cell[tb], 0, last_j);
            const double wb = a.aj.w[tb];
            double cjb = 0.0, hb = 1.0, denb = 1.0;
            int cbm = cb, cbp = cb;
            bool inner_j = false;
            if constexpr (PLM) {
                cjb = a.aj.c[tb], hb = a.aj.h[tb], denb = a.aj.den[tb];
                cbm = cb > 0 ? cb - 1 : cb, cbp = cb < last_j ? cb + 1 : cb;
                inner_j = cb > 0 && cb < last_j;
            }
            double acc[NF];
#pragma unroll
            for (int n = 0; n < NF; ++n) acc[n] = 0.0;
            for (int ta = ta0; ta < ta1; ++ta) {
                const int ca = hremap_clamp(a.ai.cell[ta], 0, last_i);
                const double wa = a.ai.w[ta];
                double cia = 0.0, ha = 1.0, dena = 1.0;
                int cam = ca, cap = ca;
                bool inner_i = false;
                if constexpr (PLM) {
                    cia = a.ai.c[ta], ha = a.ai.h[ta], dena = a.ai.den[ta];
                    cam = ca > 0 ? ca - 1 : ca, cap = ca < last_i ? ca + 1 : ca;
                    inner_i = ca > 0 && ca < last_i;
                }
#pragma unroll
                for (int n = 0; n < NF; ++n) {
                    if (n >= nf) continue;
                    const PairEntry& e = a.e[n];
                    const T* const s = reinterpret_cast<const T*>(e.src) + k * e.s[2];
                    const double q = (double)s[ca * e.s[0] + cb * e.s[1]];
                    double v = q;
                    if constexpr (PLM) {
                        const double qim = (double)s[cam * e.s[0] + cb * e.s[1]], qip = (double)s[cap * e.s[0] + cb * e.s[1]];
                        const double qjm = (double)s[ca * e.s[0] + cbm * e.s[1]], qjp = (double)s[ca * e.s[0] + cbp * e.s[1]];
                        const double si = inner_i ? remap_slope_den(qim, q, qip, dena, ha) : 0.0;
                        const double sj = inner_j ? remap_slope_den(qjm, q, qjp, denb, hb) : 0.0;
                        v = (q + si * cia) + sj * cjb;
                    }
                    const double t = wa * v;
                    acc[n] = ta == ta0 ? t : acc[n] + t;
                }
            }
#pragma unroll
            for (int n = 0; n < NF; ++n) {
                const double t = wb * acc[n];
                out[n] = tb == tb0 ? t : out[n] + t;
            }
        }
#pragma unroll
        for (int n = 0; n < NF; ++n)
            if (n < nf) reinterpret_cast<T*>(a.e[n].dst)[k * a.e[n].d[2] + j * a.e[n].d[1] + i * a.e[n].d[0]] = (T)out[n];
    }
}

// ---- the entry ------------------------------------------------------------------------------------------------------------------
const BoxChecks HREMAP_CHECKS = {"horizontal_remap", "extent", "only a src may be broadcast", false, false};

template <typename T, int METHOD>
inline void hremap_launch(const HRemapArgs& a, int64_t blocks, hipStream_t stream) {
    with_pair_entries(a.nf, [&](auto nf) {
        hipLaunchKernelGGL((horizontal_remap_kernel<T, METHOD, decltype(nf)::value>), dim3((unsigned)blocks),
                           dim3(HREMAP_TILE_I * HREMAP_TILE_J), 0, stream, a);
    });
}

// one axis of a call: counts, pointers, alignment; its arrays' byte spans go to `spans` (for the overlap sweep)
inline int hremap_check_axis(int axis, const gt4mi_overlap_axis& x, bool plm, NamedSpan* spans, int* nspans) {
    static const char* const NAMES[2][7] = {{"axis_i", "axis_i ptr", "axis_i cell", "axis_i w", "axis_i h", "axis_i c", "axis_i den"},
                                            {"axis_j", "axis_j ptr", "axis_j cell", "axis_j w", "axis_j h", "axis_j c", "axis_j den"}};
    const char* const name = NAMES[axis][0];
    if (x.ns < 1 || x.nd < 1)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "horizontal_remap: %s has ns = %d source and nd = %d destination cells, at least one each is needed",
                    name, (int)x.ns, (int)x.nd);
    if (x.nnz < x.nd || (int64_t)x.nnz > (int64_t)x.ns + x.nd - 1)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "horizontal_remap: %s has nnz = %d terms, a table of ns = %d and nd = %d has %d to %lld", name,
                    (int)x.nnz, (int)x.ns, (int)x.nd, (int)x.nd, (long long)x.ns + x.nd - 1);
    const struct {
        const void* p;
        int64_t count;
        int size;
        bool read;  // by the kernel of this method
    } arrays[6] = {{x.ptr, (int64_t)x.nd + 1, 4, true}, {x.cell, x.nnz, 4, true}, {x.w, x.nnz, 8, true},
                   {x.h, x.nnz, 8, plm},                 {x.c, x.nnz, 8, plm},     {x.den, x.nnz, 8, plm}};
    for (int n = 0; n < 6; ++n) {
        if (!arrays[n].read) continue;
        const char* const what = NAMES[axis][n + 1];
        if (arrays[n].p == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "horizontal_remap: %s is null", what);
        const uintptr_t lo = reinterpret_cast<uintptr_t>(arrays[n].p);
        if (lo % (uintptr_t)arrays[n].size != 0) return fail(GT4MI_ERR_UNSUPPORTED, "horizontal_remap: %s is not aligned to its item size", what);
        spans[(*nspans)++] = NamedSpan{what, ByteSpan{lo, lo + (uintptr_t)(arrays[n].count * arrays[n].size)}};
    }
    return GT4MI_OK;
}

// every check, then (unless `flags` carries GT4MI_HREMAP_DRY_RUN) the launches
inline int horizontal_remap(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_overlap_axis* axis_i,
                            const gt4mi_overlap_axis* axis_j, int64_t nk, int elem_size, int method, int flags, hipStream_t stream,
                            int* launches) {
    if (launches) *launches = 0;
    if (dst == nullptr || src == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "horizontal_remap: %s is null", dst == nullptr ? "dst" : "src");
    if (axis_i == nullptr || axis_j == nullptr)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "horizontal_remap: %s is null", axis_i == nullptr ? "axis_i" : "axis_j");
    if (nfields < 1) return fail(GT4MI_ERR_INVALID_ARGUMENT, "horizontal_remap: nfields = %d, at least one pair is needed", nfields);
    if (nk < 1 || nk > INT32_MAX - HREMAP_CHUNK_K) return fail(GT4MI_ERR_INVALID_ARGUMENT, "horizontal_remap: nk = %lld levels, at least one is needed", (long long)nk);
    if (flags & ~GT4MI_HREMAP_DRY_RUN) return fail(GT4MI_ERR_INVALID_ARGUMENT, "horizontal_remap: unknown bits in flags 0x%x", (unsigned)flags);
    if (method != GT4MI_HREMAP_PCM && method != GT4MI_HREMAP_PLM)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "horizontal_remap: unknown method %d", method);
    if (elem_size != 4 && elem_size != 8)
        return fail(GT4MI_ERR_UNSUPPORTED, "horizontal_remap: field item size %d is not supported (float32 or float64)", elem_size);
    NamedSpan tables[12];
    int ntables = 0;
    if (int rc = hremap_check_axis(0, *axis_i, method == GT4MI_HREMAP_PLM, tables, &ntables)) return rc;
    if (int rc = hremap_check_axis(1, *axis_j, method == GT4MI_HREMAP_PLM, tables, &ntables)) return rc;
    const int64_t d_ext[3] = {axis_i->nd, axis_j->nd, nk}, s_ext[3] = {axis_i->ns, axis_j->ns, nk};
    for (int n = 0; n < nfields; ++n) {
        if (int rc = check_box_field(HREMAP_CHECKS, "dst", n, dst[n], d_ext, elem_size, true)) return rc;
        if (int rc = check_box_field(HREMAP_CHECKS, "src", n, src[n], s_ext, elem_size, false)) return rc;
    }
    if (int rc = check_pairs_disjoint("horizontal_remap", dst, src, nfields, d_ext, s_ext, elem_size, elem_size, nullptr, tables, ntables)) return rc;
    const int64_t tiles_i = cdiv(d_ext[0], HREMAP_TILE_I), tiles_j = cdiv(d_ext[1], HREMAP_TILE_J);
    const int64_t blocks = tiles_i * tiles_j * cdiv(nk, HREMAP_CHUNK_K);
    if (blocks > INT32_MAX) return fail(GT4MI_ERR_UNSUPPORTED, "horizontal_remap: too many points for one launch");
    if (launches) *launches = (int)cdiv(nfields, PAIR_MAX_FIELDS);
    if (flags & GT4MI_HREMAP_DRY_RUN) return GT4MI_OK;
    HRemapArgs a{};
    a.ai = *axis_i, a.aj = *axis_j;
    a.nk = (int)nk;
    a.tiles_i = (unsigned)tiles_i, a.tiles_j = (unsigned)tiles_j;
    int next = 0;
    while (next_pair_batch(a, dst, src, &next, nfields, elem_size)) {
        with_item_type(elem_size, [&](auto t) {
            using T = decltype(t);
            if (method == GT4MI_HREMAP_PLM) hremap_launch<T, GT4MI_HREMAP_PLM>(a, blocks, stream);
            else hremap_launch<T, GT4MI_HREMAP_PCM>(a, blocks, stream);
        });
        GT4MI_HIP_CHECK(hipGetLastError());
    }
    return GT4MI_OK;
}

}  // namespace gt4mi
