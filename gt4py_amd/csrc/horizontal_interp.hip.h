// Horizontal interpolation at run-time positions: every point (i, j, k) of the box of up to 8 destination fields receives the
// value of its source field at level k and the horizontal position (x_i, x_j) that two position fields hold for that point,
// ONE launch, the indices and weights of a point computed once for all its fields.
//
// NEW component, no reference counterpart: GTScript takes compile-time horizontal offsets only (only K may be indexed at run
// time), and gt4py.cartesian leaves a gather at data-dependent I / J positions -- the departure-point interpolation of a
// semi-Lagrangian step, sampling on a rotated, shifted or nested grid -- to fancy indexing on its numpy / cupy storages.
//
// THE ARITHMETIC CONTRACT (include/gt4py_amd.h states it, tests/horizontal_interp_ref.py restates it in plain Python).  All
// arithmetic is float64, one rounding per operation, no FMA (-ffp-contract=off and the pragma of common.hip.h); float32 items
// and positions are widened exactly on load and the result is rounded once on store.  Per axis, with n points in the domain,
// a reach of lo / hi ghost cells, xmin = -lo and xmax = n - 1 + hi as doubles:
//   1. p = the position item; in relative mode p = double(index) + p
//   2. x = xmin if p < xmin else (xmax if p > xmax else p)            NaN passes through, +-inf clamps
//   3. b = xmin if x != x else (int64) floor(x);  t = x - double(b)   (x is finite or NaN: the conversion is always defined)
//   4. every index a method uses is clamped on its own to [xmin, xmax]: edge replication
//   nearest         index floor(x + 0.5), clamped; the item's BIT PATTERN is moved (a NaN payload survives); a NaN position
//                   stores the canonical quiet NaN
//   linear          indices b, b+1; w0 = 1 - t, w1 = t; at row b_j  r0 = w0i*v00 + w1i*v10, at row b_j + 1  r1 likewise,
//                   out = w0j*r0 + w1j*r1 (each product rounded before its addition)
//   cubic           Lagrange on the nodes -1, 0, 1, 2: indices b-1, b, b+1, b+2; with a = t + 1, c = t - 1, d = t - 2
//                     w_-1 = -(((t*c)*d) / 6.0)   w_0 = ((a*c)*d) / 2.0   w_1 = -(((a*t)*d) / 2.0)   w_2 = ((a*t)*c) / 6.0
//                   the four row values r = ((w_-1*v_-1 + w_0*v_0) + w_1*v_1) + w_2*v_2 along I, the same expression along J
//                   over the four r gives out
//   cubic_monotone  the cubic out, then out = mn if out < mn else (mx if out > mx else out) with mn = min(min(c00, c10),
//                   min(c01, c11)), mx likewise, over the four corner items at the clamped indices b, b+1 of each axis;
//                   min(a, b) = b if b < a else a, max(a, b) = b if b > a else a; a NaN out stays NaN
// A weight of zero still multiplies (0 * inf = NaN at an integer position next to an infinity), -0.0 may come back as +0.0,
// a NaN position gives NaN in every field of that point and touches nothing else.  NO ADDRESS DEPENDS ON THE DATA BEYOND THE
// CLAMPED INTEGERS OF STEP 4: every load of a src is at a point of its readable box (the domain grown by the reach), which
// the host has checked to fit the array; every store is at the thread's own (i, j, k) < extent.
//
// ONE THREAD PER DESTINATION POINT, lanes along I (the contiguous axis of the storage layout), a workgroup is 64 along I by 4
// along J, and every thread walks a chunk of INTERP_CHUNK_K levels; tiles are flattened into blockIdx.x, descriptors are
// passed by value.  The field loop is INSIDE the point: clamp, floor, t, the indices and the two sets of weights are computed
// once and applied to every entry.  Where both position fields have K stride 0 (a Field[IJ]: 2-d flow) they are computed
// once per chunk of levels.  All loads of a point's stencil for an entry are issued before its first multiply; destination
// stores are full rows.  For smooth flow adjacent lanes read adjacent items (a stencil row is one or two lines); for
// scattered positions every lane reads lines of its own.  The kernel is instantiated for 1, 4 and 8 entries (NF): the field
// loop is unrolled NF times so that the descriptors are read at constant offsets of the argument block (a run-time index
// into it would send it to scratch); the bits do not depend on NF.  No LDS, no workspace, no scratch, no atomics, no ordering
// between workgroups: the host refuses a call in which a dst box meets a src readable box, a position field or another dst
// box, so nothing a launch reads is written by it.
#pragma once

#include "common.hip.h"
#include "field_args.hip.h"

namespace gt4mi {

constexpr int INTERP_TILE_I = 64, INTERP_TILE_J = 4, INTERP_CHUNK_K = 8;

struct InterpArgs {
    PairEntry e[PAIR_MAX_FIELDS];  // dst, src: domain point (0, 0, 0); a src is readable from -lo to n - 1 + hi along I and J
    SharedField pi, pj;            // domain point (0, 0, 0); stride 0 along K broadcasts a Field[IJ]
    int ni, nj, nk, nf;
    int lo_i, hi_i, lo_j, hi_j;
    unsigned tiles_i, tiles_j;
    int relative;
};

template <int METHOD>
struct InterpTaps {
    static constexpr int N = METHOD == GT4MI_INTERP_NEAREST ? 1 : (METHOD == GT4MI_INTERP_LINEAR ? 2 : 4);
};

__device__ __forceinline__ int64_t interp_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// steps 1-4 of the contract for one axis: the clamped indices and the weights of METHOD's taps; `nan` = the position is NaN
template <int METHOD>
__device__ __forceinline__ void interp_axis(double p, int index, bool relative, int lo, int last, int64_t (&idx)[InterpTaps<METHOD>::N],
                                            double (&w)[InterpTaps<METHOD>::N], bool& nan) {
    const int64_t imin = -(int64_t)lo, imax = last;
    const double xmin = (double)imin, xmax = (double)imax;
    if (relative) p = (double)index + p;
    const double x = p < xmin ? xmin : (p > xmax ? xmax : p);
    nan = x != x;
    if constexpr (METHOD == GT4MI_INTERP_NEAREST) {
        idx[0] = interp_clamp(nan ? imin : (int64_t)floor(x + 0.5), imin, imax);
        w[0] = 1.0;  // (unused: the item is moved)
    } else {
        const int64_t b = nan ? imin : (int64_t)floor(x);
        const double t = x - (double)b;
        if constexpr (METHOD == GT4MI_INTERP_LINEAR) {
            idx[0] = interp_clamp(b, imin, imax), idx[1] = interp_clamp(b + 1, imin, imax);
            w[0] = 1.0 - t, w[1] = t;
        } else {
            idx[0] = interp_clamp(b - 1, imin, imax), idx[1] = interp_clamp(b, imin, imax);
            idx[2] = interp_clamp(b + 1, imin, imax), idx[3] = interp_clamp(b + 2, imin, imax);
            const double a = t + 1.0, c = t - 1.0, d = t - 2.0;
            w[0] = -(((t * c) * d) / 6.0);
            w[1] = ((a * c) * d) / 2.0;
            w[2] = -(((a * t) * d) / 2.0);
            w[3] = ((a * t) * c) / 6.0;
        }
    }
}

// r = ((w0*v0 + w1*v1) + w2*v2) + w3*v3, every product rounded before its addition
template <int N>
__device__ __forceinline__ double interp_combine(const double (&w)[N], const double (&v)[N]) {
    double r = w[0] * v[0];
#pragma unroll
    for (int m = 1; m < N; ++m) r = r + w[m] * v[m];
    return r;
}

__device__ __forceinline__ double interp_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double interp_max(double a, double b) { return b > a ? b : a; }

template <typename T>
struct InterpBits;
template <>
struct InterpBits<float> {
    using type = uint32_t;
    static constexpr uint32_t QNAN = 0x7FC00000u;
};
template <>
struct InterpBits<double> {
    using type = uint64_t;
    static constexpr uint64_t QNAN = 0x7FF8000000000000ull;
};

// T: item type of the fields, P: of the positions, METHOD: GT4MI_INTERP_*, NF: entries the field loop is unrolled for (a.nf <= NF)
template <typename T, typename P, int METHOD, int NF>
__global__ void __launch_bounds__(INTERP_TILE_I * INTERP_TILE_J)
horizontal_interp_kernel(const InterpArgs a) {
    constexpr int N = InterpTaps<METHOD>::N;
    unsigned tile = blockIdx.x;
    const unsigned ti = tile % a.tiles_i;
    tile /= a.tiles_i;
    const unsigned tj = tile % a.tiles_j, tk = tile / a.tiles_j;
    const int i = (int)(ti * INTERP_TILE_I + (threadIdx.x & 63u)), j = (int)(tj * INTERP_TILE_J + (threadIdx.x >> 6));
    if (i >= a.ni || j >= a.nj) return;
    const int k0 = (int)tk * INTERP_CHUNK_K, k1 = k0 + INTERP_CHUNK_K < a.nk ? k0 + INTERP_CHUNK_K : a.nk;
    const P* const pi = reinterpret_cast<const P*>(a.pi.p) + i * a.pi.s[0] + j * a.pi.s[1];
    const P* const pj = reinterpret_cast<const P*>(a.pj.p) + i * a.pj.s[0] + j * a.pj.s[1];
    const bool per_level = a.pi.s[2] != 0 || a.pj.s[2] != 0;  // (the same in every thread of the launch)
    const bool relative = a.relative != 0;
    const int nf = a.nf;
    int64_t ii[N], jj[N];
    double wi[N], wj[N];
    bool nan = false;
    for (int k = k0; k < k1; ++k) {
        if (k == k0 || per_level) {
            bool nan_i, nan_j;
            interp_axis<METHOD>((double)pi[k * a.pi.s[2]], i, relative, a.lo_i, a.ni - 1 + a.hi_i, ii, wi, nan_i);
            interp_axis<METHOD>((double)pj[k * a.pj.s[2]], j, relative, a.lo_j, a.nj - 1 + a.hi_j, jj, wj, nan_j);
            nan = nan_i || nan_j;
        }
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            if (n >= nf) continue;
            const PairEntry& e = a.e[n];
            if constexpr (METHOD == GT4MI_INTERP_NEAREST) {
                using U = typename InterpBits<T>::type;
                const U v = reinterpret_cast<const U*>(e.src)[k * e.s[2] + jj[0] * e.s[1] + ii[0] * e.s[0]];
                reinterpret_cast<U*>(e.dst)[k * e.d[2] + j * e.d[1] + i * e.d[0]] = nan ? InterpBits<T>::QNAN : v;
            } else {
                const T* const s = reinterpret_cast<const T*>(e.src) + k * e.s[2];
                T raw[N][N];  // [row along J][tap along I]: every load of the entry before its first multiply
#pragma unroll
                for (int r = 0; r < N; ++r)
#pragma unroll
                    for (int c = 0; c < N; ++c) raw[r][c] = s[jj[r] * e.s[1] + ii[c] * e.s[0]];
                double rows[N];
#pragma unroll
                for (int r = 0; r < N; ++r) {
                    double v[N];
#pragma unroll
                    for (int c = 0; c < N; ++c) v[c] = (double)raw[r][c];
                    rows[r] = interp_combine<N>(wi, v);
                }
                double out = interp_combine<N>(wj, rows);
                if constexpr (METHOD == GT4MI_INTERP_CUBIC_MONOTONE) {
                    const double c00 = (double)raw[1][1], c10 = (double)raw[1][2], c01 = (double)raw[2][1], c11 = (double)raw[2][2];
                    const double mn = interp_min(interp_min(c00, c10), interp_min(c01, c11));
                    const double mx = interp_max(interp_max(c00, c10), interp_max(c01, c11));
                    out = out < mn ? mn : (out > mx ? mx : out);
                }
                reinterpret_cast<T*>(e.dst)[k * e.d[2] + j * e.d[1] + i * e.d[0]] = (T)out;
            }
        }
    }
}

const BoxChecks INTERP_CHECKS = {"horizontal_interp", "extent", "only a src or a position field may be broadcast", false, true};
constexpr int INTERP_POS_FREE_AXES = 4;  // a Field[IJ] of positions: stride 0 along K, one item for every level, no shape to check

template <typename T, typename P, int METHOD>
inline void interp_launch(const InterpArgs& a, int64_t blocks, hipStream_t stream) {
    with_pair_entries(a.nf, [&](auto nf) {
        hipLaunchKernelGGL((horizontal_interp_kernel<T, P, METHOD, decltype(nf)::value>), dim3((unsigned)blocks),
                           dim3(INTERP_TILE_I * INTERP_TILE_J), 0, stream, a);
    });
}

// every check, then (unless `flags` carries GT4MI_INTERP_DRY_RUN) the launches
inline int horizontal_interp(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* pos_i, const gt4mi_field* pos_j,
                             const int64_t extent[3], const int64_t reach[4], int elem_size, int pos_elem_size, int method, int flags,
                             hipStream_t stream, int* launches) {
    if (launches) *launches = 0;
    if (dst == nullptr || src == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "horizontal_interp: %s is null", dst == nullptr ? "dst" : "src");
    if (pos_i == nullptr || pos_j == nullptr)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "horizontal_interp: %s is null", pos_i == nullptr ? "pos_i" : "pos_j");
    if (extent == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "horizontal_interp: extent is null");
    if (reach == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "horizontal_interp: reach is null");
    if (nfields < 1) return fail(GT4MI_ERR_INVALID_ARGUMENT, "horizontal_interp: nfields = %d, at least one pair is needed", nfields);
    for (int ax = 0; ax < 3; ++ax)
        if (extent[ax] < 0 || extent[ax] > INT32_MAX)
            return fail(GT4MI_ERR_INVALID_ARGUMENT, "horizontal_interp: invalid extent %lld along axis %d", (long long)extent[ax], ax);
    if (flags & ~(GT4MI_INTERP_RELATIVE | GT4MI_INTERP_DRY_RUN))
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "horizontal_interp: unknown bits in flags 0x%x", (unsigned)flags);
    if (method != GT4MI_INTERP_NEAREST && method != GT4MI_INTERP_LINEAR && method != GT4MI_INTERP_CUBIC && method != GT4MI_INTERP_CUBIC_MONOTONE)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "horizontal_interp: unknown method %d", method);
    for (int side = 0; side < 4; ++side) {
        if (reach[side] < 0) return fail(GT4MI_ERR_INVALID_ARGUMENT, "horizontal_interp: negative reach %lld (entry %d)", (long long)reach[side], side);
        // (indices are 32-bit in the kernel: -lo - 1 ... n - 1 + hi + 2 must fit)
        if (reach[side] + extent[side / 2] > (int64_t)INT32_MAX - 8)
            return fail(GT4MI_ERR_UNSUPPORTED, "horizontal_interp: extent %lld + reach %lld is too large", (long long)extent[side / 2],
                        (long long)reach[side]);
    }
    if (elem_size != 4 && elem_size != 8)
        return fail(GT4MI_ERR_UNSUPPORTED, "horizontal_interp: field item size %d is not supported (float32 or float64)", elem_size);
    if (pos_elem_size != 4 && pos_elem_size != 8)
        return fail(GT4MI_ERR_UNSUPPORTED, "horizontal_interp: position item size %d is not supported (float32 or float64)", pos_elem_size);
    for (int n = 0; n < nfields; ++n) {
        if (int rc = check_box_field(INTERP_CHECKS, "dst", n, dst[n], extent, elem_size, true)) return rc;
        if (int rc = check_box_field(INTERP_CHECKS, "src", n, src[n], extent, elem_size, false, 0, reach)) return rc;  // (the readable box)
    }
    if (int rc = check_box_field(INTERP_CHECKS, "pos_i", 0, *pos_i, extent, pos_elem_size, false, INTERP_POS_FREE_AXES)) return rc;
    if (int rc = check_box_field(INTERP_CHECKS, "pos_j", 0, *pos_j, extent, pos_elem_size, false, INTERP_POS_FREE_AXES)) return rc;
    if (extent[0] == 0 || extent[1] == 0 || extent[2] == 0) return GT4MI_OK;
    const NamedSpan pos[2] = {{"pos_i", box_span(*pos_i, extent, pos_elem_size)}, {"pos_j", box_span(*pos_j, extent, pos_elem_size)}};
    if (int rc = check_pairs_disjoint("horizontal_interp", dst, src, nfields, extent, extent, elem_size, elem_size, reach, pos, 2)) return rc;
    const int64_t tiles_i = cdiv(extent[0], INTERP_TILE_I), tiles_j = cdiv(extent[1], INTERP_TILE_J);
    const int64_t blocks = tiles_i * tiles_j * cdiv(extent[2], INTERP_CHUNK_K);
    if (blocks > INT32_MAX) return fail(GT4MI_ERR_UNSUPPORTED, "horizontal_interp: too many points for one launch");
    if (launches) *launches = (int)cdiv(nfields, PAIR_MAX_FIELDS);
    if (flags & GT4MI_INTERP_DRY_RUN) return GT4MI_OK;
    InterpArgs a{};
    a.pi = shared_field(*pos_i, pos_elem_size), a.pj = shared_field(*pos_j, pos_elem_size);
    a.ni = (int)extent[0], a.nj = (int)extent[1], a.nk = (int)extent[2];
    a.lo_i = (int)reach[0], a.hi_i = (int)reach[1], a.lo_j = (int)reach[2], a.hi_j = (int)reach[3];
    a.tiles_i = (unsigned)tiles_i, a.tiles_j = (unsigned)tiles_j;
    a.relative = (flags & GT4MI_INTERP_RELATIVE) ? 1 : 0;
    int next = 0;
    while (next_pair_batch(a, dst, src, &next, nfields, elem_size)) {
        with_item_type(elem_size, [&](auto t) {
            with_item_type(pos_elem_size, [&](auto p) {
                using T = decltype(t);
                using P = decltype(p);
                if (method == GT4MI_INTERP_NEAREST) interp_launch<T, P, GT4MI_INTERP_NEAREST>(a, blocks, stream);
                else if (method == GT4MI_INTERP_LINEAR) interp_launch<T, P, GT4MI_INTERP_LINEAR>(a, blocks, stream);
                else if (method == GT4MI_INTERP_CUBIC) interp_launch<T, P, GT4MI_INTERP_CUBIC>(a, blocks, stream);
                else interp_launch<T, P, GT4MI_INTERP_CUBIC_MONOTONE>(a, blocks, stream);
            });
        });
        GT4MI_HIP_CHECK(hipGetLastError());
    }
    return GT4MI_OK;
}

}  // namespace gt4mi
