// 3-D departure-point interpolation: every point (i, j, k) of the box of up to 8 destination fields receives the value of its
// source field at the position (x_i, x_j, x_k) that three position fields hold for that point, ONE launch, the three sets of
// indices and weights of a point computed once for all its fields.
//
// NEW component, no reference counterpart: GTScript takes compile-time horizontal offsets only, so the value of a field at a
// point that moved in all three directions -- the departure point of a semi-Lagrangian step -- cannot be written as a stencil.
// horizontal_interp gathers on a point's own level and vertical_interp in a point's own column; the two cannot be chained into
// this one, because the column that vertical_interp reads is the one at (i, j), not the one at the horizontal departure position.
//
// THE ARITHMETIC CONTRACT (include/gt4py_amd.h states it, tests/departure_interp_ref.py restates it in plain Python).  All
// arithmetic is float64, one rounding per operation, no FMA (-ffp-contract=off and the pragma of common.hip.h); float32 items
// and positions are widened exactly on load and the result is rounded once on store.
//   axes I, J       steps 1-4 of horizontal_interp unchanged (interp_axis): p (+ double(index) in relative mode), clamp to
//                   [-lo, n - 1 + hi], floor, t, every index clamped on its own
//   axis K          the same four steps with lo = hi = 0: K has no ghost levels, x_k is clamped to [0, nk - 1]
//   P(kk)           the PLANE VALUE of level kk: horizontal_interp's `out` for that level before any limiter -- the rows combined
//                   along I, the same expression along J
//   nearest         the level index is floor(x_k + 0.5), clamped; the BIT PATTERN of the item at the three nearest indices is
//                   moved; a NaN in any of the three positions stores the canonical quiet NaN
//   linear          levels b_k and b_k + 1, each clamped; out = w0k*P(b_k) + w1k*P(b_k + 1), w0k = 1 - t_k, w1k = t_k
//   cubic           the rule of vertical_interp, not edge replication in K: where 1 <= b_k <= nk - 3
//                     out = ((w_-1*P(b_k - 1) + w_0*P(b_k)) + w_1*P(b_k + 1)) + w_2*P(b_k + 2), the Lagrange weights of t_k;
//                   otherwise (the end intervals, and every interval when nk < 4) the linear formula along K over the two CUBIC
//                   plane values P(b_k), P(b_k + 1): only those two planes are loaded
//   cubic_monotone  the cubic out, then out = mn if out < mn else (mx if out > mx else out), mn / mx over the eight corner items
//                   at the clamped indices b, b + 1 of the three axes, folded as
//                     min(min(min(c000, c100), min(c010, c110)), min(min(c001, c101), min(c011, c111)))   index order (i, j, k)
//                   at every point, the end intervals of K included
// A weight of zero still multiplies, -0.0 may come back as +0.0, a NaN position gives NaN in every field of that point and touches
// nothing else.  NO ADDRESS DEPENDS ON THE DATA BEYOND THE CLAMPED INTEGERS: every load of a src is at a point of its readable box
// (the domain grown by the reach along I and J, levels 0 ... nk - 1), which the host has checked to fit the array; every store is
// at the thread's own (i, j, k) < extent.
//
// ONE THREAD PER DESTINATION POINT, lanes along I, a workgroup is 64 along I by 4 along J, and every thread walks a chunk of
// DEPARTURE_CHUNK_K levels; tiles are flattened into blockIdx.x, descriptors are passed by value, the kernel is instantiated for
// 1, 4 and 8 entries (NF) as horizontal_interp_kernel is.  The field loop is INSIDE the point.  Per entry the planes are handled
// ONE AFTER ANOTHER: all N x N loads of a plane are issued before its first multiply, the plane is reduced to P, P is folded into
// the K combination -- a cubic point never holds more than one plane's 16 raw items.  Where pos_i and pos_j both have K stride 0
// (Field[IJ]) their indices and weights are computed once per chunk of levels; pos_k is always IJK.  No LDS, no workspace, no
// scratch, no atomics, no ordering between workgroups: the host refuses a call in which a dst box meets a src readable box, a
// position field or another dst box.
#pragma once

#include "common.hip.h"
#include "field_args.hip.h"
#include "horizontal_interp.hip.h"  // interp_axis, interp_combine, interp_min, interp_max, InterpBits, InterpTaps

namespace gt4mi {

constexpr int DEPARTURE_TILE_I = 64, DEPARTURE_TILE_J = 4, DEPARTURE_CHUNK_K = 8;

struct DepartureArgs {
    PairEntry e[PAIR_MAX_FIELDS];  // dst, src: domain point (0, 0, 0); a src is readable from -lo to n - 1 + hi along I and J
    SharedField pi, pj, pk;        // domain point (0, 0, 0); stride 0 along K broadcasts a Field[IJ] (pi, pj only)
    int ni, nj, nk, nf;
    int lo_i, hi_i, lo_j, hi_j;
    unsigned tiles_i, tiles_j;
    int relative;
};

// P of one level (`s`: the entry's src at that level): every load before the first multiply, the rows along I, then along J.
// MONOTONE: the level's four corner items are folded into mn / mx (`first`: the point's first corner level).
template <typename T, int N, bool MONOTONE>
__device__ __forceinline__ double departure_plane(const T* s, const int64_t si, const int64_t sj, const int64_t (&ii)[N], const int64_t (&jj)[N],
                                                  const double (&wi)[N], const double (&wj)[N], bool corner, bool first, double& mn, double& mx) {
    T raw[N][N];  // [row along J][tap along I]
#pragma unroll
    for (int r = 0; r < N; ++r)
#pragma unroll
        for (int c = 0; c < N; ++c) raw[r][c] = s[jj[r] * sj + ii[c] * si];
    double rows[N];
#pragma unroll
    for (int r = 0; r < N; ++r) {
        double v[N];
#pragma unroll
        for (int c = 0; c < N; ++c) v[c] = (double)raw[r][c];
        rows[r] = interp_combine<N>(wi, v);
    }
    if constexpr (MONOTONE) {
        if (corner) {
            const double c00 = (double)raw[1][1], c10 = (double)raw[1][2], c01 = (double)raw[2][1], c11 = (double)raw[2][2];
            const double lo = interp_min(interp_min(c00, c10), interp_min(c01, c11));
            const double hi = interp_max(interp_max(c00, c10), interp_max(c01, c11));
            mn = first ? lo : interp_min(mn, lo);
            mx = first ? hi : interp_max(mx, hi);
        }
    }
    return interp_combine<N>(wj, rows);
}

// What a point needs along K for the methods that combine planes (all but nearest): levels b_k, b_k + 1 (each clamped) with the weights
// 1 - t_k, t_k -- linear, the end intervals of the cubics, the corners -- and, for the cubics, the four levels and Lagrange weights;
// `full`: the four-level formula applies, 1 <= b_k <= nk - 3, where b_k - 1 ... b_k + 2 are levels of the field.
struct DepartureLevels {
    int64_t kl[2], kc[4];
    double wl[2], wc[4];
    bool full;
    double w_lo, w_hi;  // the weights of P(b_k) and P(b_k + 1) in the formula that applies
};

template <bool CUBIC>
__device__ __forceinline__ void departure_levels(double xk, int k, bool relative, int nk, DepartureLevels& lv) {
    bool nan_k;
    interp_axis<GT4MI_INTERP_LINEAR>(xk, k, relative, 0, nk - 1, lv.kl, lv.wl, nan_k);
    lv.kc[0] = lv.kc[1] = lv.kc[2] = lv.kc[3] = 0;
    lv.wc[0] = lv.wc[1] = lv.wc[2] = lv.wc[3] = 0.0;
    lv.full = false;
    if constexpr (CUBIC) {
        interp_axis<GT4MI_INTERP_CUBIC>(xk, k, relative, 0, nk - 1, lv.kc, lv.wc, nan_k);
        lv.full = lv.kl[0] >= 1 && lv.kl[0] <= (int64_t)nk - 3;  // (x_k is clamped to [0, nk - 1]: kl[0] IS b_k)
    }
    lv.w_lo = lv.full ? lv.wc[1] : lv.wl[0], lv.w_hi = lv.full ? lv.wc[2] : lv.wl[1];
}

// One entry's value at a point (`s`: the entry's src at domain point (0, 0, 0), `st` its strides in items): the planes one after
// another, each reduced to P and folded into the K combination, then the limiter over the eight corners.
template <typename T, int METHOD>
__device__ __forceinline__ double departure_value(const T* s, const int64_t (&st)[3], const int64_t (&ii)[InterpTaps<METHOD>::N],
                                                  const int64_t (&jj)[InterpTaps<METHOD>::N], const double (&wi)[InterpTaps<METHOD>::N],
                                                  const double (&wj)[InterpTaps<METHOD>::N], const DepartureLevels& lv) {
    constexpr int N = InterpTaps<METHOD>::N;
    constexpr bool CUBIC = METHOD == GT4MI_INTERP_CUBIC || METHOD == GT4MI_INTERP_CUBIC_MONOTONE;
    constexpr bool MONOTONE = METHOD == GT4MI_INTERP_CUBIC_MONOTONE;
    double mn = 0.0, mx = 0.0, out = 0.0;
    if (CUBIC && lv.full) out = lv.wc[0] * departure_plane<T, N, MONOTONE>(s + lv.kc[0] * st[2], st[0], st[1], ii, jj, wi, wj, false, false, mn, mx);
    const double p_lo = departure_plane<T, N, MONOTONE>(s + lv.kl[0] * st[2], st[0], st[1], ii, jj, wi, wj, true, true, mn, mx);
    out = (CUBIC && lv.full) ? out + lv.w_lo * p_lo : lv.w_lo * p_lo;
    const double p_hi = departure_plane<T, N, MONOTONE>(s + lv.kl[1] * st[2], st[0], st[1], ii, jj, wi, wj, true, false, mn, mx);
    out = out + lv.w_hi * p_hi;
    if (CUBIC && lv.full) out = out + lv.wc[3] * departure_plane<T, N, MONOTONE>(s + lv.kc[3] * st[2], st[0], st[1], ii, jj, wi, wj, false, false, mn, mx);
    if constexpr (MONOTONE) out = out < mn ? mn : (out > mx ? mx : out);
    return out;
}

// T: item type of the fields, P: of the positions, METHOD: GT4MI_INTERP_*, NF: entries the field loop is unrolled for (a.nf <= NF)
template <typename T, typename P, int METHOD, int NF>
__global__ void __launch_bounds__(DEPARTURE_TILE_I * DEPARTURE_TILE_J)
departure_interp_kernel(const DepartureArgs a) {
    constexpr int N = InterpTaps<METHOD>::N;
    constexpr bool CUBIC = METHOD == GT4MI_INTERP_CUBIC || METHOD == GT4MI_INTERP_CUBIC_MONOTONE;
    constexpr bool MONOTONE = METHOD == GT4MI_INTERP_CUBIC_MONOTONE;
    unsigned tile = blockIdx.x;
    const unsigned ti = tile % a.tiles_i;
    tile /= a.tiles_i;
    const unsigned tj = tile % a.tiles_j, tk = tile / a.tiles_j;
    const int i = (int)(ti * DEPARTURE_TILE_I + (threadIdx.x & 63u)), j = (int)(tj * DEPARTURE_TILE_J + (threadIdx.x >> 6));
    if (i >= a.ni || j >= a.nj) return;
    const int k0 = (int)tk * DEPARTURE_CHUNK_K, k1 = k0 + DEPARTURE_CHUNK_K < a.nk ? k0 + DEPARTURE_CHUNK_K : a.nk;
    const P* const pi = reinterpret_cast<const P*>(a.pi.p) + i * a.pi.s[0] + j * a.pi.s[1];
    const P* const pj = reinterpret_cast<const P*>(a.pj.p) + i * a.pj.s[0] + j * a.pj.s[1];
    const P* const pk = reinterpret_cast<const P*>(a.pk.p) + i * a.pk.s[0] + j * a.pk.s[1];
    const bool per_level = a.pi.s[2] != 0 || a.pj.s[2] != 0;  // (the same in every thread of the launch)
    const bool relative = a.relative != 0;
    const int nf = a.nf, nk = a.nk;
    int64_t ii[N], jj[N];
    double wi[N], wj[N];
    bool nan_ij = false;
    for (int k = k0; k < k1; ++k) {
        if (k == k0 || per_level) {
            bool nan_i, nan_j;
            interp_axis<METHOD>((double)pi[k * a.pi.s[2]], i, relative, a.lo_i, a.ni - 1 + a.hi_i, ii, wi, nan_i);
            interp_axis<METHOD>((double)pj[k * a.pj.s[2]], j, relative, a.lo_j, a.nj - 1 + a.hi_j, jj, wj, nan_j);
            nan_ij = nan_i || nan_j;
        }
        const double xk = (double)pk[k * a.pk.s[2]];
        if constexpr (METHOD == GT4MI_INTERP_NEAREST) {
            using U = typename InterpBits<T>::type;
            int64_t kk[1];
            double wk[1];
            bool nan_k;
            interp_axis<METHOD>(xk, k, relative, 0, nk - 1, kk, wk, nan_k);
            const bool nan = nan_ij || nan_k;
#pragma unroll
            for (int n = 0; n < NF; ++n) {
                if (n >= nf) continue;
                const PairEntry& e = a.e[n];
                const U v = reinterpret_cast<const U*>(e.src)[kk[0] * e.s[2] + jj[0] * e.s[1] + ii[0] * e.s[0]];
                reinterpret_cast<U*>(e.dst)[k * e.d[2] + j * e.d[1] + i * e.d[0]] = nan ? InterpBits<T>::QNAN : v;
            }
        } else {
            DepartureLevels lv;
            departure_levels<CUBIC>(xk, k, relative, nk, lv);
#pragma unroll
            for (int n = 0; n < NF; ++n) {
                if (n >= nf) continue;
                const PairEntry& e = a.e[n];
                const double out = departure_value<T, METHOD>(reinterpret_cast<const T*>(e.src), e.s, ii, jj, wi, wj, lv);
                reinterpret_cast<T*>(e.dst)[k * e.d[2] + j * e.d[1] + i * e.d[0]] = (T)out;
            }
        }
    }
}

const BoxChecks DEPARTURE_CHECKS = {"departure_interp", "extent", "only a src or a position field may be broadcast", false, true};
constexpr int DEPARTURE_POS_FREE_AXES = 4;  // pos_i / pos_j as a Field[IJ]: stride 0 along K, one item for every level, no shape to check

template <typename T, typename P, int METHOD>
inline void departure_launch(const DepartureArgs& a, int64_t blocks, hipStream_t stream) {
    with_pair_entries(a.nf, [&](auto nf) {
        hipLaunchKernelGGL((departure_interp_kernel<T, P, METHOD, decltype(nf)::value>), dim3((unsigned)blocks),
                           dim3(DEPARTURE_TILE_I * DEPARTURE_TILE_J), 0, stream, a);
    });
}

// every check, then (unless `flags` carries GT4MI_INTERP_DRY_RUN) the launches
inline int departure_interp(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* pos_i, const gt4mi_field* pos_j,
                            const gt4mi_field* pos_k, const int64_t extent[3], const int64_t reach[4], int elem_size, int pos_elem_size,
                            int method, int flags, hipStream_t stream, int* launches) {
    if (launches) *launches = 0;
    if (dst == nullptr || src == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "departure_interp: %s is null", dst == nullptr ? "dst" : "src");
    if (pos_i == nullptr || pos_j == nullptr || pos_k == nullptr)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "departure_interp: %s is null", pos_i == nullptr ? "pos_i" : (pos_j == nullptr ? "pos_j" : "pos_k"));
    if (extent == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "departure_interp: extent is null");
    if (reach == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "departure_interp: reach is null");
    if (nfields < 1) return fail(GT4MI_ERR_INVALID_ARGUMENT, "departure_interp: nfields = %d, at least one pair is needed", nfields);
    for (int ax = 0; ax < 3; ++ax)
        if (extent[ax] < 0 || extent[ax] > INT32_MAX)
            return fail(GT4MI_ERR_INVALID_ARGUMENT, "departure_interp: invalid extent %lld along axis %d", (long long)extent[ax], ax);
    if (flags & ~(GT4MI_INTERP_RELATIVE | GT4MI_INTERP_DRY_RUN))
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "departure_interp: unknown bits in flags 0x%x", (unsigned)flags);
    if (method != GT4MI_INTERP_NEAREST && method != GT4MI_INTERP_LINEAR && method != GT4MI_INTERP_CUBIC && method != GT4MI_INTERP_CUBIC_MONOTONE)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "departure_interp: unknown method %d", method);
    for (int side = 0; side < 4; ++side) {
        if (reach[side] < 0) return fail(GT4MI_ERR_INVALID_ARGUMENT, "departure_interp: negative reach %lld (entry %d)", (long long)reach[side], side);
        // (indices are 32-bit in the kernel: -lo - 1 ... n - 1 + hi + 2 must fit)
        if (reach[side] + extent[side / 2] > (int64_t)INT32_MAX - 8)
            return fail(GT4MI_ERR_UNSUPPORTED, "departure_interp: extent %lld + reach %lld is too large", (long long)extent[side / 2],
                        (long long)reach[side]);
    }
    if (extent[2] > (int64_t)INT32_MAX - 8)  // (a chunk's last level + 1 is 32-bit in the kernel)
        return fail(GT4MI_ERR_UNSUPPORTED, "departure_interp: extent %lld along axis 2 is too large", (long long)extent[2]);
    if (elem_size != 4 && elem_size != 8)
        return fail(GT4MI_ERR_UNSUPPORTED, "departure_interp: field item size %d is not supported (float32 or float64)", elem_size);
    if (pos_elem_size != 4 && pos_elem_size != 8)
        return fail(GT4MI_ERR_UNSUPPORTED, "departure_interp: position item size %d is not supported (float32 or float64)", pos_elem_size);
    for (int n = 0; n < nfields; ++n) {
        if (int rc = check_box_field(DEPARTURE_CHECKS, "dst", n, dst[n], extent, elem_size, true)) return rc;
        if (int rc = check_box_field(DEPARTURE_CHECKS, "src", n, src[n], extent, elem_size, false, 0, reach)) return rc;  // (the readable box)
    }
    if (int rc = check_box_field(DEPARTURE_CHECKS, "pos_i", 0, *pos_i, extent, pos_elem_size, false, DEPARTURE_POS_FREE_AXES)) return rc;
    if (int rc = check_box_field(DEPARTURE_CHECKS, "pos_j", 0, *pos_j, extent, pos_elem_size, false, DEPARTURE_POS_FREE_AXES)) return rc;
    if (int rc = check_box_field(DEPARTURE_CHECKS, "pos_k", 0, *pos_k, extent, pos_elem_size, false)) return rc;  // (always a full IJK box)
    if (extent[0] == 0 || extent[1] == 0 || extent[2] == 0) return GT4MI_OK;
    // (a point reads any level of its src: the readable box is the domain grown by the reach over ALL levels, which is the extent)
    const NamedSpan pos[3] = {{"pos_i", box_span(*pos_i, extent, pos_elem_size)},
                              {"pos_j", box_span(*pos_j, extent, pos_elem_size)},
                              {"pos_k", box_span(*pos_k, extent, pos_elem_size)}};
    if (int rc = check_pairs_disjoint("departure_interp", dst, src, nfields, extent, extent, elem_size, elem_size, reach, pos, 3)) return rc;
    const int64_t tiles_i = cdiv(extent[0], DEPARTURE_TILE_I), tiles_j = cdiv(extent[1], DEPARTURE_TILE_J);
    const int64_t blocks = tiles_i * tiles_j * cdiv(extent[2], DEPARTURE_CHUNK_K);
    if (blocks > INT32_MAX) return fail(GT4MI_ERR_UNSUPPORTED, "departure_interp: too many points for one launch");
    if (launches) *launches = (int)cdiv(nfields, PAIR_MAX_FIELDS);
    if (flags & GT4MI_INTERP_DRY_RUN) return GT4MI_OK;
    DepartureArgs a{};
    a.pi = shared_field(*pos_i, pos_elem_size), a.pj = shared_field(*pos_j, pos_elem_size), a.pk = shared_field(*pos_k, pos_elem_size);
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
                if (method == GT4MI_INTERP_NEAREST) departure_launch<T, P, GT4MI_INTERP_NEAREST>(a, blocks, stream);
                else if (method == GT4MI_INTERP_LINEAR) departure_launch<T, P, GT4MI_INTERP_LINEAR>(a, blocks, stream);
                else if (method == GT4MI_INTERP_CUBIC) departure_launch<T, P, GT4MI_INTERP_CUBIC>(a, blocks, stream);
                else departure_launch<T, P, GT4MI_INTERP_CUBIC_MONOTONE>(a, blocks, stream);
            });
        });
        GT4MI_HIP_CHECK(hipGetLastError());
    }
    return GT4MI_OK;
}

}  // namespace gt4mi
