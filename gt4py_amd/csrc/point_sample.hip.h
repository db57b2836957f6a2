// Sampling at a list of run-time positions: every point p of a list of `npoints` positions receives, in up to 8 result arrays, the
// value of their source fields at (pos_i[p], pos_j[p]) on every level (COLUMN mode: a sounding per point, a curtain per path) or at
// the 3-d position (pos_i[p], pos_j[p], pos_k[p]) (POINT mode: the values along a track), ONE launch, the indices and weights of a
// point computed once for all its fields.
//
// NEW component, no reference counterpart: GTScript takes compile-time horizontal offsets only and writes fields of the shape it
// reads; a result whose first axis is "the point" cannot be a stencil's output.  horizontal_interp and departure_interp hold the
// arithmetic but write one value per point of the compute domain, at positions that are fields over that domain.
//
// THE ARITHMETIC CONTRACT is that of the two interpolators in absolute mode (include/gt4py_amd.h states it,
// tests/point_sample_ref.py restates it through tests/horizontal_interp_ref.py and tests/departure_interp_ref.py), and the code IS
// theirs: interp_axis for steps 1-4 of every axis, departure_plane for the value on one level (horizontal_interp's `out`, with the
// four corner items of its limiter), departure_levels / departure_value for the combination along K with its end-interval rule.
//   column mode   dst(p, k) = horizontal_interp's value of src at level k and (pos_i[p], pos_j[p])
//   point mode    dst(p)    = departure_interp's value of src at (pos_i[p], pos_j[p], pos_k[p]); K has no ghost levels
//   fill          with GT4MI_SAMPLE_FILL a point any of whose position items satisfies p < xmin, p > xmax or p != p (xmin = -lo,
//                 xmax = n - 1 + hi as doubles; along K 0 and nk - 1) receives (T)fill_value -- rounded once -- in every field and
//                 every level; every other point receives exactly the bits of the clamp mode
// NO ADDRESS DEPENDS ON THE DATA BEYOND THE CLAMPED INTEGERS: every load of a src is at a point of its readable box (the domain
// grown by the reach along I and J, levels 0 ... nk - 1), a filled point included (its loads are made and dropped); every store is
// at the lane's own (p, k) with p < npoints and k < nk; the position arrays are read at p < npoints.  The host has checked all
// three boxes against their arrays.
//
// COLUMN MODE: ONE LANE PER (POINT, LEVEL), the level fastest across lanes -- a wave's stores into a K-contiguous result are
// contiguous, and its loads from a K-contiguous source are too; the lanes of one point read the same two position items (one
// request) and repeat the same index arithmetic, which gives the same bits.  POINT MODE: ONE LANE PER POINT.  Lanes are flattened
// into blockIdx.x, 256 to a workgroup; descriptors are passed by value; the kernel is instantiated for 1, 4 and 8 entries (NF) as
// the interpolators' are, the field loop INSIDE the point.  No LDS, no workspace, no scratch, no atomics, no ordering between
// workgroups: the host refuses a call in which the bytes of a dst meet a src readable box, a position array or another dst.
#pragma once

#include "common.hip.h"
#include "departure_interp.hip.h"  // departure_plane, departure_levels, departure_value (and horizontal_interp.hip.h: interp_axis, InterpBits)
#include "field_args.hip.h"

namespace gt4mi {

constexpr int POINT_SAMPLE_BLOCK = 256;

struct PointSampleArgs {
    PairEntry e[PAIR_MAX_FIELDS];  // dst: the item of (point 0, level 0), d[0] / d[1] the point / level stride; src: domain point (0, 0, 0)
    SharedField pi, pj, pk;        // item of point 0, s[0] the point stride; pk is unused in column mode
    uint64_t lanes;                // column mode: npoints * nk; point mode: npoints
    int ni, nj, nk, nf;
    int lo_i, hi_i, lo_j, hi_j;
    int fill;                      // GT4MI_SAMPLE_FILL is set
    double fill_value;
};

// the fill rule for one position item: outside [xmin, xmax] or NaN (+-inf is outside)
__device__ __forceinline__ bool point_sample_outside(double p, int lo, int last) {
    const double xmin = (double)(-(int64_t)lo), xmax = (double)(int64_t)last;
    return p < xmin || p > xmax || p != p;
}

// T: item type of the fields, P: of the positions, METHOD: GT4MI_INTERP_*, NF: entries the field loop is unrolled for (a.nf <= NF),
// COLUMN: column mode (every level at the point's horizontal position) or point mode (the 3-d position)
template <typename T, typename P, int METHOD, int NF, bool COLUMN>
__global__ void __launch_bounds__(POINT_SAMPLE_BLOCK)
point_sample_kernel(const PointSampleArgs a) {
    constexpr int N = InterpTaps<METHOD>::N;
    constexpr bool CUBIC = METHOD == GT4MI_INTERP_CUBIC || METHOD == GT4MI_INTERP_CUBIC_MONOTONE;
    constexpr bool MONOTONE = METHOD == GT4MI_INTERP_CUBIC_MONOTONE;
    using U = typename InterpBits<T>::type;
    const uint64_t lane = (uint64_t)blockIdx.x * POINT_SAMPLE_BLOCK + threadIdx.x;
    if (lane >= a.lanes) return;
    const int nf = a.nf, nk = a.nk;
    const int64_t p = COLUMN ? (int64_t)(lane / (uint64_t)nk) : (int64_t)lane;
    const int64_t k = COLUMN ? (int64_t)(lane - (uint64_t)p * (uint64_t)nk) : 0;
    const double xi = (double)reinterpret_cast<const P*>(a.pi.p)[p * a.pi.s[0]];
    const double xj = (double)reinterpret_cast<const P*>(a.pj.p)[p * a.pj.s[0]];
    int64_t ii[N], jj[N];
    double wi[N], wj[N];
    bool nan_i, nan_j;
    interp_axis<METHOD>(xi, 0, false, a.lo_i, a.ni - 1 + a.hi_i, ii, wi, nan_i);
    interp_axis<METHOD>(xj, 0, false, a.lo_j, a.nj - 1 + a.hi_j, jj, wj, nan_j);
    bool filled = point_sample_outside(xi, a.lo_i, a.ni - 1 + a.hi_i) || point_sample_outside(xj, a.lo_j, a.nj - 1 + a.hi_j);
    const T fill_item = (T)a.fill_value;  // rounded once
    U fill_bits;
    __builtin_memcpy(&fill_bits, &fill_item, sizeof(U));
    if constexpr (COLUMN) {
        filled = filled && a.fill != 0;
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            if (n >= nf) continue;
            const PairEntry& e = a.e[n];
            const int64_t at = p * e.d[0] + k * e.d[1];
            if constexpr (METHOD == GT4MI_INTERP_NEAREST) {
                const U v = reinterpret_cast<const U*>(e.src)[k * e.s[2] + jj[0] * e.s[1] + ii[0] * e.s[0]];
                reinterpret_cast<U*>(e.dst)[at] = filled ? fill_bits : ((nan_i || nan_j) ? InterpBits<T>::QNAN : v);
            } else {
                double mn = 0.0, mx = 0.0;  // (the four corners of the level: horizontal_interp's limiter)
                double out = departure_plane<T, N, MONOTONE>(reinterpret_cast<const T*>(e.src) + k * e.s[2], e.s[0], e.s[1], ii, jj, wi, wj, true,
                                                             true, mn, mx);
                if constexpr (MONOTONE) out = out < mn ? mn : (out > mx ? mx : out);
                reinterpret_cast<T*>(e.dst)[at] = filled ? fill_item : (T)out;
            }
        }
    } else {
        const double xk = (double)reinterpret_cast<const P*>(a.pk.p)[p * a.pk.s[0]];
        filled = (filled || point_sample_outside(xk, 0, nk - 1)) && a.fill != 0;
        if constexpr (METHOD == GT4MI_INTERP_NEAREST) {
            int64_t kk[1];
            double wk[1];
            bool nan_k;
            interp_axis<METHOD>(xk, 0, false, 0, nk - 1, kk, wk, nan_k);
            const bool nan = nan_i || nan_j || nan_k;
#pragma unroll
            for (int n = 0; n < NF; ++n) {
                if (n >= nf) continue;
                const PairEntry& e = a.e[n];
                const U v = reinterpret_cast<const U*>(e.src)[kk[0] * e.s[2] + jj[0] * e.s[1] + ii[0] * e.s[0]];
                reinterpret_cast<U*>(e.dst)[p * e.d[0]] = filled ? fill_bits : (nan ? InterpBits<T>::QNAN : v);
            }
        } else {
            DepartureLevels lv;
            departure_levels<CUBIC>(xk, 0, false, nk, lv);
#pragma unroll
            for (int n = 0; n < NF; ++n) {
                if (n >= nf) continue;
                const PairEntry& e = a.e[n];
                const double out = departure_value<T, METHOD>(reinterpret_cast<const T*>(e.src), e.s, ii, jj, wi, wj, lv);
                reinterpret_cast<T*>(e.dst)[p * e.d[0]] = filled ? fill_item : (T)out;
            }
        }
    }
}

const BoxChecks POINT_SAMPLE_CHECKS = {"point_sample", "extent", "only a src or a position array may be broadcast", false, true};

template <typename T, typename P, int METHOD, bool COLUMN>
inline void point_sample_launch(const PointSampleArgs& a, int64_t blocks, hipStream_t stream) {
    with_pair_entries(a.nf, [&](auto nf) {
        hipLaunchKernelGGL((point_sample_kernel<T, P, METHOD, decltype(nf)::value, COLUMN>), dim3((unsigned)blocks), dim3(POINT_SAMPLE_BLOCK), 0,
                           stream, a);
    });
}

template <typename T, typename P, bool COLUMN>
inline void point_sample_method(const PointSampleArgs& a, int method, int64_t blocks, hipStream_t stream) {
    if (method == GT4MI_INTERP_NEAREST) point_sample_launch<T, P, GT4MI_INTERP_NEAREST, COLUMN>(a, blocks, stream);
    else if (method == GT4MI_INTERP_LINEAR) point_sample_launch<T, P, GT4MI_INTERP_LINEAR, COLUMN>(a, blocks, stream);
    else if (method == GT4MI_INTERP_CUBIC) point_sample_launch<T, P, GT4MI_INTERP_CUBIC, COLUMN>(a, blocks, stream);
    else point_sample_launch<T, P, GT4MI_INTERP_CUBIC_MONOTONE, COLUMN>(a, blocks, stream);
}

// every check, then (unless `flags` carries GT4MI_SAMPLE_DRY_RUN) the launches
inline int point_sample(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* pos_i, const gt4mi_field* pos_j,
                        const gt4mi_field* pos_k, int64_t npoints, const int64_t extent[3], const int64_t reach[4], int elem_size,
                        int pos_elem_size, int method, int flags, double fill_value, hipStream_t stream, int* launches) {
    if (launches) *launches = 0;
    if (dst == nullptr || src == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "point_sample: %s is null", dst == nullptr ? "dst" : "src");
    if (pos_i == nullptr || pos_j == nullptr)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "point_sample: %s is null", pos_i == nullptr ? "pos_i" : "pos_j");
    if (extent == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "point_sample: extent is null");
    if (reach == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "point_sample: reach is null");
    if (nfields < 1) return fail(GT4MI_ERR_INVALID_ARGUMENT, "point_sample: nfields = %d, at least one pair is needed", nfields);
    if (npoints < 0 || npoints > INT32_MAX) return fail(GT4MI_ERR_INVALID_ARGUMENT, "point_sample: invalid npoints %lld", (long long)npoints);
    for (int ax = 0; ax < 3; ++ax)
        if (extent[ax] < 0 || extent[ax] > INT32_MAX)
            return fail(GT4MI_ERR_INVALID_ARGUMENT, "point_sample: invalid extent %lld along axis %d", (long long)extent[ax], ax);
    if (flags & ~(GT4MI_SAMPLE_FILL | GT4MI_SAMPLE_DRY_RUN))
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "point_sample: unknown bits in flags 0x%x", (unsigned)flags);
    if (method != GT4MI_INTERP_NEAREST && method != GT4MI_INTERP_LINEAR && method != GT4MI_INTERP_CUBIC && method != GT4MI_INTERP_CUBIC_MONOTONE)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "point_sample: unknown method %d", method);
    for (int side = 0; side < 4; ++side) {
        if (reach[side] < 0) return fail(GT4MI_ERR_INVALID_ARGUMENT, "point_sample: negative reach %lld (entry %d)", (long long)reach[side], side);
        // (indices are 32-bit in interp_axis: -lo - 1 ... n - 1 + hi + 2 must fit)
        if (reach[side] + extent[side / 2] > (int64_t)INT32_MAX - 8)
            return fail(GT4MI_ERR_UNSUPPORTED, "point_sample: extent %lld + reach %lld is too large", (long long)extent[side / 2],
                        (long long)reach[side]);
    }
    if (extent[2] > (int64_t)INT32_MAX - 8)
        return fail(GT4MI_ERR_UNSUPPORTED, "point_sample: extent %lld along axis 2 is too large", (long long)extent[2]);
    if (elem_size != 4 && elem_size != 8)
        return fail(GT4MI_ERR_UNSUPPORTED, "point_sample: field item size %d is not supported (float32 or float64)", elem_size);
    if (pos_elem_size != 4 && pos_elem_size != 8)
        return fail(GT4MI_ERR_UNSUPPORTED, "point_sample: position item size %d is not supported (float32 or float64)", pos_elem_size);
    const bool column = pos_k == nullptr;
    const int64_t dst_extent[3] = {npoints, column ? extent[2] : 1, 1};  // axis 0 the point, axis 1 the level
    const int64_t pos_extent[3] = {npoints, 1, 1};
    for (int n = 0; n < nfields; ++n) {
        if (int rc = check_box_field(POINT_SAMPLE_CHECKS, "dst", n, dst[n], dst_extent, elem_size, true)) return rc;
        if (int rc = check_box_field(POINT_SAMPLE_CHECKS, "src", n, src[n], extent, elem_size, false, 0, reach)) return rc;  // (the readable box)
    }
    const gt4mi_field* const positions[3] = {pos_i, pos_j, pos_k};
    const char* const names[3] = {"pos_i", "pos_j", "pos_k"};
    const int npos = column ? 2 : 3;
    for (int m = 0; m < npos; ++m)
        if (int rc = check_box_field(POINT_SAMPLE_CHECKS, names[m], 0, *positions[m], pos_extent, pos_elem_size, false)) return rc;
    if (npoints == 0 || extent[0] == 0 || extent[1] == 0 || extent[2] == 0) return GT4MI_OK;
    NamedSpan pos[3];
    for (int m = 0; m < npos; ++m) pos[m] = NamedSpan{names[m], box_span(*positions[m], pos_extent, pos_elem_size)};
    // (a point reads any level of its src at any place of the readable box: the domain grown by the reach, over all levels)
    if (int rc = check_pairs_disjoint("point_sample", dst, src, nfields, dst_extent, extent, elem_size, elem_size, reach, pos, npos)) return rc;
    const int64_t lanes = column ? npoints * extent[2] : npoints;
    const int64_t blocks = cdiv(lanes, POINT_SAMPLE_BLOCK);
    if (blocks > INT32_MAX) return fail(GT4MI_ERR_UNSUPPORTED, "point_sample: too many points for one launch");
    if (launches) *launches = (int)cdiv(nfields, PAIR_MAX_FIELDS);
    if (flags & GT4MI_SAMPLE_DRY_RUN) return GT4MI_OK;
    PointSampleArgs a{};
    a.pi = shared_field(*pos_i, pos_elem_size), a.pj = shared_field(*pos_j, pos_elem_size);
    if (!column) a.pk = shared_field(*pos_k, pos_elem_size);
    a.lanes = (uint64_t)lanes;
    a.ni = (int)extent[0], a.nj = (int)extent[1], a.nk = (int)extent[2];
    a.lo_i = (int)reach[0], a.hi_i = (int)reach[1], a.lo_j = (int)reach[2], a.hi_j = (int)reach[3];
    a.fill = (flags & GT4MI_SAMPLE_FILL) ? 1 : 0;
    a.fill_value = fill_value;
    int next = 0;
    while (next_pair_batch(a, dst, src, &next, nfields, elem_size)) {
        with_item_type(elem_size, [&](auto t) {
            with_item_type(pos_elem_size, [&](auto q) {
                using T = decltype(t);
                using P = decltype(q);
                if (column) point_sample_method<T, P, true>(a, method, blocks, stream);
                else point_sample_method<T, P, false>(a, method, blocks, stream);
            });
        });
        GT4MI_HIP_CHECK(hipGetLastError());
    }
    return GT4MI_OK;
}

}  // namespace gt4mi
