// Vertical interpolation to run-time levels: the POINT values of up to 8 fields on the source levels of every column (i, j) become
// point values at the target levels of that column, ONE launch, the bracket and the weights of a target computed once for all fields.
//
// NEW component, no reference counterpart: gt4py.cartesian leaves output on pressure, height or isentropic levels and the vertical
// half of a semi-Lagrangian step to user stencils (a `while` loop, a carried run-time K index, reads at a run-time K index), one
// field per call, the search and the weights repeated for every field, "missing outside the range" a second pass.
//
// THE ARITHMETIC CONTRACT (include/gt4py_amd.h states it, tests/vertical_interp_ref.py restates it in plain Python).  All arithmetic
// is float64, one rounding per operation, no FMA (-ffp-contract=off and the pragma of common.hip.h); float32 items are widened exactly
// on load and the result is rounded once on store.  Per column: coordinates z[0..ns-1] (meant to increase strictly), targets
// x[0..nd-1] in ANY order, values q[0..ns-1] of each field.  A bracket index k starts at 0 and is carried from one target of the
// column to the next, m = 0, 1, ..., nd-1.  For a target x:
//   1. hunt     while k < ns-2 and z[k+1] <= x: k += 1;  then  while k > 0 and z[k] > x: k -= 1
//   2. outside  below = x < z[0], above = x > z[ns-1]
//               fill: store fill_value, next target.  clamp: x = z[0] / z[ns-1] before step 3.  linear: x stays and step 3 uses the
//               linear formula whatever the method (nearest moves item 0 / item ns-1)
//   3. inside   h = z[k+1] - z[k], t = (x - z[k]) / h
//               nearest         the ITEM q[k+1] if t >= 0.5 else q[k], its bit pattern moved; a NaN x stores the canonical quiet NaN
//               linear          (1.0 - t) * q[k] + t * q[k+1], both products rounded before the addition
//               cubic           k < 1 or k > ns-3: the linear formula; else Lagrange on z0..z3 = z[k-1..k+2],
//                               w_a = (product of (x - z_b), b != a, left to right) / (product of (z_a - z_b), b != a, left to right),
//                               out = ((w0*q0 + w1*q1) + w2*q2) + w3*q3
//               cubic_monotone  the cubic out limited to [mn, mx], mn = q[k+1] < q[k] ? q[k+1] : q[k], mx = q[k+1] > q[k] ? q[k+1] : q[k],
//                               out < mn ? mn : (out > mx ? mx : out), only where the cubic formula was used
//   4. the bracket, t and the weights are computed ONCE for all fields of the call
//
// PATH INDEPENDENCE: for strictly increasing z and a non-NaN x step 1 ends at the largest k <= ns-2 with z[k] <= x, or at 0 when there
// is none, wherever it started: the first loop leaves with k == ns-2 or z[k+1] > x, the second only moves down while z[k] > x, and
// moving down keeps z[k+1] > x.  A target's bits therefore depend on neither the other targets nor their order.
//
// WHY THE LOOPS END WHATEVER THE DATA HOLDS: the first loop only increments k, under k < ns-2; the second only decrements it, under
// k > 0.  They are the only places where k changes (`up()` and `down()` below), so 0 <= k <= ns-2 always, a target costs at most
// ns-2 steps each way, and the target loop counts to nd.  A NaN x fails every comparison: k stays, and the arithmetic yields NaN.
// Non-monotone or NaN z change which comparisons hold, never the bounds.
//
// NO DATA-DEPENDENT ADDRESSES: every K index of a load is k-1 ... k+2 -- k-1 and k+2 only under 1 <= k <= ns-3 --, 0 or ns-1; every
// K index of a store is m < nd.  The data picks among these integers, it never forms one.
//
// ONE THREAD PER COLUMN, lanes along I (the contiguous axis of the storage layout), a workgroup is 64 columns along I by 4 along J.
// The target loop is outermost: the lanes of a wave are at the same target level m (the stores of out[m] are one row) but at
// different brackets k (the loads of q[k] touch a few rows per instruction).  A lane keeps k, z[k], z[k+1] (updated as the hunt
// steps), z[0], z[ns-1] and the weights in registers; z[k-1] and z[k+2] are loaded once the hunt has settled, for the cubics only;
// the 2 or 4 values of every field are loaded after the hunt, the field loop innermost.  No LDS, no workspace, no scratch, no
// atomics, no ordering between workgroups: the host refuses a call in which a dst box meets a src box, a coordinate field or
// another dst box.
#pragma once

#include "column_entry.hip.h"
#include "common.hip.h"
#include "horizontal_interp.hip.h"  // InterpBits, interp_min, interp_max

namespace gt4mi {

struct VInterpArgs : ColumnArgs {  // (zs / zd: the coordinates)
    double fill;  // what GT4MI_VINTERP_FILL stores (rounded once to the item type in the kernel)
    int outside;
};

// T: item type of the fields, E: of the coordinates, METHOD: GT4MI_VINTERP_*, NF: entries the kernel has registers for (a.nf <= NF)
template <typename T, typename E, int METHOD, int NF>
__global__ void __launch_bounds__(COLUMN_TILE_I * COLUMN_TILE_J)
vertical_interp_kernel(const VInterpArgs a) {
    using U = typename InterpBits<T>::type;
    constexpr bool NEAREST = METHOD == GT4MI_VINTERP_NEAREST;
    constexpr bool CUBIC = METHOD == GT4MI_VINTERP_CUBIC || METHOD == GT4MI_VINTERP_CUBIC_MONOTONE;
    const unsigned tj = blockIdx.x / a.tiles_i, ti = blockIdx.x - tj * a.tiles_i;
    const int64_t i = (int64_t)ti * COLUMN_TILE_I + (threadIdx.x & 63u), j = (int64_t)tj * COLUMN_TILE_J + (threadIdx.x >> 6);
    if (i >= a.ni || j >= a.nj) return;
    const int ns = a.ns, nd = a.nd, nf = a.nf, outside = a.outside;
    const E* const zs = reinterpret_cast<const E*>(a.zs.p) + i * a.zs.s[0] + j * a.zs.s[1];
    const E* const zd = reinterpret_cast<const E*>(a.zd.p) + i * a.zd.s[0] + j * a.zd.s[1];
    const int64_t zsk = a.zs.s[2], zdk = a.zd.s[2];
    const T* src[NF];
    T* dst[NF];
#pragma unroll
    for (int n = 0; n < NF; ++n) {
        src[n] = nullptr, dst[n] = nullptr;
        if (n < nf) {
            src[n] = reinterpret_cast<const T*>(a.e[n].src) + i * a.e[n].s[0] + j * a.e[n].s[1];
            dst[n] = reinterpret_cast<T*>(a.e[n].dst) + i * a.e[n].d[0] + j * a.e[n].d[1];
        }
    }
    // fill_value in the item type: one rounding; a NaN is the canonical quiet NaN
    T fill_item = (T)a.fill;
    if (a.fill != a.fill) {
        const U bits = InterpBits<T>::QNAN;
        __builtin_memcpy(&fill_item, &bits, sizeof(T));
    }
    // the bracket [z[k], z[k+1]] (ns >= 2: the host has checked), and the two ends of the column
    int k = 0;
    double zk = (double)zs[0], zk1 = (double)zs[zsk];
    const double zfirst = zk, zlast = (double)zs[(int64_t)(ns - 1) * zsk];

    // the ONLY places where k changes; `up` is called under k < ns - 2, `down` under k > 0
    auto up = [&]() {
        ++k;
        zk = zk1, zk1 = (double)zs[(int64_t)(k + 1) * zsk];
    };
    auto down = [&]() {
        --k;
        zk1 = zk, zk = (double)zs[(int64_t)k * zsk];
    };

    for (int m = 0; m < nd; ++m) {
        double x = (double)zd[(int64_t)m * zdk];
        while (k < ns - 2 && zk1 <= x) up();
        while (k > 0 && zk > x) down();
        const bool below = x < zfirst, above = x > zlast;
        const bool out_of_range = below || above;
        if (out_of_range && outside == GT4MI_VINTERP_OUTSIDE_FILL) {
#pragma unroll
            for (int n = 0; n < NF; ++n)
                if (n < nf) dst[n][(int64_t)m * a.e[n].d[2]] = fill_item;
            continue;
        }
        if (out_of_range && outside == GT4MI_VINTERP_OUTSIDE_CLAMP) x = below ? zfirst : zlast;
        const bool extend = out_of_range && outside == GT4MI_VINTERP_OUTSIDE_LINEAR;
        const double t = (x - zk) / (zk1 - zk);
        if constexpr (NEAREST) {
            const int64_t kk = extend ? (below ? 0 : ns - 1) : (t >= 0.5 ? k + 1 : k);
            const bool nan = x != x;
#pragma unroll
            for (int n = 0; n < NF; ++n) {
                if (n < nf) {
                    const U v = reinterpret_cast<const U*>(src[n])[kk * a.e[n].s[2]];
                    reinterpret_cast<U*>(dst[n])[(int64_t)m * a.e[n].d[2]] = nan ? InterpBits<T>::QNAN : v;
                }
            }
        } else {
            bool cubic = false;
            double w0 = 0.0, w1 = 0.0, w2 = 0.0, w3 = 0.0;
            if constexpr (CUBIC) {
                cubic = !extend && k >= 1 && k <= ns - 3;
                if (cubic) {
                    const double z0 = (double)zs[(int64_t)(k - 1) * zsk], z1 = zk, z2 = zk1, z3 = (double)zs[(int64_t)(k + 2) * zsk];
                    const double x0 = x - z0, x1 = x - z1, x2 = x - z2, x3 = x - z3;
                    w0 = ((x1 * x2) * x3) / (((z0 - z1) * (z0 - z2)) * (z0 - z3));
                    w1 = ((x0 * x2) * x3) / (((z1 - z0) * (z1 - z2)) * (z1 - z3));
                    w2 = ((x0 * x1) * x3) / (((z2 - z0) * (z2 - z1)) * (z2 - z3));
                    w3 = ((x0 * x1) * x2) / (((z3 - z0) * (z3 - z1)) * (z3 - z2));
                }
            }
            const double u = 1.0 - t;
#pragma unroll
            for (int n = 0; n < NF; ++n) {
                if (n < nf) {
                    const int64_t sk = a.e[n].s[2];
                    const T* const s = src[n] + (int64_t)k * sk;
                    const T r1 = s[0], r2 = s[sk];
                    double out;
                    if (CUBIC && cubic) {
                        const T r0 = *(s - sk), r3 = s[2 * sk];  // every load of the entry before its first multiply
                        const double q0 = (double)r0, q1 = (double)r1, q2 = (double)r2, q3 = (double)r3;
                        out = ((w0 * q0 + w1 * q1) + w2 * q2) + w3 * q3;
                        if constexpr (METHOD == GT4MI_VINTERP_CUBIC_MONOTONE) {
                            const double mn = interp_min(q1, q2), mx = interp_max(q1, q2);
                            out = out < mn ? mn : (out > mx ? mx : out);
                        }
                    } else {
                        out = u * (double)r1 + t * (double)r2;
                    }
                    dst[n][(int64_t)m * a.e[n].d[2]] = (T)out;
                }
            }
        }
    }
}

const ColumnEntry VINTERP_ENTRY = {"vertical_interp", {"src_coord", "dst_coord"}, "coordinate", 0, 2,
                                   "at least two source levels and one target level are needed", GT4MI_VINTERP_DRY_RUN,
                                   {"vertical_interp", "extent", "only a src or a coordinate field may be broadcast", false, false}};

template <typename T, typename E, int METHOD>
inline void vinterp_launch(const VInterpArgs& a, int64_t blocks, hipStream_t stream) {
    with_pair_entries(a.nf, [&](auto nf) {
        hipLaunchKernelGGL((vertical_interp_kernel<T, E, METHOD, decltype(nf)::value>), dim3((unsigned)blocks),
                           dim3(COLUMN_TILE_I * COLUMN_TILE_J), 0, stream, a);
    });
}

// every check, then (unless `flags` carries GT4MI_VINTERP_DRY_RUN) the launches
inline int vertical_interp(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* src_coord,
                           const gt4mi_field* dst_coord, const int64_t extent_ij[2], int64_t ns, int64_t nd, int elem_size,
                           int coord_elem_size, int method, int outside, double fill_value, int flags, hipStream_t stream, int* launches) {
    if (int rc = column_call(VINTERP_ENTRY, dst, src, nfields, src_coord, dst_coord, extent_ij, ns, nd, flags, launches)) return rc;
    if (method < GT4MI_VINTERP_NEAREST || method > GT4MI_VINTERP_CUBIC_MONOTONE)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "vertical_interp: unknown method %d", method);
    if (outside < GT4MI_VINTERP_OUTSIDE_CLAMP || outside > GT4MI_VINTERP_OUTSIDE_FILL)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "vertical_interp: unknown outside value %d", outside);
    VInterpArgs a{};
    int64_t blocks = 0;
    if (int rc = column_fields(VINTERP_ENTRY, a, &blocks, dst, src, nfields, src_coord, dst_coord, extent_ij, ns, nd, elem_size,
                               coord_elem_size, flags, launches))
        return rc;
    if (blocks == 0) return GT4MI_OK;  // an empty extent or a dry run
    a.fill = fill_value, a.outside = outside;
    int next = 0;
    while (next_pair_batch(a, dst, src, &next, nfields, elem_size)) {
        with_item_type(elem_size, [&](auto t) {
            with_item_type(coord_elem_size, [&](auto e) {
                using T = decltype(t);
                using E = decltype(e);
                switch (method) {
                    case GT4MI_VINTERP_NEAREST: vinterp_launch<T, E, GT4MI_VINTERP_NEAREST>(a, blocks, stream); break;
                    case GT4MI_VINTERP_LINEAR: vinterp_launch<T, E, GT4MI_VINTERP_LINEAR>(a, blocks, stream); break;
                    case GT4MI_VINTERP_CUBIC: vinterp_launch<T, E, GT4MI_VINTERP_CUBIC>(a, blocks, stream); break;
                    default: vinterp_launch<T, E, GT4MI_VINTERP_CUBIC_MONOTONE>(a, blocks, stream); break;
                }
            });
        });
        GT4MI_HIP_CHECK(hipGetLastError());
    }
    return GT4MI_OK;
}

}  // namespace gt4mi
