// Conservative vertical remapping: the cell means of up to 8 fields on the source levels of every column (i, j) become cell
// means on the target levels of that column, ONE launch, the geometry of a column computed once for all its fields.
//
// NEW component, no reference counterpart: gt4py.cartesian leaves remapping to user stencils (a FORWARD sweep that carries a
// run-time source index, a `while` over the overlapping source cells, a read at a run-time K index), one field per call.
//
// THE ARITHMETIC CONTRACT (include/gt4py_amd.h states it, tests/vertical_remap_ref.py restates it in plain Python).  All
// arithmetic is float64, one rounding per operation, no FMA (-ffp-contract=off and the pragma of common.hip.h); float32 items
// are widened exactly on load and the result is rounded once on store.  Per column: source edges zs[0..ns], target edges
// zd[0..nd], source means q[0..ns-1].  The first source cell reaches to -inf, the last to +inf.  A source index k is kept
// across the target cells of the column and only grows.  For target cell m, lo = zd[m], hi = zd[m+1], d = hi - lo:
//   advance   while k < ns-1 and not (zs[k+1] > lo): k += 1
//   terms     l = lo if k == 0 else (zs[k] if zs[k] > lo else lo);  r = hi if k == ns-1 else (zs[k+1] if zs[k+1] < hi else hi)
//             w = (r - l) / d;  t = w * v_k;  the first term IS the accumulator (a lone -0.0 survives), later ones are added
//             stop after the term with k == ns-1 or zs[k+1] >= hi, else k += 1
//   out[m]    the accumulator (the weights carry 1/d)
//   pcm       v_k = q[k]
//   plm       v_k = q[k] + s[k] * (0.5 * (xl + xr) - 0.5),  h = zs[k+1] - zs[k],  xl = (l - zs[k]) / h,  xr = (r - zs[k]) / h
//             s[0] = s[ns-1] = 0; else dl = q[k] - q[k-1], dr = q[k+1] - q[k]; if dl * dr > 0:
//             g = (q[k+1] - q[k-1]) / (0.5 h[k-1] + h[k] + 0.5 h[k+1]) * h[k] (left to right), a = |g|, then a = 2|dl| if
//             2|dl| < a, then a = 2|dr| if 2|dr| < a, s[k] = copysign(a, g); else s[k] = 0
//
// WHY THE LOOPS END WHATEVER THE DATA HOLDS: the loop over m counts to nd.  `step()` is the only place where k changes, it
// adds 1, and both inner loops run it only under k < ns - 1: the advance loop tests that first, the term loop leaves at
// k >= ns - 1 before it could step.  So a column makes at most ns - 1 steps and ns + nd - 1 terms; NaN, repeated or
// non-monotone edges change which comparisons hold, never these counters.  Every K index of a load is k - 1 ... k + 2 guarded
// against ns by the same integers, every K index of a store is m < nd: no address depends on the data.
//
// ONE THREAD PER COLUMN, lanes along I (the contiguous axis of the storage layout), a workgroup is 64 columns along I by 4
// along J.  The lanes of a wave are at the same target level m (the stores of out[m] are one row) but at different source
// levels k: the loads of q[k] touch a few rows per instruction.  Each lane reads every source item once, in order, one level
// ahead of its use.  q[k-1], q[k], q[k+1], s[k] and the accumulator of every entry live in registers; the field loop is inside
// the overlap loop.  No LDS, no workspace, no scratch, no atomics, no ordering between workgroups: the host refuses a call in
// which a dst box meets a src box, an edge field or another dst box.
#pragma once

#include "column_entry.hip.h"
#include "common.hip.h"

namespace gt4mi {

struct RemapArgs : ColumnArgs {};  // (zs / zd: the edges)

// the limited centred slope across a cell of thickness hc, den = 0.5 h[k-1] + h[k] + 0.5 h[k+1] (horizontal_remap.hip.h reads den
// from its overlap table)
__device__ __forceinline__ double remap_slope_den(double qm, double qc, double qp, double den, double hc) {
    const double dl = qc - qm, dr = qp - qc;
    if (!(dl * dr > 0.0)) return 0.0;
    const double g = (qp - qm) / den * hc;
    double a = fabs(g);
    const double b = 2.0 * fabs(dl), c = 2.0 * fabs(dr);
    if (b < a) a = b;
    if (c < a) a = c;
    return copysign(a, g);
}

__device__ __forceinline__ double remap_slope(double qm, double qc, double qp, double hm, double hc, double hp) {
    return remap_slope_den(qm, qc, qp, 0.5 * hm + hc + 0.5 * hp, hc);
}

// T: item type of the fields, E: of the edges, METHOD: GT4MI_REMAP_*, NF: entries the kernel has registers for (a.nf <= NF)
template <typename T, typename E, int METHOD, int NF>
__global__ void __launch_bounds__(COLUMN_TILE_I * COLUMN_TILE_J)
vertical_remap_kernel(const RemapArgs a) {
    constexpr bool PLM = METHOD == GT4MI_REMAP_PLM;
    const unsigned tj = blockIdx.x / a.tiles_i, ti = blockIdx.x - tj * a.tiles_i;
    const int64_t i = (int64_t)ti * COLUMN_TILE_I + (threadIdx.x & 63u), j = (int64_t)tj * COLUMN_TILE_J + (threadIdx.x >> 6);
    if (i >= a.ni || j >= a.nj) return;
    const int ns = a.ns, nd = a.nd, nf = a.nf;
    const E* const zs = reinterpret_cast<const E*>(a.zs.p) + i * a.zs.s[0] + j * a.zs.s[1];
    const E* const zd = reinterpret_cast<const E*>(a.zd.p) + i * a.zd.s[0] + j * a.zd.s[1];
    const int64_t zsk = a.zs.s[2], zdk = a.zd.s[2];
    const T* src[NF];
    T* dst[NF];
    double qm[NF], qc[NF], qp[NF], sl[NF], acc[NF];
#pragma unroll
    for (int n = 0; n < NF; ++n) {
        qm[n] = qc[n] = qp[n] = sl[n] = acc[n] = 0.0;
        src[n] = nullptr, dst[n] = nullptr;
        if (n < nf) {
            src[n] = reinterpret_cast<const T*>(a.e[n].src) + i * a.e[n].s[0] + j * a.e[n].s[1];
            dst[n] = reinterpret_cast<T*>(a.e[n].dst) + i * a.e[n].d[0] + j * a.e[n].d[1];
            qc[n] = (double)src[n][0];
            if (ns > 1) qp[n] = (double)src[n][a.e[n].s[2]];
        }
    }
    // source cell k = [zk, zk1), its neighbours' far edges zkm = zs[k-1] and zk2 = zs[k+2] where they exist
    int k = 0;
    double zkm = 0.0, zk = (double)zs[0], zk1 = (double)zs[zsk], zk2 = ns > 1 ? (double)zs[2 * zsk] : 0.0;

    // the ONLY place where k changes; callers guarantee k < ns - 1 on entry
    auto step = [&]() {
        ++k;
        zkm = zk, zk = zk1, zk1 = zk2;
        if (k + 2 <= ns) zk2 = (double)zs[(int64_t)(k + 2) * zsk];
        const bool inner = k < ns - 1;  // (k > 0 here)
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            if (n < nf) {
                qm[n] = qc[n], qc[n] = qp[n];
                if (inner) qp[n] = (double)src[n][(int64_t)(k + 1) * a.e[n].s[2]];
                if constexpr (PLM) sl[n] = inner ? remap_slope(qm[n], qc[n], qp[n], zk - zkm, zk1 - zk, zk2 - zk1) : 0.0;
            }
        }
    };

    double hi = (double)zd[0];
    for (int m = 0; m < nd; ++m) {
        const double lo = hi;
        hi = (double)zd[(int64_t)(m + 1) * zdk];
        const double d = hi - lo;
        while (k < ns - 1 && !(zk1 > lo)) step();
        bool first = true;
        for (;;) {
            const double l = k == 0 ? lo : (zk > lo ? zk : lo);
            const double r = k == ns - 1 ? hi : (zk1 < hi ? zk1 : hi);
            const double w = (r - l) / d;
            double c = 0.0;
            if constexpr (PLM) {
                const double h = zk1 - zk;
                const double xl = (l - zk) / h, xr = (r - zk) / h;
                c = 0.5 * (xl + xr) - 0.5;
            }
#pragma unroll
            for (int n = 0; n < NF; ++n) {
                if (n < nf) {
                    const double v = PLM ? qc[n] + sl[n] * c : qc[n];
                    const double t = w * v;
                    acc[n] = first ? t : acc[n] + t;
                }
            }
            first = false;
            if (k >= ns - 1 || zk1 >= hi) break;
            step();
        }
#pragma unroll
        for (int n = 0; n < NF; ++n)
            if (n < nf) dst[n][(int64_t)m * a.e[n].d[2]] = (T)acc[n];
    }
}

const ColumnEntry REMAP_ENTRY = {"vertical_remap", {"src_edges", "dst_edges"}, "edge", 1, 1, "at least one each is needed", GT4MI_REMAP_DRY_RUN,
                                 {"vertical_remap", "extent", "only a src or an edge field may be broadcast", false, false}};

template <typename T, typename E, int METHOD>
inline void remap_launch(const RemapArgs& a, int64_t blocks, hipStream_t stream) {
    with_pair_entries(a.nf, [&](auto nf) {
        hipLaunchKernelGGL((vertical_remap_kernel<T, E, METHOD, decltype(nf)::value>), dim3((unsigned)blocks),
                           dim3(COLUMN_TILE_I * COLUMN_TILE_J), 0, stream, a);
    });
}

// every check, then (unless `flags` carries GT4MI_REMAP_DRY_RUN) the launches
inline int vertical_remap(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const gt4mi_field* src_edges,
                          const gt4mi_field* dst_edges, const int64_t extent_ij[2], int64_t ns, int64_t nd, int elem_size,
                          int edge_elem_size, int method, int flags, hipStream_t stream, int* launches) {
    if (int rc = column_call(REMAP_ENTRY, dst, src, nfields, src_edges, dst_edges, extent_ij, ns, nd, flags, launches)) return rc;
    if (method != GT4MI_REMAP_PCM && method != GT4MI_REMAP_PLM)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "vertical_remap: unknown method %d", method);
    RemapArgs a{};
    int64_t blocks = 0;
    if (int rc = column_fields(REMAP_ENTRY, a, &blocks, dst, src, nfields, src_edges, dst_edges, extent_ij, ns, nd, elem_size, edge_elem_size,
                               flags, launches))
        return rc;
    if (blocks == 0) return GT4MI_OK;  // an empty extent or a dry run
    int next = 0;
    while (next_pair_batch(a, dst, src, &next, nfields, elem_size)) {
        with_item_type(elem_size, [&](auto t) {
            with_item_type(edge_elem_size, [&](auto e) {
                using T = decltype(t);
                using E = decltype(e);
                if (method == GT4MI_REMAP_PLM) remap_launch<T, E, GT4MI_REMAP_PLM>(a, blocks, stream);
                else remap_launch<T, E, GT4MI_REMAP_PCM>(a, blocks, stream);
            });
        });
        GT4MI_HIP_CHECK(hipGetLastError());
    }
    return GT4MI_OK;
}

}  // namespace gt4mi
