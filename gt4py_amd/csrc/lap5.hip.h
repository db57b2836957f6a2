// 5-point star stencils for gfx950: out[i,j,k] = f(in[i,j,k], in[i-1,j,k], in[i+1,j,k], in[i,j-1,k], in[i,j+1,k]).
//
// Reference semantics: the single-statement PARALLEL stencils listed in include/gt4py_amd.h
// (numpy backend code shape: /root/reference/src/gt4py/cartesian/gtc/numpy/npir_codegen.py:205-212).
//
// Roofline: HBM.  Algorithmic traffic 2*sizeof(T) bytes per lattice update (one read, one write).
//
// Fast path ("strip" kernel): a workgroup owns a strip BLOCK*VEC points wide in I (contiguous, one
// 16-byte vector per lane) and LJ rows tall in J at one K level.
//   1. every lane issues the loads of all LJ+2 rows of its column vector up front (maximum bytes in
//      flight per wave; measured +8 % over a rolling three-row window on MI355X),
//   2. the I-neighbours in[i-1], in[i+VEC] come from the adjacent lanes with DPP wave shifts
//      (v_mov_b32_dpp wave_shr:1 / wave_shl:1); only the two edge lanes of a wave load them,
//   3. results leave with non-temporal 16-byte stores (`out` is never re-read).
// No LDS and no barriers: the J reuse lives in registers, the strip's two halo rows are L2 hits.
// Tuning data: profiles/r1_microbench_*.log (LJ, block size, nt loads/stores, XCD order).
#pragma once

#include <type_traits>

#include "common.hip.h"
#include "lane_shift.hip.h"

#pragma clang fp contract(off)

namespace gt4mi {

// c = in[0,0], w = in[-1,0], e = in[+1,0], s = in[0,-1], n = in[0,+1].
// T: field dtype, W: dtype of the float literals' promotion (double unless literal precision 32
// on float fields) -- /root/reference/src/gt4py/cartesian/gtc/passes/gtir_upcaster.py:43-143.
template <typename T, typename W, int VARIANT>
__device__ __forceinline__ T lap5_expr(T c, T w, T e, T s, T n) {
    if constexpr (VARIANT == GT4MI_LAP_NOTEBOOK) {
        // ((((-4.0*c) + w) + e) + s) + n
        W r = (W)(-4.0) * (W)c;
        r = r + (W)w;
        r = r + (W)e;
        r = r + (W)s;
        r = r + (W)n;
        return (T)r;
    } else if constexpr (VARIANT == GT4MI_LAP_DOCS) {
        // (-4.0*c) + (((e + w) + n) + s)   -- the bracket is evaluated in the field dtype
        T sum = ((e + w) + n) + s;
        return (T)(((W)(-4.0) * (W)c) + (W)sum);
    } else if constexpr (VARIANT == GT4MI_LAP_SUITE) {
        // (4.0*c) - (((e + w) + n) + s)
        T sum = ((e + w) + n) + s;
        return (T)(((W)(4.0) * (W)c) - (W)sum);
    } else {
        // 0.25 * (((n + s) + e) + w)
        T sum = ((n + s) + e) + w;
        return (T)((W)(0.25) * (W)sum);
    }
}

// The strip of ONE lane: VEC columns from i0 x rows [j0, min(j0+LJ, dJ)) of level k.  edge_w / edge_e: the lane's west / east
// neighbour column is not in the adjacent lane's registers (first / last lane of a row of lanes) and is loaded instead.
// MASKED: only the columns [c_lo, c_hi) of the (16-byte aligned) view are the compute domain -- a domain whose first column
// is not on a 16-byte boundary, or whose width is odd, shifted onto the boundary (lap5_launch_variant): vectors are loaded
// whole (they reach at most one column into the halo on either side), stored element by element where they straddle the
// domain's edge, and a neighbour column outside the halo is never loaded (its consumer is not a domain point).
template <typename T, typename W, int VARIANT, int VEC, int LJ, bool MASKED = false>
__device__ __forceinline__ void lap5_strip_lane(const View<const T>& in, const View<T>& out, int dJ, int i0, bool active,
                                                bool edge_w, bool edge_e, int j0, unsigned k, int c_lo = 0, int c_hi = 0) {
    const T* __restrict__ col = in.p + (int64_t)k * in.sk + i0;
    T* __restrict__ ocol = out.p + (int64_t)k * out.sk + i0;

    // Row t of the register tile is `in` row min(j0 - 1 + t, dJ): rows past the strip's last valid
    // halo row are clamped (their results are never stored).
    T r[LJ + 2][VEC];
    int64_t roff[LJ + 2];
#pragma unroll
    for (int t = 0; t < LJ + 2; ++t) {
        int jr = j0 - 1 + t;
        jr = jr > dJ ? dJ : jr;
        roff[t] = (int64_t)jr * in.sj;
        vload<T, VEC>(col + roff[t], r[t]);
    }
    bool first_in = true, last_in = true;  // the lane's first / last column is a domain point
    if constexpr (MASKED) {
        first_in = i0 >= c_lo && i0 < c_hi;
        last_in = i0 + VEC - 1 >= c_lo && i0 + VEC - 1 < c_hi;
    }
    T w[LJ + 2], e[LJ + 2];
#pragma unroll
    for (int t = 1; t <= LJ; ++t) {
        T wl = lane_shift<T, true>(r[t][VEC - 1]);
        T el = lane_shift<T, false>(r[t][0]);
        if (edge_w && first_in) wl = col[roff[t] - 1];
        if (edge_e && last_in) el = col[roff[t] + VEC];
        w[t] = wl;
        e[t] = el;
    }
#pragma unroll
    for (int t = 1; t <= LJ; ++t) {
        T res[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) {
            const T wv = (v == 0) ? w[t] : r[t][v - 1];
            const T ev = (v == VEC - 1) ? e[t] : r[t][v + 1];
            res[v] = lap5_expr<T, W, VARIANT>(r[t][v], wv, ev, r[t - 1][v], r[t + 1][v]);
        }
        if (active && (j0 + t - 1 < dJ)) {
            T* o = ocol + (int64_t)(j0 + t - 1) * out.sj;
            if (!MASKED || (first_in && last_in)) {
                vstore<T, VEC, true>(o, res);
            } else {
#pragma unroll
                for (int v = 0; v < VEC; ++v)
                    if (i0 + v >= c_lo && i0 + v < c_hi) __builtin_nontemporal_store(res[v], o + v);
            }
        }
    }
}

// One strip: columns [bx*BLOCK*VEC, ...) x rows [j0, min(j0+LJ, dJ)) of level k; the lanes of a wave lie along I.
template <typename T, typename W, int VARIANT, int VEC, int LJ, int BLOCK, bool MASKED = false>
__device__ __forceinline__ void lap5_strip_tile(const View<const T>& in, const View<T>& out, int dI, int dJ,
                                                unsigned bx, int j0, unsigned k, int c_lo = 0) {
    const unsigned lane = threadIdx.x & 63;
    // Lanes past the end of the row stay active (DPP needs their neighbours' exec bits) but are
    // clamped onto the last valid vector and never store.  (MASKED: dI counts from the aligned column, the domain is
    // [c_lo, dI); the last vector may hold one column of halo.)
    int i0 = (int)(bx * BLOCK + threadIdx.x) * VEC;
    const bool active = i0 < dI;
    if (!active) i0 = MASKED ? ((dI + VEC - 1) / VEC - 1) * VEC : dI - VEC;
    lap5_strip_lane<T, W, VARIANT, VEC, LJ, MASKED>(in, out, dJ, i0, active, lane == 0, (lane == 63) || (i0 + VEC >= dI), j0, k,
                                                   c_lo, dI);
}

// A box only LPR * VEC columns wide (the W / E boxes of a decomposed apply): a wave is 64 / LPR rows of LPR lanes, each row of
// lanes a strip of LJ rows of its own -- the lane shifts of lap5_strip_lane still fetch the neighbour column inside a row of
// lanes, the first and last lane of each row load theirs.  A wave covers (64 / LPR) * LJ rows of the box.
template <typename T, typename W, int VARIANT, int VEC, int LJ, int LPR>
__device__ __forceinline__ void lap5_narrow_tile(const View<const T>& in, const View<T>& out, int dI, int dJ, unsigned tile,
                                                 unsigned k) {
    const int lane = (int)(threadIdx.x & 63);
    const int li = lane % LPR, sub = lane / LPR;
    int i0 = li * VEC;
    const bool active = i0 < dI;
    if (!active) i0 = dI - VEC;
    const int j0 = ((int)tile * (64 / LPR) + sub) * LJ;
    lap5_strip_lane<T, W, VARIANT, VEC, LJ>(in, out, dJ, i0, active && j0 < dJ, li == 0, (li == LPR - 1) || (i0 + VEC >= dI),
                                            j0 < dJ ? j0 : dJ, k);
}

struct Lap5Tuning {
    static constexpr int LJ = 8;  // rows per strip; all LJ+2 row loads are in flight at once
    // Runs of 4 consecutive strips per XCD: measured 382 vs 372 GLUPS (none) vs 370 (one contiguous
    // range per XCD) at 512^3, and L2->fabric reads 1.13x instead of 1.33x the algorithmic bytes
    // (profiles/r1_microbench_g_xcd_groups.log, r1_lap512_fetch_by_variant.txt).
    static constexpr int XCDG = 4;
};

// Runs of Lap5Tuning::XCDG consecutive strips share an XCD (private L2), so the halo rows they share are L2 hits instead of a
// second fabric fetch.
template <typename T, typename W, int VARIANT, int VEC, int BLOCK, bool MASKED = false>
__global__ void __launch_bounds__(BLOCK)
lap5_strip_kernel(View<const T> in, View<T> out, int dI, int dJ, unsigned tiles_x, unsigned tiles_y, int c_lo = 0) {
    constexpr int LJ = Lap5Tuning::LJ;
    const unsigned b = xcd_remap_grouped<(unsigned)Lap5Tuning::XCDG>(blockIdx.x, gridDim.x);
    const unsigned bx = b % tiles_x;
    const unsigned by = (b / tiles_x) % tiles_y;
    const unsigned k = b / (tiles_x * tiles_y);
    lap5_strip_tile<T, W, VARIANT, VEC, LJ, BLOCK, MASKED>(in, out, dI, dJ, bx, (int)by * LJ, k, c_lo);
}

// Any-stride fallback: one thread per point, I fastest across lanes.  Correct for every layout the
// reference accepts (stencil_object.py:412-425 only warns about non-optimal layouts).
template <typename T, typename W, int VARIANT>
__global__ void __launch_bounds__(256)
lap5_generic_kernel(View<const T> in, View<T> out, int dI, int dJ, int dK) {
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= dI || j >= dJ) return;
    for (int k = blockIdx.z; k < dK; k += gridDim.z) {
        const T* p = in.p + (int64_t)i * in.si + (int64_t)j * in.sj + (int64_t)k * in.sk;
        const T r = lap5_expr<T, W, VARIANT>(p[0], p[-in.si], p[in.si], p[-in.sj], p[in.sj]);
        out.p[(int64_t)i * out.si + (int64_t)j * out.sj + (int64_t)k * out.sk] = r;
    }
}

// ---- launch configuration ------------------------------------------------------------------
template <typename T, typename W, int VARIANT, int VEC, int BLOCK>
inline int lap5_launch_strip(const View<const T>& in, const View<T>& out, const int64_t d[3],
                             hipStream_t stream) {
    constexpr int LJ = Lap5Tuning::LJ;
    const unsigned tx = (unsigned)cdiv(d[0], (int64_t)BLOCK * VEC);
    const unsigned ty = (unsigned)cdiv(d[1], LJ);
    const int64_t n = (int64_t)tx * ty * d[2];
    if (n > INT32_MAX) return fail(GT4MI_ERR_UNSUPPORTED, "lap5: domain too large for one launch");
    hipLaunchKernelGGL((lap5_strip_kernel<T, W, VARIANT, VEC, BLOCK>), dim3((unsigned)n), dim3(BLOCK),
                       launch_dynamic_lds(), stream, in, out, (int)d[0], (int)d[1], tx, ty, 0);
    return GT4MI_OK;
}

// The same strips for a domain that starts `lead` columns past a 16-byte boundary and / or has an odd width: the views are
// moved onto the boundary and the kernel masks the columns outside [lead, lead + dI) (lap5_strip_lane<..., MASKED>).
template <typename T, typename W, int VARIANT, int VEC, int BLOCK>
inline int lap5_launch_strip_masked(const View<const T>& in, const View<T>& out, const int64_t d[3], int lead, hipStream_t stream) {
    constexpr int LJ = Lap5Tuning::LJ;
    const View<const T> in_a{in.p - lead, in.si, in.sj, in.sk};
    const View<T> out_a{out.p - lead, out.si, out.sj, out.sk};
    const int64_t width = d[0] + lead;
    const unsigned tx = (unsigned)cdiv(width, (int64_t)BLOCK * VEC);
    const unsigned ty = (unsigned)cdiv(d[1], LJ);
    const int64_t n = (int64_t)tx * ty * d[2];
    if (n > INT32_MAX) return fail(GT4MI_ERR_UNSUPPORTED, "lap5: domain too large for one launch");
    hipLaunchKernelGGL((lap5_strip_kernel<T, W, VARIANT, VEC, BLOCK, true>), dim3((unsigned)n), dim3(BLOCK),
                       launch_dynamic_lds(), stream, in_a, out_a, (int)width, (int)d[1], tx, ty, lead);
    return GT4MI_OK;
}

// Lanes per strip tile for rows of `lanes_per_row` lanes: a row of up to 64 / 128 lanes gets tiles of one / two waves, so that no
// workgroup carries waves that lie past the end of the row; anything wider gets the 256 lanes the kernels were tuned with.
inline int lap5_tile_lanes(int64_t lanes_per_row) { return lanes_per_row <= 64 ? 64 : (lanes_per_row <= 128 ? 128 : 256); }

template <typename T, typename W, int VARIANT>
inline int lap5_launch_variant(const View<const T>& in, const View<T>& out, const int64_t d[3],
                               hipStream_t stream) {
    constexpr int VMAX = 16 / sizeof(T);
    // (domains only a few columns wide -- west / east boundary strips -- go to the thread-per-point kernel)
    if (in.si == 1 && out.si == 1 && d[0] >= 16) {
        const bool vec = vec_ok(in, VMAX) && vec_ok(out, VMAX) && (d[0] % VMAX == 0);
        if (vec) {
            const int block = lap5_tile_lanes(d[0] / VMAX);
            if (block == 64) return lap5_launch_strip<T, W, VARIANT, VMAX, 64>(in, out, d, stream);
            if (block == 128) return lap5_launch_strip<T, W, VARIANT, VMAX, 128>(in, out, d, stream);
            return lap5_launch_strip<T, W, VARIANT, VMAX, 256>(in, out, d, stream);
        }
        {
            // Rows that are aligned among themselves to a lane of TWO items (16 bytes for 8-byte items, 8 bytes for 4-byte
            // ones: a whole vector then reaches at most one column into the halo on either side), `inp` and `out` equally far
            // (0 or 1 column) from such a boundary: two-item lanes with masked edges instead of one-item lanes (a domain origin
            // that is not the storage's aligned column, or an odd width, cost 14-19 % on 8-byte lanes:
            // profiles/r3_misaligned_origin.log)
            constexpr int VM = 2;
            constexpr uintptr_t unit = VM * sizeof(T);
            const int lead = (int)((reinterpret_cast<uintptr_t>(in.p) % unit) / sizeof(T));
            const bool same = lead == (int)((reinterpret_cast<uintptr_t>(out.p) % unit) / sizeof(T));
            if (same && in.sj % VM == 0 && in.sk % VM == 0 && out.sj % VM == 0 && out.sk % VM == 0) {
                const int64_t lanes = cdiv(d[0] + lead, VM);
                const int block = lap5_tile_lanes(lanes);
                if (block == 64) return lap5_launch_strip_masked<T, W, VARIANT, VM, 64>(in, out, d, lead, stream);
                if (block == 128) return lap5_launch_strip_masked<T, W, VARIANT, VM, 128>(in, out, d, lead, stream);
                // one lane more than the aligned domain needs (512 columns from an odd origin: 257 lanes) must not cost a
                // second, almost empty workgroup per row: five waves instead of four where that wastes fewer lanes
                if (cdiv(lanes, 320) * 320 < cdiv(lanes, 256) * 256)
                    return lap5_launch_strip_masked<T, W, VARIANT, VM, 320>(in, out, d, lead, stream);
                return lap5_launch_strip_masked<T, W, VARIANT, VM, 256>(in, out, d, lead, stream);
            }
        }
        if (d[0] <= 64) return lap5_launch_strip<T, W, VARIANT, 1, 64>(in, out, d, stream);
        return lap5_launch_strip<T, W, VARIANT, 1, 256>(in, out, d, stream);
    }
    dim3 grid((unsigned)cdiv(d[0], 64), (unsigned)cdiv(d[1], 4),
              (unsigned)(d[2] < 65535 ? d[2] : 65535));
    hipLaunchKernelGGL((lap5_generic_kernel<T, W, VARIANT>), grid, dim3(256), 0, stream, in, out,
                       (int)d[0], (int)d[1], (int)d[2]);
    return GT4MI_OK;
}

// ---- argument preparation shared by every host entry of the family (this file, lap5_ring / lap5_push / lap5_edge.hip.h) ------
template <typename T>
inline View<const T> const_view(const View<T>& v) { return View<const T>{v.p, v.si, v.sj, v.sk}; }

inline bool empty_domain(const int64_t d[3]) { return d[0] == 0 || d[1] == 0 || d[2] == 0; }

// What the forms built on gt4mi_lap5_* refuse an overlap with; gt4mi_lap5_* itself says why (lap5_run).
constexpr const char* LAP5_OVERLAP_SEE = "lap5: 'inp' and 'out' overlap in memory (see gt4mi_lap5_*)";

// `inp` is read `reach` points beyond `domain` along I and J, `out` is written on `domain`: may a written element be a read one?
template <typename T>
inline int lap5_refuse_overlap(const View<T>& in_v, const View<T>& out_v, const int64_t domain[3], int reach, const char* message) {
    const int h[3] = {reach, reach, 0}, h0[3] = {0, 0, 0};
    return views_overlap(in_v, h, h, out_v, h0, h0, domain) ? fail(GT4MI_ERR_UNSUPPORTED, "%s", message) : GT4MI_OK;
}

// The views of `inp` and `out` on a (checked) domain.  `overlap` is what an overlap of the two is refused with; nullptr: not tested
// here -- the caller does it later (lap5_run: behind its empty-domain return; lap5_step_run) or has done it on a larger domain.
template <typename T>
inline int lap5_views(const int64_t domain[3], const gt4mi_field* inp, const gt4mi_field* outf, int reach, const char* overlap,
                      View<T>* in_v, View<T>* out_v) {
    const int h[3] = {reach, reach, 0}, h0[3] = {0, 0, 0};
    if (int rc = make_view<T>("inp", inp, domain, h, h, in_v)) return rc;
    if (int rc = make_view<T>("out", outf, domain, h0, h0, out_v)) return rc;
    return overlap ? lap5_refuse_overlap(*in_v, *out_v, domain, reach, overlap) : GT4MI_OK;
}

// The run-time `variant` as a compile-time constant: f(std::integral_constant<int, GT4MI_LAP_*>{}) -> return code.
template <typename F>
inline int lap5_with_variant(int variant, F&& f) {
    switch (variant) {
        case GT4MI_LAP_NOTEBOOK: return f(std::integral_constant<int, GT4MI_LAP_NOTEBOOK>{});
        case GT4MI_LAP_DOCS: return f(std::integral_constant<int, GT4MI_LAP_DOCS>{});
        case GT4MI_LAP_SUITE: return f(std::integral_constant<int, GT4MI_LAP_SUITE>{});
        case GT4MI_LAP_AVG: return f(std::integral_constant<int, GT4MI_LAP_AVG>{});
        default: return fail(GT4MI_ERR_INVALID_ARGUMENT, "lap5: unknown variant %d", variant);
    }
}

// The interior of a distributed step on whole 16-byte lanes, inside a launch that holds other work too (lap5_push / lap5_edge
// .hip.h): the strips of lap5_strip_kernel, `tpb` tiles of lap5_tile_lanes lanes to a 256-thread workgroup.
struct Lap5InteriorTiling {
    int tpb;           // tiles per workgroup: 4 / 2 / 1
    unsigned tx, ty;   // tiles along I and J of one level
    int64_t tiles;     // of all levels
    int64_t interior;  // workgroups
};

template <typename T>
inline Lap5InteriorTiling lap5_interior_tiling(int64_t di, int64_t rows, int64_t dk) {
    constexpr int VMAX = 16 / (int)sizeof(T);
    Lap5InteriorTiling t;
    const int lanes = lap5_tile_lanes(di / VMAX);
    t.tpb = 256 / lanes;
    t.tx = (unsigned)cdiv(di, (int64_t)lanes * VMAX);
    t.ty = (unsigned)cdiv(rows > 0 ? rows : 0, (int64_t)Lap5Tuning::LJ);
    t.tiles = (int64_t)t.tx * t.ty * dk;
    t.interior = cdiv(t.tiles, (int64_t)t.tpb);
    return t;
}

template <typename T, typename W>
inline int lap5_run(const int64_t domain[3], const gt4mi_field* inp, const gt4mi_field* outf,
                    int variant, hipStream_t stream) {
    if (int rc = check_domain(domain)) return rc;
    View<T> in_v, out_v;
    if (int rc = lap5_views<T>(domain, inp, outf, 1, nullptr, &in_v, &out_v)) return rc;
    if (empty_domain(domain)) return GT4MI_OK;
    if (int rc = lap5_refuse_overlap(in_v, out_v, domain, 1,
                                     "lap5: 'inp' and 'out' overlap in memory; every point reads its neighbours' OLD values (the "
                                     "reference evaluates the right-hand side before it assigns), which an in-place kernel cannot "
                                     "provide -- pass a separate output array"))
        return rc;
    if (int rc = lap5_with_variant(variant, [&](auto v) {
            return lap5_launch_variant<T, W, decltype(v)::value>(const_view(in_v), out_v, domain, stream);
        }))
        return rc;
    GT4MI_HIP_CHECK(hipGetLastError());
    return GT4MI_OK;
}

}  // namespace gt4mi
