// Boundary-condition halo fill: the I/J ghost cells of up to 8 fields from their own compute domain, ONE launch.
//
// NEW component: gt4py.cartesian leaves boundary conditions to slicing on its numpy / cupy storages; the storages of this
// backend are DeviceArrays, where eight slice assignments are eight launches of a generic strided copy.
//
// Semantics (include/gt4py_amd.h, gt4mi_halo_fill): the result equals "the I sides first, then the J sides over the whole
// padded I range" -- numpy.pad's treatment of axes.  Coordinates below are relative to the origin: the domain is
// [0, ni) x [0, nj) x [0, nk), the padded I range [-lo_i, ni + hi_i).
//
// NO READ-AFTER-WRITE HAZARD, hence one launch and no ordering between its workgroups:
//   * what the launch WRITES: the I-face cells (i outside [0, ni) on an active I side, j inside [0, nj)) and the rows of the
//     active J sides (j outside [0, nj), every i of the padded range);
//   * what it READS:  an I-face cell reads (map_i(i), j), and map_i lands in [0, ni) because the widths are bounded by the
//     mode (PERIODIC / SYMMETRIC <= n, REFLECT <= n - 1, checked on the host): a domain cell, never written.  A J-row cell
//     reads (i', map_j(j)) with map_j(j) in [0, nj) for the same reason, and i' = i inside the domain, i' = map_i(i) (a domain
//     cell again) where its I side is active, i' = i where it is not: a ghost column of a domain row whose I side is
//     INACTIVE, which is exactly the set of I-face cells this launch does not write (the caller's content, e.g. a halo
//     exchange that ran before).
//   Every read is a cell the launch leaves alone; values are moved as bit patterns, never computed.
//
// Work units (a block of 256 lanes takes 256 consecutive units of ONE section; blockIdx.y = field):
//   J rows   unit = one 16-byte lane (fields with unit I stride whose rows all sit alike relative to a 16-byte boundary; the
//            `lead` idea of hdiff_jmarch.hip.h: the lanes start `lead` items into the row, a partial lane in front) or one
//            item (any stride) of one ghost row (side, d, k).  A lane whose cells all map straight down the J axis moves 16
//            bytes at once; the lanes that hold corner cells of an active I side, and the partial ones, go item by item.
//   I faces  unit = one domain row of one (side, k): consecutive lanes on consecutive rows, a regular stride of one row
//            pitch across the wave; the lane moves the row's few ghost cells.  The cost is lines touched (one or two at
//            the row's end, plus the far end for PERIODIC), not bytes.
// Plain vector stores: the ghost cells are read by the stencil that follows.  No LDS, no atomics, no scratch.
#pragma once

#include <cstring>

#include "common.hip.h"
#include "field_args.hip.h"
#include "halo.hip.h"

namespace gt4mi {

constexpr int HALO_FILL_MAX_FIELDS = 8;

struct HaloFillField {
    char* origin;        // address of the first compute-domain point
    int64_t si, sj, sk;  // strides in ITEMS
    int lead;            // 16-byte lanes: items from the row's first padded cell to the first 16-byte boundary; -1 = item lanes
    unsigned lanes;      // 16-byte lanes of a J row (partial ones included)
};

struct HaloFillArgs {
    HaloFillField f[HALO_FILL_MAX_FIELDS];
    uint64_t value;            // CONSTANT: the item's bit pattern
    int ni, nj, nk;
    int lo_i, hi_i;            // widths of the padded I range (what a J row spans)
    int act_lo_i, act_hi_i;    // 1 = that I side is selected and mode_i != NONE
    int w_lo_j, w_hi_j;        // ACTIVE J widths (0 = side not selected, or mode_j == NONE)
    int mode_i, mode_j;
    unsigned j_blocks;                   // blocks of the J section (what the field with the most units needs)
    unsigned i_units;                    // units of the I section per field
};

// index inside [0, n) that a cell at distance d >= 1 outside the axis takes its value from
__device__ __forceinline__ int halo_fill_map(int mode, bool low, int d, int n) {
    switch (mode) {
        case GT4MI_HALO_PERIODIC: return low ? n - d : d - 1;
        case GT4MI_HALO_ZERO_GRADIENT: return low ? 0 : n - 1;
        case GT4MI_HALO_SYMMETRIC: return low ? d - 1 : n - d;
        default: return low ? d : n - 1 - d;  // GT4MI_HALO_REFLECT
    }
}

// one cell of a J row: i in the padded I range, source row `src`, destination row `dst` (both at i = 0)
template <typename U>
__device__ __forceinline__ void halo_fill_row_item(const HaloFillArgs& a, const U* src, U* dst, int64_t si, int i) {
    U v;
    int is = i;
    bool constant = a.mode_j == GT4MI_HALO_CONSTANT;
    if (!constant && i < 0 && a.act_lo_i) {
        if (a.mode_i == GT4MI_HALO_CONSTANT) constant = true;
        else is = halo_fill_map(a.mode_i, true, -i, a.ni);
    } else if (!constant && i >= a.ni && a.act_hi_i) {
        if (a.mode_i == GT4MI_HALO_CONSTANT) constant = true;
        else is = halo_fill_map(a.mode_i, false, i - a.ni + 1, a.ni);
    }
    v = constant ? (U)a.value : src[is * si];
    dst[i * si] = v;
}

template <typename U>
__global__ void __launch_bounds__(256)
halo_fill_kernel(const HaloFillArgs a) {
    // (selected with scalar moves: indexing the by-value argument block with blockIdx.y makes the compiler copy it to scratch)
    HaloFillField f = a.f[0];
#pragma unroll
    for (int n = 1; n < HALO_FILL_MAX_FIELDS; ++n)
        if (blockIdx.y == (unsigned)n) f = a.f[n];
    U* const p = reinterpret_cast<U*>(f.origin);
    const bool vec = f.lead >= 0;
    const unsigned j_blocks = a.j_blocks;
    const int L = a.lo_i + a.ni + a.hi_i;
    const int wj = a.w_lo_j + a.w_hi_j;
    if (blockIdx.x < j_blocks) {
        // ---- J rows (corners included) ----
        const unsigned t = blockIdx.x * 256u + threadIdx.x;
        const unsigned per_row = vec ? f.lanes : (unsigned)L;
        if (t >= (unsigned)(wj * a.nk) * per_row) return;  // (a field with fewer units than the grid was sized for)
        const unsigned row = t / per_row, x = t - row * per_row;
        const int k = (int)(row / (unsigned)wj), r = (int)(row - (unsigned)k * wj);
        const bool low = r < a.w_lo_j;
        const int d = low ? r + 1 : r - a.w_lo_j + 1;
        const int jd = low ? -d : a.nj - 1 + d;
        const bool constant = a.mode_j == GT4MI_HALO_CONSTANT;
        const int js = constant ? 0 : halo_fill_map(a.mode_j, low, d, a.nj);
        U* const dst = p + jd * f.sj + k * f.sk;
        const U* const src = p + js * f.sj + k * f.sk;
        if (!vec) {
            halo_fill_row_item<U>(a, src, dst, f.si, (int)x - a.lo_i);
            return;
        }
        constexpr int V = 16 / (int)sizeof(U);
        // lane x covers the padded cells [e0, e0 + V) cut to [0, L); with lead > 0 lane 0 is the partial one in front
        const int e0 = f.lead > 0 ? f.lead + ((int)x - 1) * V : (int)x * V;
        const int i0 = e0 - a.lo_i;
        // cells that map straight down the J axis: the domain and the ghost columns of inactive I sides
        const int s_lo = a.act_lo_i ? 0 : -a.lo_i, s_hi = a.act_hi_i ? a.ni : a.ni + a.hi_i;
        if (e0 >= 0 && e0 + V <= L && (constant || (i0 >= s_lo && i0 + V <= s_hi))) {
            u32x4 v;
            if (constant) {
                uint64_t w = a.value;
                if constexpr (sizeof(U) < 8) w = (w << 32) | (w & 0xffffffffull);  // (the host replicated 1- and 2-byte items)
                v = u32x4{(unsigned)w, (unsigned)(w >> 32), (unsigned)w, (unsigned)(w >> 32)};
            } else {
                v = *reinterpret_cast<const u32x4*>(src + i0);
            }
            *reinterpret_cast<u32x4*>(dst + i0) = v;
        } else {
            const int lo = e0 < 0 ? 0 : e0, hi = e0 + V > L ? L : e0 + V;
            for (int e = lo; e < hi; ++e) halo_fill_row_item<U>(a, src, dst, 1, e - a.lo_i);
        }
        return;
    }
    // ---- I faces ----
    const unsigned t = (blockIdx.x - j_blocks) * 256u + threadIdx.x;
    if (t >= a.i_units) return;
    const unsigned per_side = (unsigned)a.nj * (unsigned)a.nk;
    const unsigned s = t / per_side, q = t - s * per_side;  // s: 0 = the first active side, 1 = the second
    const int k = (int)(q / (unsigned)a.nj), j = (int)(q - (unsigned)k * a.nj);
    const bool low = s == 0 && a.act_lo_i;
    const int w = low ? a.lo_i : a.hi_i;
    U* const row = p + j * f.sj + k * f.sk;
    const bool constant = a.mode_i == GT4MI_HALO_CONSTANT;
    for (int d0 = 1; d0 <= w; d0 += 4) {  // (four independent loads in flight, then their stores)
        U v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (d0 + u <= w) v[u] = constant ? (U)a.value : row[halo_fill_map(a.mode_i, low, d0 + u, a.ni) * f.si];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (d0 + u <= w) row[(low ? -(d0 + u) : a.ni - 1 + d0 + u) * f.si] = v[u];
    }
}

inline const char* halo_fill_mode_name(int mode) {
    static const char* names[] = {"NONE", "PERIODIC", "ZERO_GRADIENT", "SYMMETRIC", "REFLECT", "CONSTANT"};
    return mode >= 0 && mode <= GT4MI_HALO_CONSTANT ? names[mode] : "?";
}

// every check, then (unless `sides` carries GT4MI_HALO_DRY_RUN) the launches; *launches = kernels the call enqueues
inline int halo_fill(const gt4mi_field* fields, int nfields, const int64_t domain[3], const int64_t halo[4], int mode_i,
                     int mode_j, int sides, const void* value, int elem_size, hipStream_t stream, int* launches) {
    if (launches) *launches = 0;
    if (fields == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_fill: fields is null");
    if (nfields < 1) return fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_fill: nfields = %d, at least one field is needed", nfields);
    if (halo == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_fill: halo is null");
    if (int rc = check_domain(domain)) return rc;
    if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8)
        return fail(GT4MI_ERR_UNSUPPORTED, "halo_fill: item size %d is not supported (1, 2, 4 or 8 bytes)", elem_size);
    const int modes[2] = {mode_i, mode_j};
    for (int ax = 0; ax < 2; ++ax)
        if (modes[ax] < GT4MI_HALO_NONE || modes[ax] > GT4MI_HALO_CONSTANT)
            return fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_fill: unknown mode %d for axis %c", modes[ax], "IJ"[ax]);
    const int all_sides = GT4MI_HALO_I_LO | GT4MI_HALO_I_HI | GT4MI_HALO_J_LO | GT4MI_HALO_J_HI;
    if (sides & ~(all_sides | GT4MI_HALO_DRY_RUN))
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_fill: unknown bits in sides 0x%x", (unsigned)sides);
    if ((mode_i == GT4MI_HALO_CONSTANT || mode_j == GT4MI_HALO_CONSTANT) && value == nullptr)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_fill: value is null (mode CONSTANT)");
    for (int h = 0; h < 4; ++h) {
        const int ax = h / 2;
        const int64_t n = domain[ax];
        if (halo[h] < 0 || halo[h] > INT32_MAX / 4)
            return fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_fill: invalid %s width %lld along axis %c", h % 2 ? "high" : "low",
                        (long long)halo[h], "IJ"[ax]);
        const int m = modes[ax];
        if (m != GT4MI_HALO_PERIODIC && m != GT4MI_HALO_SYMMETRIC && m != GT4MI_HALO_REFLECT) continue;  // any width that fits
        const int64_t most = m == GT4MI_HALO_REFLECT ? (n > 0 ? n - 1 : 0) : n;  // numpy.pad iterates beyond; this does not
        if (halo[h] > most)
            return fail(GT4MI_ERR_INVALID_ARGUMENT,
                        "halo_fill: %s width %lld along axis %c is larger than %lld, the most mode %s can take from %lld cells",
                        h % 2 ? "high" : "low", (long long)halo[h], "IJ"[ax], (long long)most, halo_fill_mode_name(m),
                        (long long)n);
    }
    for (int n = 0; n < nfields; ++n) {
        const gt4mi_field& f = fields[n];
        if (f.data == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_fill: field %d is null", n);
        if (reinterpret_cast<uintptr_t>(f.data) % (uintptr_t)elem_size != 0)
            return fail(GT4MI_ERR_UNSUPPORTED, "halo_fill: field %d is not aligned to its item size", n);
        for (int ax = 0; ax < 3; ++ax) {
            if (f.stride[ax] % elem_size != 0)
                return fail(GT4MI_ERR_UNSUPPORTED, "halo_fill: field %d: byte stride %lld along axis %d is not a multiple of the item size",
                            n, (long long)f.stride[ax], ax);
            if (ax < 2 && f.stride[ax] == 0 && f.shape[ax] > 1)
                return fail(GT4MI_ERR_INVALID_ARGUMENT, "halo_fill: field %d has no %c axis (stride 0)", n, "IJ"[ax]);
            const int64_t lo = ax < 2 ? halo[2 * ax] : 0, hi = ax < 2 ? halo[2 * ax + 1] : 0;
            if (f.origin[ax] < lo)
                return fail(GT4MI_ERR_OUT_OF_BOUNDS, "halo_fill: field %d: low width %lld along axis %d is outside the array (origin %lld)",
                            n, (long long)lo, ax, (long long)f.origin[ax]);
            if (f.origin[ax] + domain[ax] + hi > f.shape[ax])
                return fail(GT4MI_ERR_OUT_OF_BOUNDS,
                            "halo_fill: field %d: high width %lld along axis %d is outside the array (shape %lld, origin %lld + domain %lld)",
                            n, (long long)hi, ax, (long long)f.shape[ax], (long long)f.origin[ax], (long long)domain[ax]);
        }
    }
    HaloFillArgs a{};
    a.ni = (int)domain[0], a.nj = (int)domain[1], a.nk = (int)domain[2];
    a.lo_i = (int)halo[0], a.hi_i = (int)halo[1];
    a.act_lo_i = (sides & GT4MI_HALO_I_LO) && mode_i != GT4MI_HALO_NONE && a.lo_i > 0;
    a.act_hi_i = (sides & GT4MI_HALO_I_HI) && mode_i != GT4MI_HALO_NONE && a.hi_i > 0;
    a.w_lo_j = ((sides & GT4MI_HALO_J_LO) && mode_j != GT4MI_HALO_NONE) ? (int)halo[2] : 0;
    a.w_hi_j = ((sides & GT4MI_HALO_J_HI) && mode_j != GT4MI_HALO_NONE) ? (int)halo[3] : 0;
    a.mode_i = mode_i, a.mode_j = mode_j;
    if (a.ni == 0 || a.nj == 0 || a.nk == 0) return GT4MI_OK;  // (ZERO_GRADIENT / CONSTANT around nothing: nothing to take from)
    if (value != nullptr) {  // the item's bits, replicated to 32 bits so that a 16-byte lane can be splatted from two words
        uint64_t bits = 0;
        memcpy(&bits, value, (size_t)elem_size);
        if (elem_size == 1) bits *= 0x01010101ull;
        if (elem_size == 2) bits *= 0x00010001ull;
        a.value = bits;
    }
    const int64_t L = (int64_t)a.lo_i + a.ni + a.hi_i;
    const int64_t rows = (int64_t)(a.w_lo_j + a.w_hi_j) * a.nk;
    const int64_t i_units = (int64_t)(a.act_lo_i + a.act_hi_i) * a.nj * a.nk;
    const int V = 16 / elem_size;
    const int64_t limit = (int64_t)INT32_MAX - 512;
    // (L on its own too: with I faces only, a row longer than an int can index would pass the products below)
    if (L > limit || rows * (L + 1) > limit || i_units > limit || rows > limit)
        return fail(GT4MI_ERR_UNSUPPORTED, "halo_fill: too many ghost cells for one launch");
    a.i_units = (unsigned)i_units;
    const int count = (int)cdiv(nfields, HALO_FILL_MAX_FIELDS);
    if (rows == 0 && i_units == 0) return GT4MI_OK;
    if (launches) *launches = count;
    if (sides & GT4MI_HALO_DRY_RUN) return GT4MI_OK;
    for (int first = 0; first < nfields; first += HALO_FILL_MAX_FIELDS) {
        const int nf = nfields - first < HALO_FILL_MAX_FIELDS ? nfields - first : HALO_FILL_MAX_FIELDS;
        unsigned most_lanes = 0;
        bool any_item = false;
        for (int n = 0; n < nf; ++n) {
            const gt4mi_field& f = fields[first + n];
            HaloFillField& d = a.f[n];
            d.origin = origin_ptr(f);
            d.si = f.stride[0] / elem_size, d.sj = f.stride[1] / elem_size, d.sk = f.stride[2] / elem_size;
            d.lead = -1;
            d.lanes = 0;
            // 16-byte lanes: unit I stride and every row (source and destination alike) equally far from a 16-byte boundary
            if (V > 1 && d.si == 1 && f.stride[1] % 16 == 0 && f.stride[2] % 16 == 0 && L >= 2 * V) {
                const uintptr_t first_cell = reinterpret_cast<uintptr_t>(d.origin) - (uintptr_t)a.lo_i * elem_size;
                d.lead = (int)(((16 - first_cell % 16) % 16) / elem_size);
                d.lanes = (unsigned)((d.lead > 0) + cdiv(L - d.lead, V));
                if (d.lanes > most_lanes) most_lanes = d.lanes;
            } else {
                any_item = true;
            }
        }
        // one grid for all fields of the chunk, sized for the field with the most J units (item lanes need more than 16-byte
        // lanes); the surplus blocks of the others find no unit and leave
        a.j_blocks = (unsigned)cdiv(rows * (any_item ? L : (int64_t)most_lanes), 256);
        const unsigned blocks = a.j_blocks + (unsigned)cdiv(i_units, 256);
        dim3 grid(blocks, (unsigned)nf);
        if (elem_size == 8) hipLaunchKernelGGL((halo_fill_kernel<uint64_t>), grid, dim3(256), 0, stream, a);
        else if (elem_size == 4) hipLaunchKernelGGL((halo_fill_kernel<uint32_t>), grid, dim3(256), 0, stream, a);
        else if (elem_size == 2) hipLaunchKernelGGL((halo_fill_kernel<uint16_t>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((halo_fill_kernel<uint8_t>), grid, dim3(256), 0, stream, a);
        GT4MI_HIP_CHECK(hipGetLastError());
    }
    return GT4MI_OK;
}

}  // namespace gt4mi
