// Layout-converting field copy: the box [origin, origin + extent) of up to 8 (dst, src) pairs, ONE launch.
//
// NEW component: gt4py.cartesian moves fields in and out of its numpy / cupy storages with slicing and `cp.asarray`; the
// storages of this backend are DeviceArrays in an I-contiguous, row-padded layout, and a generic strided copy between that
// layout and a K-fastest (numpy C order) buffer is a full 3-d transpose by a kernel that knows neither layout.
//
// Every pair has its own pointers, strides and origins on both sides, and any layout; the host picks one of three paths per
// pair from its strides and alignment (blockIdx.y = pair, a block works on ONE pair and one path):
//   ROWS   both sides have unit item stride along the same axis.  Unit = one 16-byte lane of one row where both sides allow it
//          (equal item sizes, the other strides multiples of 16 bytes and both rows equally far from a 16-byte boundary: the
//          `lead` idea of halo_fill.hip.h, the lanes start `lead` items into the row and the partial lanes at both ends go item
//          by item), else one item.  A thread takes four units 256 apart: the loads are issued before the first store.
//   TILES  the two sides have unit stride along DIFFERENT axes (ifirst <-> kfirst, ifirst <-> jfirst, jfirst <-> kfirst).  A
//          workgroup moves one T x T tile over A (src's fast axis) and B (dst's fast axis) at one index of the third axis C
//          through LDS: it reads rows along A (consecutive lanes on consecutive items: coalesced), and after ONE barrier
//          writes rows along B (coalesced again).  T = 64 items (32 for 8-byte items): rows of 256 bytes for 4- and 8-byte items.
//          Edge tiles are predicated.  Tiles are numbered with B innermost and dst's slowest axis outermost, so that the
//          workgroups in flight write a nearly sequential stream.
//   ITEMS  everything else (no unit stride on an axis longer than 1 on one side, a broadcast src of stride 0): one item per
//          unit, numbered in the order of dst's strides.
//
// WHY ONE BARRIER AND NO ORDERING BETWEEN WORKGROUPS: the host refuses a call in which the bytes of any dst meet the bytes of
// any src or of another dst, so no workgroup reads what any workgroup writes, and every destination item is written by
// exactly one thread of one workgroup.  Inside a tile the only hand-over is the LDS tile: written once, barrier, read once.
//
// LDS PITCH (64 banks of 4 bytes; conflicts count per 32-lane half for 4-byte reads, per pair of banks for 8-byte reads):
// the tile is stored [b][a] with a pitch of T items plus a pad; the row-wise side (stores along a) is conflict-free by
// construction, the column-wise side (lane l reads [l][a]) walks the banks with the pitch as its stride:
//   4-byte items  pitch 65 dwords: lane l of a half on bank (65 l + a) mod 32 = (l + a) mod 32, 32 lanes on 32 banks;
//   8-byte items  pitch 33 items = 66 dwords: lane l on the bank PAIR (33 l + a) mod 32 = (l + a) mod 32, 32 pairs of 64 banks;
//   2- / 1-byte   pitch 64 items + 4 bytes = 33 / 17 dwords, odd: lane l on dword bank (33 l | 17 l + a / 2 | a / 4) mod 32, distinct.
// A tile is 16 640 bytes at most (4-byte items), so the 160 KiB of a CU hold more workgroups than its wave slots (8 of 256 lanes).
//
// Loads are nontemporal (the source is read once), stores plain (a stencil reads the result next).  Equal item sizes move
// bit patterns; float64 -> float32 is the ONE double -> float rounding (to nearest even) the kernel library stores through
// everywhere, float32 -> float64 is exact.  No synchronisation, allocation, atomics, flags, spinning or scratch.
#pragma once

#include "common.hip.h"
#include "field_args.hip.h"
#include "halo.hip.h"

namespace gt4mi {

constexpr int FIELD_COPY_MAX_PAIRS = 8;
constexpr int FIELD_COPY_UNROLL = 4;  // units per thread on the ROWS and ITEMS paths
enum { FIELD_COPY_LANES = 0, FIELD_COPY_TILES = 1, FIELD_COPY_ITEMS = 2 };  // what a block of the kernel does

// The axes are PERMUTED per pair by the host (n, d, s below are in the kernel's order, strides in ITEMS of their side):
//   LANES  0 = the common fast axis (d[0] = s[0] = 1), 1 and 2 = the others, dst's smaller stride first
//   TILES  0 = A, src's fast axis (s[0] = 1), 1 = B, dst's fast axis (d[1] = 1), 2 = C
//   ITEMS  the order of dst's strides, smallest first (a ROWS pair that goes item by item: the fast axis first)
struct CopyPair {
    char* dst;        // first item of the box
    const char* src;
    int64_t d[3], s[3];
    int n[3];
    int mode;         // FIELD_COPY_*
    int lead;         // LANES: items from a row's first item to the first 16-byte boundary
    unsigned lanes;   // LANES: 16-byte lanes of a row (partial ones included)
    int c_outer;      // TILES: 1 = C is dst's slowest axis (tiles: B, A, C from the inside), 0 = A is (B, C, A)
};

struct CopyArgs {
    CopyPair f[FIELD_COPY_MAX_PAIRS];
};

template <typename D, typename S>
__device__ __forceinline__ D field_copy_item(S v) {
    return (D)v;  // (equal types: the bits; double -> float: one rounding to nearest even; float -> double: exact)
}

template <typename D, typename S>
__global__ void __launch_bounds__(256)
field_copy_kernel(const CopyArgs a) {
    constexpr int T = (sizeof(D) > 4 || sizeof(S) > 4) ? 32 : 64;
    constexpr int PAD = sizeof(D) >= 4 ? 1 : 4 / (int)sizeof(D);
    constexpr int ROWS_PER_PASS = 256 / T, PASSES = T / ROWS_PER_PASS;
    __shared__ D tile[T][T + PAD];
    // (selected with scalar moves: indexing the by-value argument block with blockIdx.y makes the compiler copy it to scratch)
    CopyPair f = a.f[0];
#pragma unroll
    for (int n = 1; n < FIELD_COPY_MAX_PAIRS; ++n)
        if (blockIdx.y == (unsigned)n) f = a.f[n];
    D* const dst = reinterpret_cast<D*>(f.dst);
    const S* const src = reinterpret_cast<const S*>(f.src);

    if (f.mode == FIELD_COPY_TILES) {
        const unsigned ta_n = ((unsigned)f.n[0] + T - 1) / T, tb_n = ((unsigned)f.n[1] + T - 1) / T;
        unsigned t = blockIdx.x;
        if (t >= ta_n * tb_n * (unsigned)f.n[2]) return;  // (a pair with fewer tiles than the grid was sized for; whole blocks leave)
        const unsigned tb = t % tb_n;
        t /= tb_n;
        unsigned ta, c;
        if (f.c_outer) ta = t % ta_n, c = t / ta_n;
        else c = t % (unsigned)f.n[2], ta = t / (unsigned)f.n[2];
        const int a0 = (int)ta * T, b0 = (int)tb * T;
        const int x = (int)threadIdx.x % T, y = (int)threadIdx.x / T;
        const S* const sp = src + (int64_t)c * f.s[2];
        D* const dp = dst + (int64_t)c * f.d[2];
        S v[PASSES];
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {  // rows along A: all loads in flight, then the tile
            const int b = y + p * ROWS_PER_PASS;
            if (a0 + x < f.n[0] && b0 + b < f.n[1]) v[p] = __builtin_nontemporal_load(sp + (a0 + x) + (int64_t)(b0 + b) * f.s[1]);
        }
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {
            const int b = y + p * ROWS_PER_PASS;
            if (a0 + x < f.n[0] && b0 + b < f.n[1]) tile[b][x] = field_copy_item<D, S>(v[p]);
        }
        __syncthreads();
#pragma unroll
        for (int p = 0; p < PASSES; ++p) {  // rows along B
            const int aa = y + p * ROWS_PER_PASS;
            if (b0 + x < f.n[1] && a0 + aa < f.n[0]) dp[(int64_t)(a0 + aa) * f.d[0] + (b0 + x)] = tile[x][aa];
        }
        return;
    }

    const unsigned first = blockIdx.x * (256u * FIELD_COPY_UNROLL) + threadIdx.x;
    if constexpr (sizeof(D) == sizeof(S)) {
        if (f.mode == FIELD_COPY_LANES) {
            constexpr int V = 16 / (int)sizeof(D);
            const unsigned total = f.lanes * (unsigned)f.n[1] * (unsigned)f.n[2];
            u32x4 v[FIELD_COPY_UNROLL];
            const S* from[FIELD_COPY_UNROLL];
            D* to[FIELD_COPY_UNROLL];
            int e0[FIELD_COPY_UNROLL];
#pragma unroll
            for (int u = 0; u < FIELD_COPY_UNROLL; ++u) {
                const unsigned unit = first + (unsigned)u * 256u;
                e0[u] = INT32_MIN;  // no unit
                if (unit >= total) continue;
                const unsigned row = unit / f.lanes, lane = unit - row * f.lanes;
                const unsigned r2 = row / (unsigned)f.n[1], r1 = row - r2 * (unsigned)f.n[1];
                from[u] = src + (int64_t)r1 * f.s[1] + (int64_t)r2 * f.s[2];
                to[u] = dst + (int64_t)r1 * f.d[1] + (int64_t)r2 * f.d[2];
                // lane x covers the items [e0, e0 + V) cut to [0, n); with lead > 0 lane 0 is the partial one in front
                e0[u] = f.lead > 0 ? f.lead + ((int)lane - 1) * V : (int)lane * V;
                if (e0[u] >= 0 && e0[u] + V <= f.n[0]) v[u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(from[u] + e0[u]));
            }
#pragma unroll
            for (int u = 0; u < FIELD_COPY_UNROLL; ++u) {
                if (e0[u] == INT32_MIN) continue;
                if (e0[u] >= 0 && e0[u] + V <= f.n[0]) {
                    *reinterpret_cast<u32x4*>(to[u] + e0[u]) = v[u];
                } else {
                    const int lo = e0[u] < 0 ? 0 : e0[u], hi = e0[u] + V > f.n[0] ? f.n[0] : e0[u] + V;
                    for (int e = lo; e < hi; ++e) to[u][e] = __builtin_nontemporal_load(from[u] + e);
                }
            }
            return;
        }
    }

    // ---- ITEMS ----
    const unsigned total = (unsigned)f.n[0] * (unsigned)f.n[1] * (unsigned)f.n[2];
    S w[FIELD_COPY_UNROLL];
    int64_t where[FIELD_COPY_UNROLL];
#pragma unroll
    for (int u = 0; u < FIELD_COPY_UNROLL; ++u) {
        const unsigned unit = first + (unsigned)u * 256u;
        where[u] = -1;
        if (unit >= total) continue;
        const unsigned q = unit / (unsigned)f.n[0], i0 = unit - q * (unsigned)f.n[0];
        const unsigned i2 = q / (unsigned)f.n[1], i1 = q - i2 * (unsigned)f.n[1];
        w[u] = __builtin_nontemporal_load(src + (int64_t)i0 * f.s[0] + (int64_t)i1 * f.s[1] + (int64_t)i2 * f.s[2]);
        where[u] = (int64_t)i0 * f.d[0] + (int64_t)i1 * f.d[1] + (int64_t)i2 * f.d[2];
    }
    // (dst strides may be negative, so "no unit" is a flag of its own rather than a negative offset)
#pragma unroll
    for (int u = 0; u < FIELD_COPY_UNROLL; ++u)
        if (first + (unsigned)u * 256u < total) dst[where[u]] = field_copy_item<D, S>(w[u]);
}

const BoxChecks FIELD_COPY_CHECKS = {"field_copy", "extent", "only a src may be broadcast", false, false};

// the axis (of extent > 1) along which a side has unit item stride, -1 = none
inline int field_copy_unit_axis(const gt4mi_field& f, const int64_t extent[3], int elem_size, int other = -1) {
    if (other >= 0 && extent[other] > 1 && f.stride[other] == elem_size) return other;  // (the other side's, if it is one of several)
    for (int ax = 0; ax < 3; ++ax)
        if (extent[ax] > 1 && f.stride[ax] == elem_size) return ax;
    return -1;
}

// path of a pair and its descriptor
inline int field_copy_plan(const gt4mi_field& dst, const gt4mi_field& src, const int64_t extent[3], int dsize, int ssize, CopyPair* out) {
    CopyPair p{};
    p.dst = origin_ptr(dst), p.src = origin_ptr(src);
    int64_t d[3], s[3];
    item_strides(dst, dsize, d), item_strides(src, ssize, s);
    bool broadcast = false;
    for (int ax = 0; ax < 3; ++ax)
        if (extent[ax] > 1 && s[ax] == 0) broadcast = true;
    const int ua_src = field_copy_unit_axis(src, extent, ssize);
    const int ua_dst = field_copy_unit_axis(dst, extent, dsize, ua_src);
    int order[3] = {0, 1, 2};
    int path;
    auto by_dst_stride = [&](int from) {  // order[from..2] ascending in |dst stride|, axes of extent 1 last
        auto key = [&](int ax) { return extent[ax] > 1 ? (d[ax] < 0 ? -d[ax] : d[ax]) : INT64_MAX; };
        for (int x = from; x < 3; ++x)
            for (int y = x + 1; y < 3; ++y)
                if (key(order[y]) < key(order[x])) { const int t = order[x]; order[x] = order[y]; order[y] = t; }
    };
    if (broadcast || ua_src < 0 || ua_dst < 0) {
        path = GT4MI_COPY_PATH_ITEMS;
        p.mode = FIELD_COPY_ITEMS;
        by_dst_stride(0);
    } else if (ua_src == ua_dst) {
        path = GT4MI_COPY_PATH_ROWS;
        order[0] = ua_src, order[1] = (ua_src + 1) % 3, order[2] = (ua_src + 2) % 3;
        by_dst_stride(1);
        p.mode = FIELD_COPY_ITEMS;
        const int V = 16 / dsize;
        const int o1 = order[1], o2 = order[2];
        const bool pitches = (extent[o1] == 1 || (dst.stride[o1] % 16 == 0 && src.stride[o1] % 16 == 0)) &&
                             (extent[o2] == 1 || (dst.stride[o2] % 16 == 0 && src.stride[o2] % 16 == 0));
        const uintptr_t da = reinterpret_cast<uintptr_t>(p.dst) % 16, sa = reinterpret_cast<uintptr_t>(p.src) % 16;
        if (dsize == ssize && V > 1 && pitches && da == sa && extent[ua_src] >= 2 * V) {
            p.mode = FIELD_COPY_LANES;
            p.lead = (int)(((16 - da) % 16) / dsize);
            p.lanes = (unsigned)((p.lead > 0) + cdiv(extent[ua_src] - p.lead, V));
        }
    } else {
        path = GT4MI_COPY_PATH_TILES;
        p.mode = FIELD_COPY_TILES;
        order[0] = ua_src, order[1] = ua_dst, order[2] = 3 - ua_src - ua_dst;
        const int64_t da = d[order[0]] < 0 ? -d[order[0]] : d[order[0]], dc = d[order[2]] < 0 ? -d[order[2]] : d[order[2]];
        p.c_outer = extent[order[2]] == 1 || da <= dc;
    }
    for (int x = 0; x < 3; ++x) p.n[x] = (int)extent[order[x]], p.d[x] = d[order[x]], p.s[x] = s[order[x]];
    *out = p;
    return path;
}

inline int64_t field_copy_blocks(const CopyPair& p, int dsize, int ssize) {
    if (p.mode == FIELD_COPY_TILES) {
        const int T = (dsize > 4 || ssize > 4) ? 32 : 64;
        return cdiv(p.n[0], T) * cdiv(p.n[1], T) * p.n[2];
    }
    const int64_t per_row = p.mode == FIELD_COPY_LANES ? (int64_t)p.lanes : (int64_t)p.n[0];
    return cdiv(per_row * p.n[1] * p.n[2], 256 * FIELD_COPY_UNROLL);
}

// every check, then (unless `flags` carries GT4MI_COPY_DRY_RUN) the launches
inline int field_copy(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const int64_t extent[3], int dsize, int ssize,
                      int flags, hipStream_t stream, int* paths, int* launches) {
    if (launches) *launches = 0;
    if (dst == nullptr || src == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "field_copy: %s is null", dst == nullptr ? "dst" : "src");
    if (nfields < 1) return fail(GT4MI_ERR_INVALID_ARGUMENT, "field_copy: nfields = %d, at least one pair is needed", nfields);
    if (extent == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "field_copy: extent is null");
    for (int ax = 0; ax < 3; ++ax)
        if (extent[ax] < 0 || extent[ax] > INT32_MAX)
            return fail(GT4MI_ERR_INVALID_ARGUMENT, "field_copy: invalid extent %lld along axis %d", (long long)extent[ax], ax);
    if (flags & ~(GT4MI_COPY_CONVERT | GT4MI_COPY_DRY_RUN))
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "field_copy: unknown bits in flags 0x%x", (unsigned)flags);
    const int sizes[2] = {dsize, ssize};
    for (int w = 0; w < 2; ++w)
        if (sizes[w] != 1 && sizes[w] != 2 && sizes[w] != 4 && sizes[w] != 8)
            return fail(GT4MI_ERR_UNSUPPORTED, "field_copy: %s item size %d is not supported (1, 2, 4 or 8 bytes)", w ? "src" : "dst", sizes[w]);
    if (dsize != ssize) {
        if (!(flags & GT4MI_COPY_CONVERT))
            return fail(GT4MI_ERR_UNSUPPORTED, "field_copy: item sizes %d (dst) and %d (src) differ and GT4MI_COPY_CONVERT is not set", dsize, ssize);
        if (dsize + ssize != 12)
            return fail(GT4MI_ERR_UNSUPPORTED, "field_copy: GT4MI_COPY_CONVERT converts float32 <-> float64 only, not item size %d to %d", ssize, dsize);
    }
    for (int n = 0; n < nfields; ++n) {
        if (int rc = check_box_field(FIELD_COPY_CHECKS, "dst", n, dst[n], extent, dsize, true)) return rc;
        if (int rc = check_box_field(FIELD_COPY_CHECKS, "src", n, src[n], extent, ssize, false)) return rc;
    }
    const bool empty = extent[0] == 0 || extent[1] == 0 || extent[2] == 0;
    if (!empty) {
        if (int rc = check_pairs_disjoint("field_copy", dst, src, nfields, extent, extent, dsize, ssize)) return rc;
        if ((int64_t)extent[0] * extent[1] > INT32_MAX || (int64_t)extent[0] * extent[1] * extent[2] > (int64_t)INT32_MAX - 2048)
            return fail(GT4MI_ERR_UNSUPPORTED, "field_copy: too many items for one launch");
    }
    // (paths are reported for an empty box too: they depend on strides and extents alone)
    CopyPair pair;
    if (paths)
        for (int n = 0; n < nfields; ++n) paths[n] = field_copy_plan(dst[n], src[n], extent, dsize, ssize, &pair);
    if (empty) return GT4MI_OK;
    if (launches) *launches = (int)cdiv(nfields, FIELD_COPY_MAX_PAIRS);
    if (flags & GT4MI_COPY_DRY_RUN) return GT4MI_OK;
    for (int first = 0; first < nfields; first += FIELD_COPY_MAX_PAIRS) {
        const int nf = nfields - first < FIELD_COPY_MAX_PAIRS ? nfields - first : FIELD_COPY_MAX_PAIRS;
        CopyArgs a{};
        int64_t blocks = 0;
        for (int n = 0; n < nf; ++n) {
            field_copy_plan(dst[first + n], src[first + n], extent, dsize, ssize, &a.f[n]);
            const int64_t b = field_copy_blocks(a.f[n], dsize, ssize);
            if (b > blocks) blocks = b;
        }
        // one grid for all pairs of the chunk, sized for the pair with the most blocks; the surplus blocks of the others leave
        dim3 grid((unsigned)blocks, (unsigned)nf);
        if (dsize == 8 && ssize == 4) hipLaunchKernelGGL((field_copy_kernel<double, float>), grid, dim3(256), 0, stream, a);
        else if (dsize == 4 && ssize == 8) hipLaunchKernelGGL((field_copy_kernel<float, double>), grid, dim3(256), 0, stream, a);
        else if (dsize == 8) hipLaunchKernelGGL((field_copy_kernel<uint64_t, uint64_t>), grid, dim3(256), 0, stream, a);
        else if (dsize == 4) hipLaunchKernelGGL((field_copy_kernel<uint32_t, uint32_t>), grid, dim3(256), 0, stream, a);
        else if (dsize == 2) hipLaunchKernelGGL((field_copy_kernel<uint16_t, uint16_t>), grid, dim3(256), 0, stream, a);
        else hipLaunchKernelGGL((field_copy_kernel<uint8_t, uint8_t>), grid, dim3(256), 0, stream, a);
        GT4MI_HIP_CHECK(hipGetLastError());
    }
    return GT4MI_OK;
}

}  // namespace gt4mi
