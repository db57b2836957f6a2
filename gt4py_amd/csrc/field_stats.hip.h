// Field statistics: count, non-finite count, sum, sum |x|, sum x*x, min, max and a dot product over the compute domain of up
// to 8 entries per launch, the field read ONCE, the result BIT-REPRODUCIBLE.
//
// NEW component, no reference counterpart: gt4py.cartesian leaves reductions to numpy / cupy on storages that ARE numpy / cupy
// arrays; the storages of this backend are DeviceArrays.
//
// An entry is a field `a` and optionally a second field `b` of the same item type (float or double).  x = a, or with b the
// difference a - b rounded once in double.  ALL arithmetic is double: float items are widened first, so a - b is rounded
// once and the products x*x and a*b of floats are exact.  The contract below needs every product and sum to be rounded on its
// own: it rests on -ffp-contract=off of the build (csrc/Makefile) and on the pragma of common.hip.h.
//
// THE ORDER OF THE ADDITIONS is a function of the domain (ni, nj, nk) alone -- not of pointers, strides, padding, alignment,
// the load path, the number of entries in the launch, the grid, the CUs or the arrival order of workgroups:
//   rows     a row is one (j, k) of the domain, row number r = j + nj * k, rows = nj * nk.
//   tiles    RW = ceil(rows / (4 * 4096)) rows per wave; a tile is 4 * RW consecutive rows, tiles = ceil(rows / (4 * RW)) <= 4096.
//            Wave w (0..3) of tile t takes the rows [(4 t + w) RW, (4 t + w + 1) RW) that exist.
//   lanes    lane l (0..63) of a wave owns the columns i with (i mod 256) div 4 == l.  It keeps ONE set of accumulators (sums
//            start at +0.0, min at +inf, max at -inf) and adds its items in the order (row, i) increasing: for every row of the
//            wave, for every chunk of 256 columns, its 4 columns.  Columns >= ni and rows >= rows add nothing.
//            A lane whose sum |x| ended NaN (an item was NaN: |x| of anything else never adds up to NaN) sets min = max = NaN.
//   wave     a butterfly over the 64 lanes: for s = 1, 2, 4, 8, 16, 32: v[l] = v[l] (+) v[l ^ s] -- the balanced binary tree
//            ((l0 + l1) + (l2 + l3)) + ... ; every lane takes part, also one that owned no column.
//   tile     the 4 wave values left to right: ((w0 + w1) + w2) + w3, through LDS.  The tile's 8 doubles go to the workspace
//            with plain vector stores: partial[(entry * tiles + tile) * 8 + slot].
//   finish   a SECOND kernel on the same stream, one workgroup per entry, nothing shared between workgroups: leaf q (0..127)
//            adds the tiles [q C, (q + 1) C), C = ceil(tiles / 128), left to right starting FROM its first tile (no zero in
//            front); the m = ceil(tiles / C) leaves are then halved level by level: new[i] = old[2i] (+) old[2i + 1], an odd
//            last one is carried up unchanged.
//   (+) is + for the sums and counts, and for min / max the IEEE-754-2019 minimum / maximum: NaN if either is NaN,
//   min(-0, +0) = -0, max(-0, +0) = +0 -- associative and commutative, so min and max do not depend on the order at all.
// The partials cross the launch boundary, the only ordering there is: no float atomics, no ticket, flag or spin, no workgroup
// waits for another.  tests/stats_ref.py restates this order in numpy.
//
// TWO LOAD PATHS, THE SAME ADDITIONS: a lane fetches the 4 items it owns in a chunk either as 16-byte lanes (unit I stride, the
// address of its first item on a 16-byte boundary: true for every lane when the origin column and the J / K strides are
// multiples of 16 bytes, which every `aligned_index` storage gives) or item by item (any stride, 0 for a broadcast weight);
// which one ran changes how the operands reach the registers, not which operands are added to which accumulator in which order.
// Loads are nontemporal (the field is read once, as the library's other read-once streams are: DESIGN.md section 4b).
// LDS: 4 x 8 doubles for the tile combine, 128 x 8 for the finish.  No scratch.
#pragma once

#include <cmath>

#include "common.hip.h"
#include "field_args.hip.h"

namespace gt4mi {

constexpr int STATS_MAX_ENTRIES = 8;
constexpr int STATS_SLOTS = 8;
constexpr int STATS_GROUP = 4;                 // consecutive columns a lane owns in a chunk
constexpr int STATS_CHUNK = 64 * STATS_GROUP;  // columns a wave covers at once
constexpr int STATS_WAVES = 4;
constexpr int STATS_MAX_TILES = 4096;
constexpr int STATS_LEAVES = 128;  // of the finish kernel, 8 slots each = 1024 threads
constexpr int STATS_BATCH = 4;     // chunks a wave has in flight before it adds them (in order)
enum { STATS_COUNT = 0, STATS_NONFINITE = 1, STATS_SUM = 2, STATS_SUM_ABS = 3, STATS_SUM_SQ = 4, STATS_MIN = 5, STATS_MAX = 6, STATS_DOT = 7 };

struct StatsEntry {
    const char* a;  // address of the first compute-domain point
    const char* b;  // nullptr: no second field
    int64_t ai, aj, ak, bi, bj, bk;  // strides in ITEMS (b's may be 0: a broadcast weight)
    int vec;                         // bit 0: `a` takes the 16-byte lanes, bit 1: `b`
};

struct StatsArgs {
    StatsEntry e[STATS_MAX_ENTRIES];
    double* partials;  // of the launch's first entry
    int ni, nj;
    int64_t rows;
    int rows_per_wave;
    unsigned tiles;
};

struct StatsGeometry {
    int64_t rows;
    int rows_per_wave;
    unsigned tiles;
};

inline StatsGeometry stats_geometry(const int64_t domain[3]) {
    StatsGeometry g;
    g.rows = domain[1] * domain[2];
    g.rows_per_wave = (int)cdiv(g.rows, (int64_t)STATS_WAVES * STATS_MAX_TILES);
    g.tiles = (unsigned)cdiv(g.rows, (int64_t)STATS_WAVES * g.rows_per_wave);
    return g;
}

struct StatsAcc {
    double sum, sum_abs, sum_sq, mn, mx, dot;
    unsigned count, nonfinite;
};

// IEEE-754-2019 minimum / maximum (see the header comment)
__device__ __forceinline__ double stats_min(double a, double b) {
    if (a != a || b != b) return __builtin_nan("");
    if (a < b) return a;
    if (b < a) return b;
    return __longlong_as_double(__double_as_longlong(a) | __double_as_longlong(b));  // equal: -0 wins over +0
}
__device__ __forceinline__ double stats_max(double a, double b) {
    if (a != a || b != b) return __builtin_nan("");
    if (a > b) return a;
    if (b > a) return b;
    return __longlong_as_double(__double_as_longlong(a) & __double_as_longlong(b));  // equal: +0 wins over -0
}

__device__ __forceinline__ double stats_combine(int slot, double a, double b) {
    if (slot == STATS_MIN) return stats_min(a, b);
    if (slot == STATS_MAX) return stats_max(a, b);
    return a + b;
}

template <bool PAIR>
__device__ __forceinline__ void stats_item(StatsAcc& s, double a, double b) {
    const double x = PAIR ? a - b : a;
    s.sum = s.sum + x;
    s.sum_abs = s.sum_abs + __builtin_fabs(x);
    const double sq = x * x;
    s.sum_sq = s.sum_sq + sq;
    // NaN items are skipped here (minNum / maxNum) and accounted for after the loop through sum_abs; the order of a zero of
    // either sign against the other is the instruction's (v_min_f64 / v_max_f64: -0 < +0)
    s.mn = __builtin_fmin(s.mn, x);
    s.mx = __builtin_fmax(s.mx, x);
    s.nonfinite += ((unsigned)__double2hiint(x) & 0x7ff00000u) == 0x7ff00000u ? 1u : 0u;
    s.count += 1u;
    if constexpr (PAIR) {
        const double p = a * b;
        s.dot = s.dot + p;
    }
}

// the (up to) 4 items of this lane in one chunk: columns [i0, i0 + nvalid)
template <typename T>
__device__ __forceinline__ void stats_load(const T* row, int64_t si, bool vec, int i0, int nvalid, T (&v)[STATS_GROUP]) {
#pragma unroll
    for (int e = 0; e < STATS_GROUP; ++e) v[e] = (T)0;
    if (vec && nvalid >= STATS_GROUP) {
        constexpr int V = 16 / (int)sizeof(T);  // items of a 16-byte lane
        using Vec = typename VecT<T, V>::type;
#pragma unroll
        for (int h = 0; h < STATS_GROUP / V; ++h) {
            const Vec x = __builtin_nontemporal_load(reinterpret_cast<const Vec*>(row + i0) + h);
#pragma unroll
            for (int e = 0; e < V; ++e) v[h * V + e] = x[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < STATS_GROUP; ++e)
            if (e < nvalid) v[e] = __builtin_nontemporal_load(row + (int64_t)(i0 + e) * si);
    }
}

// everything one wave adds: its rows, chunk by chunk, STATS_BATCH chunks in flight
template <typename T, bool PAIR>
__device__ __forceinline__ void stats_wave(int ni, int nj, const StatsEntry& f, int64_t row0, int nrows, int lane, StatsAcc& s) {
    const int chunks = (ni + STATS_CHUNK - 1) / STATS_CHUNK;
    int k = (int)(row0 / nj), j = (int)(row0 - (int64_t)k * nj), c = 0;
    const T* const A = reinterpret_cast<const T*>(f.a);
    const T* const B = reinterpret_cast<const T*>(f.b);
    for (int64_t left = (int64_t)nrows * chunks; left > 0; left -= STATS_BATCH) {
        T va[STATS_BATCH][STATS_GROUP], vb[STATS_BATCH][STATS_GROUP];
        int nvalid[STATS_BATCH];
#pragma unroll
        for (int u = 0; u < STATS_BATCH; ++u) {
            nvalid[u] = 0;
            if (u < left) {
                const int i0 = c * STATS_CHUNK + lane * STATS_GROUP;
                const int n = ni - i0;
                nvalid[u] = n < 0 ? 0 : (n > STATS_GROUP ? STATS_GROUP : n);
                stats_load<T>(A + (int64_t)j * f.aj + (int64_t)k * f.ak, f.ai, (f.vec & 1) != 0, i0, nvalid[u], va[u]);
                if constexpr (PAIR)
                    stats_load<T>(B + (int64_t)j * f.bj + (int64_t)k * f.bk, f.bi, (f.vec & 2) != 0, i0, nvalid[u], vb[u]);
                if (++c == chunks) {
                    c = 0;
                    if (++j == nj) j = 0, ++k;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < STATS_BATCH; ++u) {
            if (__builtin_amdgcn_ballot_w64(nvalid[u] != STATS_GROUP) == 0) {  // a whole chunk: no lane masks
#pragma unroll
                for (int e = 0; e < STATS_GROUP; ++e) stats_item<PAIR>(s, (double)va[u][e], PAIR ? (double)vb[u][e] : 0.0);
            } else {
#pragma unroll
                for (int e = 0; e < STATS_GROUP; ++e)
                    if (e < nvalid[u]) stats_item<PAIR>(s, (double)va[u][e], PAIR ? (double)vb[u][e] : 0.0);
            }
        }
    }
}

__device__ __forceinline__ void stats_init(StatsAcc& s) {
    s.sum = s.sum_abs = s.sum_sq = s.dot = 0.0;
    s.mn = __builtin_inf();
    s.mx = -__builtin_inf();
    s.count = s.nonfinite = 0u;
}

// the end of a lane's chain (a NaN item makes min and max NaN), then the butterfly over the 64 lanes
__device__ __forceinline__ void stats_butterfly(StatsAcc& s) {
    if (s.sum_abs != s.sum_abs) s.mn = s.mx = __builtin_nan("");
#pragma unroll
    for (int step = 1; step < 64; step <<= 1) {
        s.sum = s.sum + __shfl_xor(s.sum, step, 64);
        s.sum_abs = s.sum_abs + __shfl_xor(s.sum_abs, step, 64);
        s.sum_sq = s.sum_sq + __shfl_xor(s.sum_sq, step, 64);
        s.dot = s.dot + __shfl_xor(s.dot, step, 64);
        s.mn = stats_min(s.mn, __shfl_xor(s.mn, step, 64));
        s.mx = stats_max(s.mx, __shfl_xor(s.mx, step, 64));
        s.count += (unsigned)__shfl_xor((int)s.count, step, 64);
        s.nonfinite += (unsigned)__shfl_xor((int)s.nonfinite, step, 64);
    }
}

// a wave's eight values into its row of the workgroup's LDS block (every lane holds them after the butterfly)
__device__ __forceinline__ void stats_wave_values(const StatsAcc& s, double* w) {
    w[STATS_COUNT] = (double)s.count, w[STATS_NONFINITE] = (double)s.nonfinite;
    w[STATS_SUM] = s.sum, w[STATS_SUM_ABS] = s.sum_abs, w[STATS_SUM_SQ] = s.sum_sq;
    w[STATS_MIN] = s.mn, w[STATS_MAX] = s.mx, w[STATS_DOT] = s.dot;
}

template <typename T>
__global__ void __launch_bounds__(64 * STATS_WAVES)
field_stats_kernel(const StatsArgs g) {
    __shared__ double wave_values[STATS_WAVES][STATS_SLOTS];
    // (selected with scalar moves: indexing the by-value argument block with blockIdx.y makes the compiler copy it to scratch)
    StatsEntry f = g.e[0];
#pragma unroll
    for (int n = 1; n < STATS_MAX_ENTRIES; ++n)
        if (blockIdx.y == (unsigned)n) f = g.e[n];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const int64_t row0 = ((int64_t)blockIdx.x * STATS_WAVES + wave) * g.rows_per_wave;
    const int64_t rest = g.rows - row0;
    const int nrows = rest <= 0 ? 0 : (rest < g.rows_per_wave ? (int)rest : g.rows_per_wave);
    StatsAcc s;
    stats_init(s);
    if (f.b != nullptr) stats_wave<T, true>(g.ni, g.nj, f, row0, nrows, lane, s);
    else stats_wave<T, false>(g.ni, g.nj, f, row0, nrows, lane, s);
    stats_butterfly(s);
    if (lane == 0) stats_wave_values(s, wave_values[wave]);
    __syncthreads();
    if (threadIdx.x < (unsigned)STATS_SLOTS) {  // the four waves, left to right; 8 lanes store the tile's 64 bytes
        const int slot = (int)threadIdx.x;
        double v = wave_values[0][slot];
#pragma unroll
        for (int w = 1; w < STATS_WAVES; ++w) v = stats_combine(slot, v, wave_values[w][slot]);
        g.partials[((size_t)blockIdx.y * g.tiles + blockIdx.x) * STATS_SLOTS + slot] = v;
    }
}

// one workgroup per entry: leaves of C consecutive tiles, then the halving tree (header comment)
__global__ void __launch_bounds__(STATS_LEAVES * STATS_SLOTS)
field_stats_finish_kernel(const double* __restrict__ partials, double* __restrict__ result, unsigned tiles) {
    __shared__ double level[STATS_SLOTS][STATS_LEAVES];
    const int slot = (int)(threadIdx.x % STATS_SLOTS), q = (int)(threadIdx.x / STATS_SLOTS);
    const double* const p = partials + (size_t)blockIdx.x * tiles * STATS_SLOTS;
    const unsigned per_leaf = (tiles + STATS_LEAVES - 1) / STATS_LEAVES;
    const unsigned first = (unsigned)q * per_leaf;
    if (first < tiles) {
        const unsigned last = first + per_leaf < tiles ? first + per_leaf : tiles;
        double v = p[(size_t)first * STATS_SLOTS + slot];
        for (unsigned t = first + 1; t < last; ++t) v = stats_combine(slot, v, p[(size_t)t * STATS_SLOTS + slot]);
        level[slot][q] = v;
    }
    __syncthreads();
    for (int n = (int)((tiles + per_leaf - 1) / per_leaf); n > 1; n = (n + 1) >> 1) {
        const int half = n >> 1;
        const bool pair = q < half, carry = (n & 1) && q == half;
        double x = 0.0, y = 0.0;
        if (pair) x = level[slot][2 * q], y = level[slot][2 * q + 1];
        else if (carry) x = level[slot][n - 1];
        __syncthreads();
        if (pair) level[slot][q] = stats_combine(slot, x, y);
        else if (carry) level[slot][q] = x;
        __syncthreads();
    }
    if (q == 0) result[(size_t)blockIdx.x * STATS_SLOTS + slot] = level[slot][0];
}

// 16-byte lanes for a field: unit I stride, every lane's first item (a multiple of 4 columns from the origin) on a 16-byte boundary
inline bool stats_vec_ok(const gt4mi_field& f, const char* origin, int elem_size) {
    return f.stride[0] == elem_size && reinterpret_cast<uintptr_t>(origin) % 16 == 0 && f.stride[1] % 16 == 0 && f.stride[2] % 16 == 0;
}

// the descriptor of one entry: field `f` and, unless null, the second field `o`
inline void stats_fill_entry(StatsEntry& d, const gt4mi_field& f, const gt4mi_field* o, int elem_size) {
    d = StatsEntry{};
    d.a = origin_ptr(f);
    d.ai = f.stride[0] / elem_size, d.aj = f.stride[1] / elem_size, d.ak = f.stride[2] / elem_size;
    d.vec = stats_vec_ok(f, d.a, elem_size) ? 1 : 0;
    if (o == nullptr) return;
    d.b = origin_ptr(*o);
    d.bi = o->stride[0] / elem_size, d.bj = o->stride[1] / elem_size, d.bk = o->stride[2] / elem_size;
    d.vec |= stats_vec_ok(*o, d.b, elem_size) ? 2 : 0;
}

// the second field of entry n, null if there is none (others == NULL, or a descriptor with data == NULL)
inline const gt4mi_field* stats_other(const gt4mi_field* others, int n) {
    return others != nullptr && others[n].data != nullptr ? &others[n] : nullptr;
}

inline BoxChecks stats_checks(const char* entry) { return BoxChecks{entry, "domain", "only a second field may be broadcast", true, false}; }

// the fields of a call: `field` n must exist, `other` n is checked where there is one and may be broadcast along any axis
inline int stats_check_fields(const char* entry, const gt4mi_field* fields, const gt4mi_field* others, int nfields, const int64_t domain[3],
                              int elem_size) {
    const BoxChecks checks = stats_checks(entry);
    for (int n = 0; n < nfields; ++n) {
        if (int rc = check_box_field(checks, "field", n, fields[n], domain, elem_size, true)) return rc;
        if (const gt4mi_field* o = stats_other(others, n))
            if (int rc = check_box_field(checks, "other", n, *o, domain, elem_size, false, 7)) return rc;
    }
    return GT4MI_OK;
}

// workspace (`needed` bytes) and result (`result_bytes`): there unless the call is a dry run, large enough, aligned to 8 bytes,
// clear of every field and of each other.  (A dry run without buffers asks for the workspace size; buffers that are passed
// are checked in either case.)
inline int stats_check_buffers(const char* entry, const gt4mi_field* fields, const gt4mi_field* others, int nfields, const int64_t domain[3],
                               int elem_size, const void* workspace, int64_t workspace_bytes, int64_t needed, const void* result,
                               int64_t result_bytes, bool dry) {
    if (!dry && (workspace == nullptr || result == nullptr))
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: %s is null", entry, workspace == nullptr ? "workspace" : "result");
    if (workspace != nullptr && workspace_bytes < needed)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: workspace of %lld bytes is too small, %lld are needed", entry, (long long)workspace_bytes,
                    (long long)needed);
    const ByteSpan spans[2] = {
        ByteSpan{reinterpret_cast<uintptr_t>(workspace), reinterpret_cast<uintptr_t>(workspace) + (uintptr_t)needed},
        ByteSpan{reinterpret_cast<uintptr_t>(result), reinterpret_cast<uintptr_t>(result) + (uintptr_t)result_bytes}};
    const char* const names[2] = {"workspace", "result"};
    for (int w = 0; w < 2; ++w) {
        if (spans[w].lo == 0) continue;
        if (spans[w].lo % 8 != 0) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: %s is not aligned to 8 bytes", entry, names[w]);
        for (int n = 0; n < nfields; ++n) {
            if (spans_overlap(spans[w], box_span(fields[n], domain, elem_size)))
                return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: %s overlaps field %d", entry, names[w], n);
            if (const gt4mi_field* o = stats_other(others, n))
                if (spans_overlap(spans[w], box_span(*o, domain, elem_size)))
                    return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: %s overlaps other %d", entry, names[w], n);
        }
    }
    if (workspace != nullptr && result != nullptr && spans_overlap(spans[0], spans[1]))
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: workspace overlaps result", entry);
    return GT4MI_OK;
}

// every check, then (unless `flags` carries GT4MI_STATS_DRY_RUN) the launches; *launches = kernels the call enqueues
inline int field_stats(const gt4mi_field* fields, const gt4mi_field* others, int nfields, const int64_t domain[3], int elem_size,
                       void* workspace, int64_t workspace_bytes, double* result, int flags, hipStream_t stream,
                       int64_t* workspace_needed, int* launches) {
    if (launches) *launches = 0;
    if (workspace_needed) *workspace_needed = 0;
    if (fields == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "field_stats: fields is null");
    if (nfields < 1) return fail(GT4MI_ERR_INVALID_ARGUMENT, "field_stats: nfields = %d, at least one field is needed", nfields);
    if (int rc = check_domain(domain)) return rc;
    for (int ax = 0; ax < 3; ++ax)
        if (domain[ax] < 1) return fail(GT4MI_ERR_INVALID_ARGUMENT, "field_stats: empty domain (%lld along axis %d)", (long long)domain[ax], ax);
    if (elem_size != 4 && elem_size != 8)
        return fail(GT4MI_ERR_UNSUPPORTED, "field_stats: item size %d is not supported (float32 or float64 fields)", elem_size);
    if (flags & ~GT4MI_STATS_DRY_RUN) return fail(GT4MI_ERR_INVALID_ARGUMENT, "field_stats: unknown bits in flags 0x%x", (unsigned)flags);
    const bool dry = (flags & GT4MI_STATS_DRY_RUN) != 0;
    if ((double)domain[0] * (double)domain[1] * (double)domain[2] > 1099511627776.0)  // 2^40: the lanes count in 32 bits
        return fail(GT4MI_ERR_UNSUPPORTED, "field_stats: more than 2^40 points in the domain");
    if (int rc = stats_check_fields("field_stats", fields, others, nfields, domain, elem_size)) return rc;
    const StatsGeometry geo = stats_geometry(domain);
    const int64_t needed = (int64_t)nfields * geo.tiles * STATS_SLOTS * (int64_t)sizeof(double);
    if (workspace_needed) *workspace_needed = needed;
    if (int rc = stats_check_buffers("field_stats", fields, others, nfields, domain, elem_size, workspace, workspace_bytes, needed, result,
                                     (int64_t)nfields * STATS_SLOTS * (int64_t)sizeof(double), dry))
        return rc;
    const int count = (int)cdiv(nfields, STATS_MAX_ENTRIES) + 1;
    if (launches) *launches = count;
    if (dry) return GT4MI_OK;
    StatsArgs a{};
    a.ni = (int)domain[0], a.nj = (int)domain[1];
    a.rows = geo.rows, a.rows_per_wave = geo.rows_per_wave, a.tiles = geo.tiles;
    for (int first = 0; first < nfields; first += STATS_MAX_ENTRIES) {
        const int nf = nfields - first < STATS_MAX_ENTRIES ? nfields - first : STATS_MAX_ENTRIES;
        for (int n = 0; n < nf; ++n) stats_fill_entry(a.e[n], fields[first + n], stats_other(others, first + n), elem_size);
        a.partials = static_cast<double*>(workspace) + (size_t)first * geo.tiles * STATS_SLOTS;
        const dim3 grid(geo.tiles, (unsigned)nf);
        if (elem_size == 8) hipLaunchKernelGGL((field_stats_kernel<double>), grid, dim3(64 * STATS_WAVES), 0, stream, a);
        else hipLaunchKernelGGL((field_stats_kernel<float>), grid, dim3(64 * STATS_WAVES), 0, stream, a);
        GT4MI_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(field_stats_finish_kernel, dim3((unsigned)nfields), dim3(STATS_LEAVES * STATS_SLOTS), 0, stream,
                       static_cast<const double*>(workspace), result, geo.tiles);
    GT4MI_HIP_CHECK(hipGetLastError());
    return GT4MI_OK;
}

}  // namespace gt4mi
