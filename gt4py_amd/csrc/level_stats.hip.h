// Per-level statistics (K profiles): the eight slots of field_stats.hip.h over the plane (ni, nj) of EVERY level k of the
// domain, plus the horizontal mean, for up to 8 entries per launch, the field read ONCE, the result BIT-REPRODUCIBLE and left on
// the device as contiguous runs of nk doubles -- what a stencil takes as Field[K, float64].
//
// NEW component, no reference counterpart: GTScript has no reduction over I and J; gt4py.cartesian leaves it to numpy / cupy
// (`field.sum(axis=(0, 1))`) on storages that ARE numpy / cupy arrays.
//
// Entries, x = a or a - b, the slots, the NaN and signed-zero rules and the all-double arithmetic are those of
// field_stats.hip.h, whose device functions (StatsAcc, stats_item, stats_load, stats_wave, stats_butterfly, stats_min /
// stats_max / stats_combine) do the work here too.
//
// THE ORDER OF THE ADDITIONS OF LEVEL k is a function of (ni, nj) alone -- not of nk or of which level it is, not of pointers,
// strides, padding, alignment, the load path, the number of entries in the call, the grid or the arrival order of workgroups:
//   rows     a row of a level is one j.  RW = ceil(nj / (4 * LT)) rows per wave, LT = LEVEL_STATS_MAX_TILES; a tile is 4 waves,
//            TL = ceil(nj / (4 * RW)) <= LT tiles per level.  Wave w of tile t takes the rows [(4 t + w) RW, (4 t + w + 1) RW)
//            that exist.
//   lanes, wave, tile
//            exactly as field_stats: lane l owns the columns with (i mod 256) div 4 == l and adds them from +0.0 in (row, i)
//            order; a lane whose sum |x| is NaN sets min = max = NaN; the butterfly s = 1 ... 32; the four waves left to right
//            through LDS.  The tile's 8 doubles go to the workspace with plain stores:
//            partial[((entry * nk + k) * TL + t) * 8 + slot].
//   finish   a SECOND kernel on the same stream, one thread per (entry, level, slot): it loads the TL tile values of its level
//            (all loads issued before the first addition), halves them level by level in registers,
//            new[i] = old[2i] (+) old[2i + 1], an odd last one carried up unchanged -- no leaf chain -- and stores
//            result[(entry * 9 + slot) * nk + k]; the thread of SUM also stores row 8, mean = SUM / COUNT, one IEEE division.
// The partials cross the launch boundary, the only ordering there is: no float atomics, no ticket, flag or spin, no workgroup
// waits for another.  tests/level_stats_ref.py restates this order in numpy.
//
// GRID: tile fastest, then level, flattened into blockIdx.x (no 65 535 limit; the workgroups in flight read a nearly
// sequential stream of an I-contiguous field); the entry is blockIdx.y.  Loads are nontemporal.  LDS: 4 x 8 doubles for the
// tile combine.  No scratch.
#pragma once

#include "field_stats.hip.h"

namespace gt4mi {

constexpr int LEVEL_STATS_MAX_TILES = GT4MI_LEVEL_STATS_MAX_TILES;  // LT: part of the bit contract
constexpr int LEVEL_STATS_ROWS = GT4MI_LEVEL_STATS_ROWS;
constexpr int LEVEL_STATS_FINISH_THREADS = 64;
constexpr int64_t LEVEL_STATS_MAX_WORKGROUPS = (int64_t)1 << 24;  // grid.x * 256 threads stays below 2^32
static_assert(LEVEL_STATS_MAX_TILES >= 1 && (LEVEL_STATS_MAX_TILES & (LEVEL_STATS_MAX_TILES - 1)) == 0, "LT is a power of two");
static_assert(LEVEL_STATS_ROWS == STATS_SLOTS + 1 && GT4MI_LEVEL_STATS_MEAN == STATS_SLOTS, "row 8 is the mean");

struct LevelStatsArgs {
    StatsEntry e[STATS_MAX_ENTRIES];
    double* partials;  // of the launch's first entry
    int ni, nj, nk;
    int rows_per_wave;
    unsigned tiles;  // per level
};

struct LevelStatsGeometry {
    int rows_per_wave;
    unsigned tiles;
};

inline LevelStatsGeometry level_stats_geometry(const int64_t domain[3]) {
    LevelStatsGeometry g;
    g.rows_per_wave = (int)cdiv(domain[1], (int64_t)STATS_WAVES * LEVEL_STATS_MAX_TILES);
    g.tiles = (unsigned)cdiv(domain[1], (int64_t)STATS_WAVES * g.rows_per_wave);
    return g;
}

template <typename T>
__global__ void __launch_bounds__(64 * STATS_WAVES)
level_stats_kernel(const LevelStatsArgs g) {
    __shared__ double wave_values[STATS_WAVES][STATS_SLOTS];
    // (selected with scalar moves: indexing the by-value argument block with blockIdx.y makes the compiler copy it to scratch)
    StatsEntry f = g.e[0];
#pragma unroll
    for (int n = 1; n < STATS_MAX_ENTRIES; ++n)
        if (blockIdx.y == (unsigned)n) f = g.e[n];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const unsigned k = blockIdx.x / g.tiles, tile = blockIdx.x - k * g.tiles;
    const int j0 = ((int)tile * STATS_WAVES + wave) * g.rows_per_wave;  // <= nj + 4 RW: no overflow
    const int rest = g.nj - j0;
    const int nrows = rest <= 0 ? 0 : (rest < g.rows_per_wave ? rest : g.rows_per_wave);
    StatsAcc s;
    stats_init(s);
    // the rows [j0, j0 + nrows) of level k: rows k nj + j0 ... of the field, none of them in another level
    const int64_t row0 = (int64_t)k * g.nj + (nrows > 0 ? j0 : 0);
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
        g.partials[(((size_t)blockIdx.y * g.nk + k) * g.tiles + tile) * STATS_SLOTS + slot] = v;
    }
}

// one thread per (entry, level, slot), slot fastest: the 8 threads of a level read 64 consecutive bytes per tile
__global__ void __launch_bounds__(LEVEL_STATS_FINISH_THREADS)
level_stats_finish_kernel(const double* __restrict__ partials, double* __restrict__ result, unsigned tiles, int nk, int64_t total) {
    const int64_t id = (int64_t)blockIdx.x * LEVEL_STATS_FINISH_THREADS + threadIdx.x;  // (entry * nk + k) * 8 + slot
    const bool live = id < total;
    const int slot = (int)(threadIdx.x % STATS_SLOTS);
    const int64_t level = id / STATS_SLOTS;  // entry * nk + k
    double v[LEVEL_STATS_MAX_TILES];
    const double* const p = partials + (size_t)(live ? level : 0) * tiles * STATS_SLOTS + slot;
#pragma unroll
    for (int t = 0; t < LEVEL_STATS_MAX_TILES; ++t) v[t] = (unsigned)t < tiles ? p[(size_t)t * STATS_SLOTS] : 0.0;
    unsigned n = tiles;
#pragma unroll
    for (int width = LEVEL_STATS_MAX_TILES; width > 1; width >>= 1) {  // n <= width
#pragma unroll
        for (int i = 0; i < width / 2; ++i) v[i] = (unsigned)(2 * i + 1) < n ? stats_combine(slot, v[2 * i], v[2 * i + 1]) : v[2 * i];
        n = (n + 1) >> 1;
    }
    // COUNT of this level is with the first of its 8 threads, in the same wave
    const double count = __shfl(v[0], (int)(threadIdx.x & ~7u) + STATS_COUNT, 64);
    if (!live) return;
    const int64_t entry = level / nk, k = level - entry * nk;
    double* const r = result + (size_t)entry * LEVEL_STATS_ROWS * nk + k;
    r[(size_t)slot * nk] = v[0];
    if (slot == STATS_SUM) r[(size_t)GT4MI_LEVEL_STATS_MEAN * nk] = v[0] / count;
}

// every check, then (unless `flags` carries GT4MI_STATS_DRY_RUN) the launches; *launches = kernels the call enqueues
inline int level_stats(const gt4mi_field* fields, const gt4mi_field* others, int nfields, const int64_t domain[3], int elem_size,
                       void* workspace, int64_t workspace_bytes, double* result, int flags, hipStream_t stream,
                       int64_t* workspace_needed, int* launches) {
    if (launches) *launches = 0;
    if (workspace_needed) *workspace_needed = 0;
    if (fields == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "level_stats: fields is null");
    if (nfields < 1) return fail(GT4MI_ERR_INVALID_ARGUMENT, "level_stats: nfields = %d, at least one field is needed", nfields);
    if (int rc = check_domain(domain)) return rc;
    for (int ax = 0; ax < 3; ++ax)
        if (domain[ax] < 1) return fail(GT4MI_ERR_INVALID_ARGUMENT, "level_stats: empty domain (%lld along axis %d)", (long long)domain[ax], ax);
    if (elem_size != 4 && elem_size != 8)
        return fail(GT4MI_ERR_UNSUPPORTED, "level_stats: item size %d is not supported (float32 or float64 fields)", elem_size);
    if (flags & ~GT4MI_STATS_DRY_RUN) return fail(GT4MI_ERR_INVALID_ARGUMENT, "level_stats: unknown bits in flags 0x%x", (unsigned)flags);
    const bool dry = (flags & GT4MI_STATS_DRY_RUN) != 0;
    if ((double)domain[0] * (double)domain[1] > 1099511627776.0)  // 2^40: the lanes count in 32 bits
        return fail(GT4MI_ERR_UNSUPPORTED, "level_stats: more than 2^40 points in a level");
    const LevelStatsGeometry geo = level_stats_geometry(domain);
    if (domain[2] * (int64_t)geo.tiles > LEVEL_STATS_MAX_WORKGROUPS)
        return fail(GT4MI_ERR_UNSUPPORTED, "level_stats: %lld levels of %u tiles are more than 2^24 workgroups", (long long)domain[2], geo.tiles);
    if (int rc = stats_check_fields("level_stats", fields, others, nfields, domain, elem_size)) return rc;
    const int64_t levels = (int64_t)nfields * domain[2];
    if (levels > ((int64_t)1 << 28))  // the finish kernel's grid: 8 threads per level, below 2^32
        return fail(GT4MI_ERR_UNSUPPORTED, "level_stats: %d fields of %lld levels are more than 2^28 profiles", nfields, (long long)domain[2]);
    const int64_t needed = levels * geo.tiles * STATS_SLOTS * (int64_t)sizeof(double);
    const int64_t result_bytes = levels * LEVEL_STATS_ROWS * (int64_t)sizeof(double);
    if (workspace_needed) *workspace_needed = needed;
    if (int rc = stats_check_buffers("level_stats", fields, others, nfields, domain, elem_size, workspace, workspace_bytes, needed, result,
                                     result_bytes, dry))
        return rc;
    const int count = (int)cdiv(nfields, STATS_MAX_ENTRIES) + 1;
    if (launches) *launches = count;
    if (dry) return GT4MI_OK;
    LevelStatsArgs a{};
    a.ni = (int)domain[0], a.nj = (int)domain[1], a.nk = (int)domain[2];
    a.rows_per_wave = geo.rows_per_wave, a.tiles = geo.tiles;
    for (int first = 0; first < nfields; first += STATS_MAX_ENTRIES) {
        const int nf = nfields - first < STATS_MAX_ENTRIES ? nfields - first : STATS_MAX_ENTRIES;
        for (int n = 0; n < nf; ++n) stats_fill_entry(a.e[n], fields[first + n], stats_other(others, first + n), elem_size);
        a.partials = static_cast<double*>(workspace) + (size_t)first * a.nk * geo.tiles * STATS_SLOTS;
        const dim3 grid((unsigned)(domain[2] * geo.tiles), (unsigned)nf);
        if (elem_size == 8) hipLaunchKernelGGL((level_stats_kernel<double>), grid, dim3(64 * STATS_WAVES), 0, stream, a);
        else hipLaunchKernelGGL((level_stats_kernel<float>), grid, dim3(64 * STATS_WAVES), 0, stream, a);
        GT4MI_HIP_CHECK(hipGetLastError());
    }
    const int64_t total = levels * STATS_SLOTS;
    hipLaunchKernelGGL(level_stats_finish_kernel, dim3((unsigned)cdiv(total, LEVEL_STATS_FINISH_THREADS)), dim3(LEVEL_STATS_FINISH_THREADS),
                       0, stream, static_cast<const double*>(workspace), result, geo.tiles, a.nk, total);
    GT4MI_HIP_CHECK(hipGetLastError());
    return GT4MI_OK;
}

}  // namespace gt4mi
