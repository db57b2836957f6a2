// Histograms: how the values of up to 8 fields are distributed over caller-given bins, over the whole box or per level k, ONE
// pass and ONE kernel launch, the counts left on the device as int64.
//
// NEW component, no reference counterpart: GTScript has no reduction and no result of another shape than its fields;
// gt4py.cartesian leaves a PDF, a median, a "fraction above" or a contoured-frequency-by-altitude diagram to numpy / cupy
// (`histogram`, `searchsorted` + `bincount`) on storages that ARE numpy / cupy arrays.
//
// THE CONTRACT (include/gt4py_amd.h states it, tests/histogram_ref.py restates it in plain Python and in numpy).  For one field,
// one row (the whole box, or one level of it) and nb bins the caller gives nb + 1 float64 edges e[0] < e[1] < ... < e[nb], all
// finite.  Every item x of the row's box is converted exactly to float64 and lands in exactly ONE of nb + 3 int64 counters:
//   nan     if x != x;
//   below   if x < e[0]  (-inf included);
//   above   if x > e[nb] (+inf included);
//   bin nb - 1 if x == e[nb]: the last bin is closed, as in numpy.histogram;
//   else the bin b with e[b] <= x < e[b+1]; -0.0 == 0.0 as IEEE compares them.
// The counters of a row sum to the items of its box.  They are integers: additions commute, so the result is exact and the same
// bits for any layout, path, grid, device or decomposition, without a fixed order.  Pads, ghost cells outside the box and
// anything else outside it are never read.
//
// THE COUNT DEPENDS ON THE EDGES ALONE (histogram_slot).  The bin is GUESSED as (x - e[0]) * nb / (e[nb] - e[0]), cut to
// [0, nb - 1]; the guess is moved by at most HIST_NUDGE bins towards x and ACCEPTED only if e[g] <= x && (x < e[g+1] || g == nb-1)
// holds on the edges themselves; otherwise a bisection of e[] decides.  Whatever rounding does to the guess, the answer is the
// bin the comparisons name.  EVERY LOOP IS BOUNDED BY A CONSTANT (HIST_NUDGE, HIST_BISECT = 13 > log2(4096)): any content of the
// edges buffer terminates and gives a slot in [0, nb + 3).  (The host checks the edges in the dry run only; a buffer overwritten
// later miscounts but neither hangs nor leaves the counters.)
//
// TWO PATHS, chosen per field from its strides as field_copy chooses (reported: GT4MI_HISTOGRAM_PATH_*):
//   ROWS   the field has unit item stride along an axis of the row's box that is longer than 1, whichever of I, J or K: that axis
//          is walked first.  Unit = one 16-byte lane of a line where the other strides (and the level stride) are multiples of 16
//          bytes and a line holds two lanes (the `lead` idea of field_copy.hip.h: partial lanes at both ends go item by item);
//          else one item.  The order of items is irrelevant to a count.
//   ITEMS  everything else, item by item in the order of the strides.  PER LEVEL the row's box is (ni, nj, 1): a K-contiguous
//          field has no line inside a level and goes this way (correct, and as slow as a strided read is).
// A thread takes HIST_UNROLL units 256 apart; their loads (nontemporal: the field is read once) are issued before the first count.
//
// ONE ROW PER WORKGROUP: blockIdx.x = row * chunks + chunk, blockIdx.y = field.  A workgroup counts `chunk` consecutive units of ONE
// row (one level, or the whole box), so everything it holds belongs to the row it flushes to.
//
// LDS PLAN (160 KiB per CU).  The edges are staged once per workgroup as float64, the counters are uint32:
//   nb <= 1024   one counter copy PER WAVE: 1025 * 8 + 4 * 1027 * 4 + 8 of padding = 24 640 bytes: 6 workgroups (24 waves) per CU;
//   nb <= 4096   one copy per workgroup: 4097 * 8 + 4099 * 4 + 12 of padding = 49 184 bytes: 3 workgroups (12 waves) per CU.
// Both live in ONE object (HistShared, aligned and so padded to 16 bytes): its sizeof IS the kernel's LDS size, asserted below.
// GT4MI_HISTOGRAM_MAX_BINS = 4096 is what leaves more than two workgroups per CU with the edges on chip; 8192 bins would leave one.
// Counting is `atomicAdd` on LDS words in plain HIP C++ (an LDS integer add, no return value used).
//
// THE HOT BIN (histogram_count).  Precipitation is zero at most points: most lanes of a wave hit ONE counter and the LDS adds of
// a wave serialise there.  Before the adds a wave peels, HIST_PEEL times, the bin of its first lane still to be counted: one
// ballot finds the lanes with the same bin, ONE lane adds their number, they are done.  All lanes equal = one add of the lane
// count.  What is left after the peels adds 1 per lane.  Every live lane is counted exactly once either way.
//
// NO COUNTER WRAPS: the host refuses a box of more than 2^31 - 1 items, a workgroup counts part of ONE row ONCE and flushes at its
// end, so a uint32 counter (and the sum of the four copies) stays below 2^31.  The flush adds the non-zero counters to the int64
// result with 64-bit integer atomics, relaxed, at agent scope; the result is complete when the kernel is (stream order).
// Without GT4MI_HISTOGRAM_ACCUMULATE the result is zeroed first by histogram_zero_kernel on the same stream (*launches counts
// the counting kernels and is 1).  It is a kernel and not a hipMemsetAsync because the call may be captured in a hipGraph.
// OBSERVED, not explained: with the memset, a captured call gave the right counts in the first replay of its graph and other
// words than zero plus the counts from the second replay on (tests/test_gpu_graph_replay.py; eager calls were never affected).
// Whether the runtime's memset node or the way this call made it is at fault was not found out and nothing was measured; the
// kernel is a workaround that takes the question away.  No float atomics, no inline assembly, no scratch, no workspace, no
// allocation, no synchronisation.
//
// OUT OF SCOPE: weighted histograms (float sums would need a fixed order), rows along I or J, two-dimensional (joint)
// histograms, edges changed after the checks (build a new call).
#pragma once

#include "common.hip.h"
#include "field_args.hip.h"

namespace gt4mi {

constexpr int HIST_MAX_FIELDS = GT4MI_HISTOGRAM_MAX_FIELDS;
constexpr int HIST_MAX_BINS = GT4MI_HISTOGRAM_MAX_BINS;
constexpr int HIST_EXTRA = GT4MI_HISTOGRAM_EXTRA;  // below, above, nan: behind the bins
constexpr int HIST_SMALL_BINS = 1024;              // up to here a counter copy per wave
constexpr int HIST_BLOCK = 256, HIST_WAVES = HIST_BLOCK / 64;
constexpr int HIST_UNROLL = 4;   // units per thread in flight
constexpr int HIST_PEEL = 2;     // hot bins a wave folds before the per-lane adds
constexpr int HIST_NUDGE = 2;    // bins the guess may be moved before the bisection takes over
constexpr int HIST_BISECT = 13;  // halvings of [0, nb]: more than log2(HIST_MAX_BINS)
constexpr int64_t HIST_MAX_WORKGROUPS = (int64_t)1 << 24;  // grid.x * 256 threads stays below 2^32
// everything a workgroup keeps in LDS
template <int CAP, int COPIES>
struct alignas(16) HistShared {
    double edge[CAP + 1];
    unsigned count[COPIES][CAP + HIST_EXTRA];
};
constexpr unsigned HIST_SMALL_LDS = sizeof(HistShared<HIST_SMALL_BINS, HIST_WAVES>);
constexpr unsigned HIST_LARGE_LDS = sizeof(HistShared<HIST_MAX_BINS, 1>);
static_assert(HIST_SMALL_LDS == 24640 && HIST_LARGE_LDS == 49184, "the LDS plan above");
static_assert(2 * HIST_LARGE_LDS <= 160 * 1024, "two workgroups per CU at the most bins");
static_assert((1 << (HIST_BISECT - 1)) >= HIST_MAX_BINS, "the bisection reaches one bin");
enum { HIST_LANES = 0, HIST_ITEMS = 1 };  // what a unit of a field is

// Zeroes `words` 64-bit words: a grid-stride loop, so that the grid stays small whatever the result's size.
__global__ void histogram_zero_kernel(unsigned long long* __restrict__ result, size_t words) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) result[i] = 0ull;
}

// The axes of a ROW's box are permuted per field by the host: [0] the unit-stride axis (ROWS) or the smallest stride (ITEMS).
struct HistField {
    const char* p;   // first item of the box
    int64_t s[3];    // strides in ITEMS
    int64_t srow;    // from one row (level) to the next, in ITEMS
    int n[3];
    int mode;        // HIST_LANES or HIST_ITEMS
    int lead;        // LANES: items from a line's first item to the first 16-byte boundary
    unsigned lanes;  // LANES: 16-byte lanes of a line (partial ones included)
    unsigned units;  // of a row
    unsigned chunk;  // units of a workgroup, a multiple of HIST_BLOCK * HIST_UNROLL
};

struct HistArgs {
    HistField f[HIST_MAX_FIELDS];
    const double* edges;
    unsigned long long* result;  // (int64 counters; the adds are the same bits)
    int nb, nrows, per_field;
    unsigned chunks;  // workgroups per row
};

// The slot of one item in [0, nb + HIST_EXTRA): the contract, decided by comparisons against edge[] alone.
__device__ __forceinline__ int histogram_slot(double x, const double* edge, int nb, double e0, double top, double scale) {
    if (x != x) return nb + GT4MI_HISTOGRAM_NAN;
    if (x < e0) return nb + GT4MI_HISTOGRAM_BELOW;
    if (x > top) return nb + GT4MI_HISTOGRAM_ABOVE;
    double t = (x - e0) * scale;  // (may be anything, a NaN included, if the edges are extreme: the comparisons below decide)
    t = t >= 0.0 ? t : 0.0;
    t = t <= (double)(nb - 1) ? t : (double)(nb - 1);
    int g = (int)t;
#pragma unroll
    for (int step = 0; step < HIST_NUDGE; ++step) {
        if (g > 0 && x < edge[g]) --g;
        else if (g < nb - 1 && x >= edge[g + 1]) ++g;
    }
    if (edge[g] <= x && (x < edge[g + 1] || g == nb - 1)) return g;
    int lo = 0, hi = nb;  // e[lo] <= x, and x < e[hi] or hi == nb
    for (int it = 0; it < HIST_BISECT && hi - lo > 1; ++it) {
        const int mid = (lo + hi) >> 1;
        if (x >= edge[mid]) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Count one item per live lane of a wave (every lane of the wave calls this together): equal slots are folded first.
__device__ __forceinline__ void histogram_count(unsigned* count, int slot, bool live, int lane) {
    unsigned long long todo = __ballot(live);
#pragma unroll
    for (int round = 0; round < HIST_PEEL; ++round) {
        if (todo == 0) break;  // (uniform)
        const int leader = __ffsll((long long)todo) - 1;
        const int hot = __shfl(slot, leader);
        const unsigned long long same = __ballot(slot == hot) & todo;  // the leader is one of them
        if (lane == leader) atomicAdd(&count[hot], (unsigned)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1) atomicAdd(&count[slot], 1u);
}

template <typename T, int CAP, int COPIES>
__global__ void __launch_bounds__(HIST_BLOCK)
field_histogram_kernel(const HistArgs a) {
    constexpr int V = 16 / (int)sizeof(T);
    using Vec = typename VecT<T, V>::type;
    __shared__ HistShared<CAP, COPIES> lds;
    double* const edge = lds.edge;
    auto& count = lds.count;
    // (selected with scalar moves: indexing the by-value argument block with blockIdx.y makes the compiler copy it to scratch)
    HistField f = a.f[0];
#pragma unroll
    for (int n = 1; n < HIST_MAX_FIELDS; ++n)
        if (blockIdx.y == (unsigned)n) f = a.f[n];
    const unsigned row = blockIdx.x / a.chunks, chunk = blockIdx.x - row * a.chunks;
    const unsigned begin = chunk * f.chunk;  // (below units + 1024 * chunks <= 2 * 2^31: the host sizes chunks by the field with the most units)
    if (begin >= f.units) return;  // a field with fewer units than the grid was sized for: whole workgroups leave, before any barrier
    const unsigned end = f.units - begin < f.chunk ? f.units : begin + f.chunk;
    const int nb = a.nb, slots = nb + HIST_EXTRA;
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    const double* const from = a.edges + (a.per_field ? (size_t)blockIdx.y * (size_t)(nb + 1) : 0);
    for (int i = (int)threadIdx.x; i <= nb; i += HIST_BLOCK) edge[i] = from[i];
    for (int i = (int)threadIdx.x; i < slots; i += HIST_BLOCK) {
#pragma unroll
        for (int c = 0; c < COPIES; ++c) count[c][i] = 0u;
    }
    __syncthreads();
    const double e0 = edge[0], top = edge[nb];
    const double scale = (double)nb / (top - e0);
    unsigned* const mine = count[COPIES > 1 ? wave : 0];
    const T* const base = reinterpret_cast<const T*>(f.p) + (int64_t)row * f.srow;
    const bool lanes = f.mode == HIST_LANES;

    for (unsigned first = begin; first < end; first += (unsigned)(HIST_BLOCK * HIST_UNROLL)) {  // (uniform over the workgroup)
        T v[HIST_UNROLL][V];
        unsigned ok[HIST_UNROLL];  // bit e: item e of the unit is inside the box
#pragma unroll
        for (int u = 0; u < HIST_UNROLL; ++u) {
            const unsigned unit = first + (unsigned)u * HIST_BLOCK + threadIdx.x;
            ok[u] = 0u;
#pragma unroll
            for (int e = 0; e < V; ++e) v[u][e] = T(0);
            if (unit >= end) continue;
            if (lanes) {
                const unsigned line = unit / f.lanes, x = unit - line * f.lanes;
                const unsigned r2 = line / (unsigned)f.n[1], r1 = line - r2 * (unsigned)f.n[1];
                const T* const p = base + (int64_t)r1 * f.s[1] + (int64_t)r2 * f.s[2];
                // lane x covers the items [i0, i0 + V) cut to [0, n); with lead > 0 lane 0 is the partial one in front
                const int i0 = f.lead > 0 ? f.lead + ((int)x - 1) * V : (int)x * V;
                if (i0 >= 0 && i0 + V <= f.n[0]) {
                    const Vec w = __builtin_nontemporal_load(reinterpret_cast<const Vec*>(p + i0));
#pragma unroll
                    for (int e = 0; e < V; ++e) v[u][e] = w[e];
                    ok[u] = (1u << V) - 1u;
                } else {
#pragma unroll
                    for (int e = 0; e < V; ++e)
                        if (i0 + e >= 0 && i0 + e < f.n[0]) v[u][e] = __builtin_nontemporal_load(p + (i0 + e)), ok[u] |= 1u << e;
                }
            } else {
                const unsigned q = unit / (unsigned)f.n[0], i0 = unit - q * (unsigned)f.n[0];
                const unsigned i2 = q / (unsigned)f.n[1], i1 = q - i2 * (unsigned)f.n[1];
                v[u][0] = __builtin_nontemporal_load(base + (int64_t)i0 * f.s[0] + (int64_t)i1 * f.s[1] + (int64_t)i2 * f.s[2]);
                ok[u] = 1u;
            }
        }
#pragma unroll
        for (int u = 0; u < HIST_UNROLL; ++u) {
#pragma unroll
            for (int e = 0; e < V; ++e) {
                if (e > 0 && !lanes) break;  // (uniform: an ITEMS unit is one item)
                const int slot = histogram_slot((double)v[u][e], edge, nb, e0, top, scale);
                histogram_count(mine, slot, (ok[u] >> e) & 1u, lane);
            }
        }
    }

    __syncthreads();
    unsigned long long* const out = a.result + ((size_t)blockIdx.y * (size_t)a.nrows + row) * (size_t)slots;
    for (int i = (int)threadIdx.x; i < slots; i += HIST_BLOCK) {
        unsigned total = 0u;
#pragma unroll
        for (int c = 0; c < COPIES; ++c) total += count[c][i];
        if (total != 0u) __hip_atomic_fetch_add(out + i, (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
const BoxChecks HIST_CHECKS = {"field_histogram", "extent", "a histogram counts items, no field may be broadcast", false, false};

// path of a field and its descriptor (units and chunk are set by the caller's second pass: they need every field's units)
inline int histogram_plan(const gt4mi_field& fld, const int64_t extent[3], int elem_size, int by, HistField* out) {
    HistField h{};
    h.p = origin_ptr(fld);
    const int64_t ext[3] = {extent[0], extent[1], by ? 1 : extent[2]};  // the box of one row
    int64_t s[3];
    item_strides(fld, elem_size, s);
    int ua = -1;
    for (int ax = 2; ax >= 0; --ax)
        if (ext[ax] > 1 && fld.stride[ax] == elem_size) ua = ax;
    int order[3] = {0, 1, 2};
    auto by_stride = [&](int first) {  // order[first..2] ascending in |stride|, axes of extent 1 last
        auto key = [&](int ax) { return ext[ax] > 1 ? (s[ax] < 0 ? -s[ax] : s[ax]) : INT64_MAX; };
        for (int x = first; x < 3; ++x)
            for (int y = x + 1; y < 3; ++y)
                if (key(order[y]) < key(order[x])) { const int t = order[x]; order[x] = order[y]; order[y] = t; }
    };
    h.mode = HIST_ITEMS;
    if (ua < 0) {
        by_stride(0);
    } else {
        order[0] = ua, order[1] = (ua + 1) % 3, order[2] = (ua + 2) % 3;
        by_stride(1);
        const int V = 16 / elem_size;
        const bool pitches = (ext[order[1]] == 1 || fld.stride[order[1]] % 16 == 0) && (ext[order[2]] == 1 || fld.stride[order[2]] % 16 == 0) &&
                             (!by || extent[2] == 1 || fld.stride[2] % 16 == 0);
        if (pitches && ext[ua] >= 2 * V) {
            h.mode = HIST_LANES;
            h.lead = (int)(((16 - reinterpret_cast<uintptr_t>(h.p) % 16) % 16) / (uintptr_t)elem_size);
            h.lanes = (unsigned)((h.lead > 0) + cdiv(ext[ua] - h.lead, V));
        }
    }
    for (int x = 0; x < 3; ++x) h.n[x] = (int)ext[order[x]], h.s[x] = s[order[x]];
    h.srow = by ? s[2] : 0;
    h.units = (unsigned)((h.mode == HIST_LANES ? (int64_t)h.lanes : (int64_t)h.n[0]) * h.n[1] * h.n[2]);
    *out = h;
    return ua >= 0 ? GT4MI_HISTOGRAM_PATH_ROWS : GT4MI_HISTOGRAM_PATH_ITEMS;
}

// every check, then (unless `flags` carries GT4MI_HISTOGRAM_DRY_RUN) the zeroing and the launch
inline int field_histogram(const gt4mi_field* fields, int nfields, const int64_t extent[3], int elem_size, int nbins, const double* edges,
                           const double* edges_host, int by, int64_t* result, int flags, hipStream_t stream, int* path, int* launches) {
    if (launches) *launches = 0;
    if (path) *path = -1;
    const char* const entry = HIST_CHECKS.entry;
    if (fields == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: fields is null", entry);
    if (extent == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: extent is null", entry);
    if (nfields < 1 || nfields > HIST_MAX_FIELDS)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: nfields = %d is outside 1 .. %d", entry, nfields, HIST_MAX_FIELDS);
    if (nbins < 1 || nbins > HIST_MAX_BINS) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: nbins = %d is outside 1 .. %d", entry, nbins, HIST_MAX_BINS);
    for (int ax = 0; ax < 3; ++ax) {
        if (extent[ax] < 0 || extent[ax] > INT32_MAX)
            return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: invalid extent %lld along axis %d", entry, (long long)extent[ax], ax);
        if (extent[ax] == 0) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: empty box (0 along axis %d)", entry, ax);
    }
    if (elem_size != 4 && elem_size != 8)
        return fail(GT4MI_ERR_UNSUPPORTED, "%s: item size %d is not supported (float32 or float64)", entry, elem_size);
    if (by != GT4MI_HISTOGRAM_WHOLE && by != GT4MI_HISTOGRAM_BY_K)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: by %d is not GT4MI_HISTOGRAM_WHOLE or GT4MI_HISTOGRAM_BY_K", entry, by);
    if (flags & ~(GT4MI_HISTOGRAM_ACCUMULATE | GT4MI_HISTOGRAM_EDGES_PER_FIELD | GT4MI_HISTOGRAM_DRY_RUN))
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: unknown bits in flags 0x%x", entry, (unsigned)flags);
    const bool dry = (flags & GT4MI_HISTOGRAM_DRY_RUN) != 0, per_field = (flags & GT4MI_HISTOGRAM_EDGES_PER_FIELD) != 0;
    const int sets = per_field ? nfields : 1;
    if (dry) {  // the edges themselves: the dry run, and only the dry run, reads them (from the host copy)
        if (edges_host == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: edges_host is null (the dry run checks the edges)", entry);
        for (int k = 0; k < sets; ++k) {
            const double* const e = edges_host + (size_t)k * (size_t)(nbins + 1);
            for (int i = 0; i <= nbins; ++i) {
                if (!(e[i] - e[i] == 0.0)) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: edge %d of set %d is not finite", entry, i, k);
                if (i > 0 && !(e[i - 1] < e[i]))
                    return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: the edges of set %d are not strictly increasing at index %d", entry, k, i);
            }
        }
    }
    for (int k = 0; k < nfields; ++k)
        if (int rc = check_box_field(HIST_CHECKS, "field", k, fields[k], extent, elem_size, true)) return rc;
    if ((double)extent[0] * (double)extent[1] * (double)extent[2] > (double)INT32_MAX)
        return fail(GT4MI_ERR_UNSUPPORTED, "%s: more than 2^31 - 1 items in the box", entry);
    const int64_t nrows = by ? extent[2] : 1;
    if (nrows > HIST_MAX_WORKGROUPS) return fail(GT4MI_ERR_UNSUPPORTED, "%s: %lld levels are more than 2^24 workgroups", entry, (long long)nrows);
    // edges and result: there unless the call is a dry run, aligned to 8 bytes, the result clear of everything that is read
    if (!dry && edges == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: edges is null", entry);
    if (!dry && result == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: result is null", entry);
    if (edges != nullptr && reinterpret_cast<uintptr_t>(edges) % 8 != 0)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: edges is not aligned to 8 bytes", entry);
    const size_t result_bytes = (size_t)nfields * (size_t)nrows * (size_t)(nbins + HIST_EXTRA) * sizeof(int64_t);
    if (result != nullptr) {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(result);
        const ByteSpan span{lo, lo + (uintptr_t)result_bytes};
        if (lo % 8 != 0) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: result is not aligned to 8 bytes", entry);
        for (int k = 0; k < nfields; ++k)
            if (spans_overlap(span, box_span(fields[k], extent, elem_size)))
                return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: result overlaps field %d", entry, k);
        if (edges != nullptr) {
            const uintptr_t elo = reinterpret_cast<uintptr_t>(edges);
            if (spans_overlap(span, ByteSpan{elo, elo + (uintptr_t)sets * (uintptr_t)(nbins + 1) * sizeof(double)}))
                return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: result overlaps edges", entry);
        }
    }
    HistArgs a{};
    int common = GT4MI_HISTOGRAM_PATH_ROWS;  // ROWS if every field goes that way
    unsigned most = 0;
    for (int k = 0; k < nfields; ++k) {
        if (histogram_plan(fields[k], extent, elem_size, by, &a.f[k]) != GT4MI_HISTOGRAM_PATH_ROWS) common = GT4MI_HISTOGRAM_PATH_ITEMS;
        if (a.f[k].units > most) most = a.f[k].units;
    }
    if (path) *path = common;
    if (launches) *launches = 1;
    if (dry) return GT4MI_OK;
    // one wave of resident workgroups over all rows and fields, never less than one pass of HIST_UNROLL units per thread each
    const bool small = nbins <= HIST_SMALL_BINS;
    const int64_t pass = HIST_BLOCK * HIST_UNROLL;
    int64_t chunks = (int64_t)256 * (small ? 160 * 1024 / HIST_SMALL_LDS : 160 * 1024 / HIST_LARGE_LDS) / (nrows * nfields);
    if (chunks > cdiv(most, pass)) chunks = cdiv(most, pass);
    if (chunks < 1) chunks = 1;
    if (nrows * chunks > HIST_MAX_WORKGROUPS) chunks = HIST_MAX_WORKGROUPS / nrows;
    for (int k = 0; k < nfields; ++k) a.f[k].chunk = (unsigned)(cdiv(cdiv(a.f[k].units, chunks), pass) * pass);
    a.edges = edges, a.result = reinterpret_cast<unsigned long long*>(result);
    a.nb = nbins, a.nrows = (int)nrows, a.per_field = per_field ? 1 : 0, a.chunks = (unsigned)chunks;
    if (!(flags & GT4MI_HISTOGRAM_ACCUMULATE)) {
        const size_t words = result_bytes / sizeof(int64_t);
        const unsigned blocks = (unsigned)(cdiv((int64_t)words, (int64_t)HIST_BLOCK) < 1024 ? cdiv((int64_t)words, (int64_t)HIST_BLOCK) : 1024);
        hipLaunchKernelGGL(histogram_zero_kernel, dim3(blocks), dim3(HIST_BLOCK), 0, stream, a.result, words);
    }
    const dim3 grid((unsigned)(nrows * chunks), (unsigned)nfields);
    with_item_type(elem_size, [&](auto t) {
        using T = decltype(t);
        if (small) hipLaunchKernelGGL((field_histogram_kernel<T, HIST_SMALL_BINS, HIST_WAVES>), grid, dim3(HIST_BLOCK), 0, stream, a);
        else hipLaunchKernelGGL((field_histogram_kernel<T, HIST_MAX_BINS, 1>), grid, dim3(HIST_BLOCK), 0, stream, a);
    });
    GT4MI_HIP_CHECK(hipGetLastError());
    return GT4MI_OK;
}

}  // namespace gt4mi
