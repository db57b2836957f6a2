// Fourier filtering along periodic lines of I, J or K: every line of the box along `axis` is transformed, each wavenumber m is multiplied
// by a real response[m] and the line is transformed back (FILTER), or the forward transform alone is stored (SPECTRUM), for up to 8
// fields per launch.
//
// NEW component.  The reference has nothing in wavenumber space: a stencil reads its neighbours at compile-time offsets, a Fourier
// coefficient reads the whole line.  Its users leave for an FFT library: rfft, a multiply and irfft per field, three launches and more,
// complex intermediates of the field's size, the order of the arithmetic the library's.
//
// THE ARITHMETIC CONTRACT (include/gt4py_amd.h states it, tests/line_filter_ref.py restates it in plain Python and in numpy).  n =
// extent[axis] is a power of two, 2 <= n <= 4096; L = log2 n; nh = n / 2 + 1.  All arithmetic is IEEE float64 on the items converted
// exactly, one rounding per operation, no FMA; one rounding to the fields' type on the store.
//   TWIDDLES  an INPUT, computed on the host: wr[j] = cos(2 pi j / n), wi[j] = -sin(2 pi j / n) for j < n/2, with w[0] = (1, 0) and
//             w[n/4] = (0, -1) set exactly.  The device never evaluates a sine or a cosine.
//   FORWARD   radix-2 decimation in frequency, natural order in, bit-reversed order out; x[p] = (item p, +0.0).  For h = n/2, n/4, .. 1,
//             for every block start (a multiple of 2h) and j < h:  p = start + j, q = p + h, w = w[j * n / (2h)]:
//               u = a - b ;  a' = a + b ;  b'.re = wr * u.re - wi * u.im ;  b'.im = wr * u.im + wi * u.re        (a = x[p], b = x[q])
//   MULTIPLY  slot p holds wavenumber m = bitrev_L(p): both parts are multiplied by response[min(m, n - m)].
//   INVERSE   radix-2 decimation in time, bit-reversed order in, natural order out, with conj(w).  For h = 1, 2, .. n/2, p, q, w as above:
//               t.re = wr * b.re + wi * b.im ;  t.im = wr * b.im - wi * b.re ;  a' = a + t ;  b' = a - t
//             dst[p] = T(x[p].re * (1.0 / n)); the imaginary part is dropped.
//   SPECTRUM  the slot at p is stored at m = bitrev_L(p) where m <= n/2.
// No trivial twiddle is skipped and no zero imaginary part is left out of the arithmetic: 1 * x - 0 * y is not x where y is an inf or
// a NaN, or where x is -0.0 and y is negative.  A line's bits depend on the line, its response row and n alone.
//
// WHY IT ENDS AND STAYS IN ITS BOX WHATEVER THE DATA HOLDS: every loop bound and every address follows from n, the extents and the
// strides, which the host has checked against every field's shape; none depends on field data, the response or the twiddles.
//
// ONE KERNEL TEMPLATE.  Unlike the march kernels of the family, the parallelism is INSIDE the line: a workgroup of 256 lanes owns a TILE
// of whole lines in LDS, as float64 real and imaginary parts in two arrays -- 2048 points (32 KiB) where n <= 2048, beside the twiddles
// (16 KiB), so that three workgroups share a CU; 4096 points (all 64 KiB of the static limit) for n = 4096, one line, the twiddles read
// through the cache.  The tile is 2048 / n (4096 / n) consecutive lines; field `blockIdx.y` of the launch.
//   load      global -> re[], by the path (below); the imaginary part is never stored: the first pass takes +0.0.
//   passes    up to three radix-2 stages are fused in registers: a lane takes the 2, 4 or 8 points that these stages connect, does every
//             butterfly of the contract on them in the contract's order, and puts them back.  The stages above the last three go first
//             (the remainder of L / 3, then threes); the last three forward stages, the multiply and the first three inverse stages
//             touch the same 8 slots and are ONE pass in registers.  One workgroup barrier per pass.  No permutation is executed: the
//             bit reversal exists only in the index of the response (and of the spectrum's store).
//   store     re[] -> global, by the path.
// LDS BANKS.  Point P of the tile lives at P ^ ((P >> 5) & 7) ^ (((P >> 6) & 3) << 3): a permutation inside every 32 points.  An 8-byte
// LDS read is served in two halves of 32 lanes over 32 banks of 8 bytes.  In a pass whose points are 2^lh apart (lh = 0, 3, 6, 9: the
// remainder goes first), 32 consecutive lanes read points that differ in bits 0 .. lh-1 and lh+3 .. 7 of P; the fold brings bits 5 .. 7
// back into the bank index, once beside bits 3, 4 (lh = 0) and once beside bits 0 .. 2 (lh = 3): every read of every pass is free of
// conflicts, every write but those of the lh = 0 pass (2-way, which an 8-byte LDS write hides behind its own issue cost).  Counted by
// enumeration of the addresses, not measured.  The loads of the LANES path and the spectrum's store (lanes along m, slots bit-reversed)
// do conflict; both touch every point once.
// THREE PATHS by the family's rule (line_geometry.hip.h: LinePlan; the response is fed as a loose field that is unit along the line):
//   TILES  the line axis has unit stride in every field: lanes along the line itself, 16 bytes per lane where every line of the call
//          starts on a 16-byte boundary (`wide`), else item by item, still coalesced.
//   LANES  another axis has unit stride: the tile's lines are neighbours along it, lanes run across them: a load covers runs of
//          2048 / n items along that axis.
//   ITEMS  anything else: lanes along the line, one strided item each.
// The path, filter or spectrum and `wide` are UNIFORM branches: 4 kernels (float, double) x (n <= 2048, n = 4096).  No scratch, no
// atomics, no ordering between workgroups, no host synchronisation, no workspace.  dst[k] may BE src[k]: a workgroup has read all of
// its lines before it stores the first item, and no other workgroup touches them.
#pragma once

#include <type_traits>

#include "line_geometry.hip.h"

#pragma clang fp contract(off)

namespace gt4mi {

constexpr int FILTER_BLOCK = 256;    // lanes of a workgroup
constexpr int FILTER_MAX_LOG = 12;   // n <= 4096
constexpr int FILTER_SMALL_LOG = 11; // the tile of the small kernel: 2048 points, and as many twiddle doubles

struct FilterArgs {
    PairEntry e[PAIR_MAX_FIELDS];  // strides permuted by the host: [0] the line axis, [1] the lane axis A, [2] the remaining axis B
    const double* response;        // FILTER: row (ia, ib) starts at response[ia * ra + ib * rb]; 0 broadcasts
    const double* twiddles;        // wr[0 .. n/2) then wi[0 .. n/2)
    double* result;                // SPECTRUM: result[(f * 2 + part) * qp + ia * qa + ib * qb + m]
    int64_t ra, rb, qa, qb, qp;
    double scale;                  // 1.0 / n
    int n, logn, na, nb, nf, spectrum, across, wide;  // across: LANES; wide: 16-byte lanes on TILES
};

// where point P of a tile lives (see LDS BANKS)
__device__ __forceinline__ int filter_slot(int p) { return p ^ ((p >> 5) & 7) ^ (((p >> 6) & 3) << 3); }

// The S radix-2 stages that connect the 2^S points base + k * 2^lh of a line (j = base mod 2^lh), in the contract's order: forward
// from the widest (k's top bit) down, inverse from the narrowest up.  The twiddle of a pair h apart at offset jj in its half block
// is w[jj * n / (2h)].
template <int S, bool FORWARD>
__device__ __forceinline__ void filter_stages(double (&xr)[1 << S], double (&xi)[1 << S], int j, int lh, int logn, const double* wr,
                                              const double* wi) {
    constexpr int R = 1 << S;
#pragma unroll
    for (int step = 0; step < S; ++step) {
        const int s = FORWARD ? S - 1 - step : step;  // the bit of k that tells a from b
        const int kd = 1 << s;
        const int shift = logn - 1 - (lh + s);
#pragma unroll
        for (int low = 0; low < kd; ++low) {
            const int at = (j + (low << lh)) << shift;
            const double cr = wr[at], ci = wi[at];
#pragma unroll
            for (int high = 0; high < R / (2 * kd); ++high) {
                const int ka = high * 2 * kd + low, kb = ka + kd;
                if constexpr (FORWARD) {
                    const double ur = xr[ka] - xr[kb], ui = xi[ka] - xi[kb];
                    xr[ka] = xr[ka] + xr[kb], xi[ka] = xi[ka] + xi[kb];
                    xr[kb] = cr * ur - ci * ui, xi[kb] = cr * ui + ci * ur;
                } else {
                    const double tr = cr * xr[kb] + ci * xi[kb], ti = cr * xi[kb] - ci * xr[kb];
                    const double ar = xr[ka], ai = xi[ka];
                    xr[ka] = ar + tr, xi[ka] = ai + ti;
                    xr[kb] = ar - tr, xi[kb] = ai - ti;
                }
            }
        }
    }
}

// One pass over the `work` live lane jobs of a tile (2^S points each): S stages whose narrowest pairs are 2^lh apart.  `first`: the
// imaginary parts are +0.0 and not in LDS yet; `last`: the real parts are scaled and the imaginary parts dropped.
template <int S, bool FORWARD>
__device__ __forceinline__ void filter_pass(double* re, double* im, int work, int lh, int logn, const double* wr, const double* wi, bool first,
                                            bool last, double scale) {
    constexpr int R = 1 << S;
    for (int w = (int)threadIdx.x; w < work; w += FILTER_BLOCK) {
        const int j = w & ((1 << lh) - 1);
        const int base = ((w >> lh) << (lh + S)) | j;
        double xr[R], xi[R];
        int at[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            at[k] = filter_slot(base | (k << lh));
            xr[k] = re[at[k]];
            xi[k] = first ? 0.0 : im[at[k]];
        }
        filter_stages<S, FORWARD>(xr, xi, j, lh, logn, wr, wi);
#pragma unroll
        for (int k = 0; k < R; ++k) {
            re[at[k]] = last ? xr[k] * scale : xr[k];
            if (!last) im[at[k]] = xi[k];
        }
    }
}

// The pass in the middle, on the 2^S neighbouring slots of a lane (lh = 0): the last S forward stages, then FILTER: the multiply and the
// first S inverse stages; SPECTRUM: nothing more.  S = min(L, 3); for L <= 3 it is the only pass, first and last at once.
template <int S>
__device__ __forceinline__ void filter_middle(const FilterArgs& a, double* re, double* im, int work, int64_t line0, const double* wr,
                                              const double* wi) {
    constexpr int R = 1 << S;
    const int logn = a.logn, n = a.n;
    const bool only = logn <= 3;
    for (int w = (int)threadIdx.x; w < work; w += FILTER_BLOCK) {
        const int base = w << S;
        double xr[R], xi[R];
        int at[R];
#pragma unroll
        for (int k = 0; k < R; ++k) {
            at[k] = filter_slot(base | k);
            xr[k] = re[at[k]];
            xi[k] = only ? 0.0 : im[at[k]];
        }
        filter_stages<S, true>(xr, xi, 0, 0, logn, wr, wi);
        if (!a.spectrum) {
            const uint32_t line = (uint32_t)(line0 + (base >> logn));
            const uint32_t ib = line / (uint32_t)a.na, ia = line - ib * (uint32_t)a.na;
            const double* const row = a.response + (int64_t)ia * a.ra + (int64_t)ib * a.rb;
            double r[R];
#pragma unroll
            for (int k = 0; k < R; ++k) {
                const int m = (int)(__brev((uint32_t)((base | k) & (n - 1))) >> (32 - logn));
                r[k] = row[m < n - m ? m : n - m];
            }
#pragma unroll
            for (int k = 0; k < R; ++k) xr[k] = xr[k] * r[k], xi[k] = xi[k] * r[k];
            filter_stages<S, false>(xr, xi, 0, 0, logn, wr, wi);
        }
        const bool last = only && !a.spectrum;
#pragma unroll
        for (int k = 0; k < R; ++k) {
            re[at[k]] = last ? xr[k] * a.scale : xr[k];
            if (!last) im[at[k]] = xi[k];
        }
    }
}

// Move the tile's live lines between a field and re[]: LOAD converts exactly to double, the store rounds once to T.  s[]: the field's
// strides in items ([0] line axis, [1] A, [2] B).  Lines are numbered ia + na * ib; the tile's are line0 .. line0 + live.
template <typename T, bool LOAD>
__device__ __forceinline__ void filter_move(const FilterArgs& a, double* re, std::conditional_t<LOAD, const T, T>* field, const int64_t (&s)[3],
                                            int64_t line0, int live, int tile_log) {
    const int logn = a.logn, n = a.n;
    const uint32_t na = (uint32_t)a.na;
    auto offset = [&](int l) {
        const uint32_t line = (uint32_t)(line0 + l);
        const uint32_t ib = line / na, ia = line - ib * na;
        return (int64_t)ia * s[1] + (int64_t)ib * s[2];
    };
    if (a.across) {  // LANES: consecutive lanes on consecutive lines
        const int lines_log = tile_log - logn, lines = 1 << lines_log;
        for (int e = (int)threadIdx.x; e < (1 << tile_log); e += FILTER_BLOCK) {
            const int l = e & (lines - 1), m = e >> lines_log;
            if (l >= live) continue;
            const int64_t o = offset(l) + (int64_t)m * s[0];
            const int at = filter_slot((l << logn) | m);
            if constexpr (LOAD) re[at] = (double)field[o];
            else field[o] = (T)re[at];
        }
    } else if (a.wide) {  // TILES, 16 bytes per lane (the host has checked the alignment of every line)
        constexpr int V = 16 / (int)sizeof(T);
        using Vec = T __attribute__((ext_vector_type(V)));
        for (int e = (int)threadIdx.x * V; e < (live << logn); e += FILTER_BLOCK * V) {
            const int64_t o = offset(e >> logn) + (e & (n - 1));
            if constexpr (LOAD) {
                const Vec v = *reinterpret_cast<const Vec*>(field + o);
#pragma unroll
                for (int u = 0; u < V; ++u) re[filter_slot(e + u)] = (double)v[u];
            } else {
                Vec v;
#pragma unroll
                for (int u = 0; u < V; ++u) v[u] = (T)re[filter_slot(e + u)];
                *reinterpret_cast<Vec*>(field + o) = v;
            }
        }
    } else {  // TILES item by item, ITEMS
        for (int e = (int)threadIdx.x; e < (live << logn); e += FILTER_BLOCK) {
            const int64_t o = offset(e >> logn) + (int64_t)(e & (n - 1)) * s[0];
            if constexpr (LOAD) re[filter_slot(e)] = (double)field[o];
            else field[o] = (T)re[filter_slot(e)];
        }
    }
}

template <typename T, bool BIG>
__global__ void __launch_bounds__(FILTER_BLOCK)
line_filter_kernel(const FilterArgs a) {
    constexpr int TILE_LOG = BIG ? FILTER_MAX_LOG : FILTER_SMALL_LOG, TILE = 1 << TILE_LOG;
    __shared__ double lds[BIG ? 2 * TILE : 3 * TILE];  // re, im and (small) the twiddles: 64 KiB / 48 KiB
    double* const re = lds;
    double* const im = lds + TILE;
    const int logn = a.logn, n = a.n;
    const int lines_log = TILE_LOG - logn;
    const int64_t lines = (int64_t)a.na * a.nb, line0 = (int64_t)blockIdx.x << lines_log;
    const int live = lines - line0 < (1 << lines_log) ? (int)(lines - line0) : 1 << lines_log;
    const PairEntry& e = a.e[blockIdx.y];
    const double *wr = a.twiddles, *wi = a.twiddles + n / 2;
    if constexpr (!BIG) {
        double* const tw = lds + 2 * TILE;
        for (int i = (int)threadIdx.x; i < n; i += FILTER_BLOCK) tw[i] = a.twiddles[i];
        wr = tw, wi = tw + n / 2;
    }
    filter_move<T, true>(a, re, reinterpret_cast<const T*>(e.src), e.s, line0, live, TILE_LOG);
    __syncthreads();
    // the stages above the last three: the remainder first, then threes; `lh`: how far apart the narrowest pairs of the pass are
    const int middle = logn < 3 ? logn : 3, rest = (logn - middle) % 3;
    int lh = logn;
    bool first = true;
    if (rest != 0) {
        lh -= rest;
        if (rest == 1) filter_pass<1, true>(re, im, live << (logn - 1), lh, logn, wr, wi, first, false, a.scale);
        else filter_pass<2, true>(re, im, live << (logn - 2), lh, logn, wr, wi, first, false, a.scale);
        first = false;
        __syncthreads();
    }
    while (lh > middle) {
        lh -= 3;
        filter_pass<3, true>(re, im, live << (logn - 3), lh, logn, wr, wi, first, false, a.scale);
        first = false;
        __syncthreads();
    }
    if (middle == 3) filter_middle<3>(a, re, im, live << (logn - 3), line0, wr, wi);
    else if (middle == 2) filter_middle<2>(a, re, im, live, line0, wr, wi);
    else filter_middle<1>(a, re, im, live, line0, wr, wi);
    __syncthreads();
    if (a.spectrum) {  // lanes along m: the stores are coalesced, the slots bit-reversed
        const uint32_t nh = (uint32_t)(n / 2 + 1), na = (uint32_t)a.na;
        double* const out = a.result + (int64_t)blockIdx.y * 2 * a.qp;
        for (uint32_t i = threadIdx.x; i < (uint32_t)live * nh; i += FILTER_BLOCK) {
            const uint32_t l = i / nh, m = i - l * nh;
            const uint32_t line = (uint32_t)(line0 + l);
            const uint32_t ib = line / na, ia = line - ib * na;
            const int at = filter_slot((int)((l << logn) | (__brev(m) >> (32 - logn))));
            double* const to = out + (int64_t)ia * a.qa + (int64_t)ib * a.qb + m;
            to[0] = re[at];
            to[a.qp] = im[at];
        }
        return;
    }
    // the inverse stages above the first three: threes, then the remainder; the last pass scales and drops the imaginary parts
    for (lh = middle; lh < logn - rest; lh += 3) {
        filter_pass<3, false>(re, im, live << (logn - 3), lh, logn, wr, wi, false, lh + 3 == logn, a.scale);
        __syncthreads();
    }
    if (rest != 0) {
        if (rest == 1) filter_pass<1, false>(re, im, live << (logn - 1), lh, logn, wr, wi, false, true, a.scale);
        else filter_pass<2, false>(re, im, live << (logn - 2), lh, logn, wr, wi, false, true, a.scale);
        __syncthreads();
    }
    filter_move<T, false>(a, re, reinterpret_cast<T*>(e.dst), e.d, line0, live, TILE_LOG);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
const BoxChecks FILTER_CHECKS = {"line_filter", "extent", "only a src may be broadcast", false, false};
const PairRoles FILTER_ROLES = {"dst", "src", true};      // a dst may BE its own src (the same box), and meet nothing else
const PairRoles SPECTRUM_ROLES = {"field", "field", true};

// every check, then (unless `flags` carries GT4MI_FILTER_DRY_RUN) the launches
inline int line_filter(const gt4mi_field* dst, const gt4mi_field* src, int nfields, const double* response, const int64_t* response_extent,
                       const double* twiddles, double* result, const int64_t extent[3], int axis, int elem_size, int mode, int flags,
                       hipStream_t stream, int* path, int* launches) {
    if (launches) *launches = 0;
    if (path) *path = -1;
    const char* const entry = FILTER_CHECKS.entry;
    const bool spectrum = mode == GT4MI_FILTER_SPECTRUM;
    if (mode != GT4MI_FILTER_APPLY && mode != GT4MI_FILTER_SPECTRUM)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: mode %d is not GT4MI_FILTER_APPLY or GT4MI_FILTER_SPECTRUM", entry, mode);
    if (spectrum && dst != nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: a dst goes with GT4MI_FILTER_APPLY only", entry);
    const gt4mi_field* const written = spectrum ? src : dst;  // (a spectrum writes no field: its fields stand in both lists)
    int free_axes = 0;
    if (int rc = line_front(
            FILTER_CHECKS, spectrum ? SPECTRUM_ROLES : FILTER_ROLES, written, src, nfields, nullptr, extent, axis, elem_size,
            [&]() -> int {
                const bool unknown = (flags & ~GT4MI_FILTER_DRY_RUN) != 0;
                return unknown ? fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: unknown bits in flags 0x%x", entry, (unsigned)flags) : GT4MI_OK;
            },
            [&]() -> int {
                const int64_t n = extent[axis];
                if (n < 2 || n > (1 << FILTER_MAX_LOG) || (n & (n - 1)) != 0)
                    return fail(GT4MI_ERR_UNSUPPORTED, "%s: a line of %lld points along axis %d: the length must be a power of two from 2 to %d "
                                "(mixed radix is not offered)", entry, (long long)n, axis, 1 << FILTER_MAX_LOG);
                return GT4MI_OK;
            },
            &free_axes))
        return rc;
    const bool dry = (flags & GT4MI_FILTER_DRY_RUN) != 0;
    const int other0 = axis == 0 ? 1 : 0, other1 = axis == 2 ? 1 : 2;  // the two other axes in IJK order
    const int64_t n = extent[axis], nh = n / 2 + 1;
    if (spectrum) {
        if (response != nullptr || response_extent != nullptr)
            return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: a response goes with GT4MI_FILTER_APPLY only", entry);
        if (!dry && result == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: result is null", entry);
    } else {
        if (result != nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: a result goes with GT4MI_FILTER_SPECTRUM only", entry);
        if (response_extent == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: response_extent is null", entry);
        const int others[2] = {other0, other1};
        for (int x = 0; x < 2; ++x)
            if (response_extent[x] != 1 && response_extent[x] != extent[others[x]])
                return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: response extent %lld along axis %d is neither 1 nor the box's %lld", entry,
                            (long long)response_extent[x], others[x], (long long)extent[others[x]]);
        if (!dry && response == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: response is null", entry);
    }
    if (!dry && twiddles == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: twiddles is null", entry);
    const struct {
        const char* name;
        const void* p;
    } tables[3] = {{"response", response}, {"twiddles", twiddles}, {"result", result}};
    for (const auto& t : tables)
        if (reinterpret_cast<uintptr_t>(t.p) % 8 != 0) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: %s is not aligned to 8 bytes", entry, t.name);
    if (extent[0] == 0 || extent[1] == 0 || extent[2] == 0) return GT4MI_OK;
    // what is read by every pair, against everything that is written
    NamedSpan shared[2] = {};
    int nshared = 0;
    if (response != nullptr) {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(response);
        shared[nshared++] = NamedSpan{"response", ByteSpan{lo, lo + (uintptr_t)(response_extent[0] * response_extent[1] * nh) * sizeof(double)}};
    }
    if (twiddles != nullptr) {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(twiddles);
        shared[nshared++] = NamedSpan{"twiddles", ByteSpan{lo, lo + (uintptr_t)n * sizeof(double)}};
    }
    if (!spectrum) {
        if (int rc = check_pairs_disjoint(entry, dst, src, nfields, extent, extent, elem_size, elem_size, nullptr, shared, nshared, &FILTER_ROLES))
            return rc;
    } else if (result != nullptr) {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(result);
        const ByteSpan span{lo, lo + (uintptr_t)nfields * 2 * (uintptr_t)(extent[other0] * extent[other1] * nh) * sizeof(double)};
        for (int k = 0; k < nfields; ++k)
            if (spans_overlap(span, box_span(src[k], extent, elem_size))) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: result overlaps field %d", entry, k);
        for (int s = 0; s < nshared; ++s)
            if (spans_overlap(span, shared[s].span)) return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: result overlaps %s", entry, shared[s].name);
    }
    // the path: every field strict; the response loose: unit along the line (it is read by wavenumber, never in lanes along the line),
    // broadcast or not along the two other axes
    LinePlan plan(axis, elem_size);
    for (int k = 0; k < nfields; ++k) {
        if (!spectrum) plan.strict(dst[k]);
        plan.strict(src[k]);
    }
    gt4mi_field as_field{};
    if (!spectrum) {
        as_field.stride[axis] = elem_size;
        as_field.stride[other0] = response_extent[0] == 1 ? 0 : response_extent[1] * nh * (int64_t)sizeof(double);
        as_field.stride[other1] = response_extent[1] == 1 ? 0 : nh * (int64_t)sizeof(double);
        plan.loose(&as_field);
    }
    LineGrid g;
    if (int rc = line_grid(entry, plan, extent, 1 << FILTER_SMALL_LOG, &g)) return rc;
    if (path) *path = g.path;
    if (launches) *launches = (int)cdiv(nfields, PAIR_MAX_FIELDS);
    if (dry) return GT4MI_OK;
    FilterArgs a{};
    a.n = (int)n, a.na = g.na, a.nb = g.nb, a.scale = 1.0 / (double)n;
    while ((1 << a.logn) < a.n) ++a.logn;
    a.spectrum = spectrum, a.across = g.path == GT4MI_LINE_PATH_LANES;
    a.twiddles = twiddles;
    const bool swap = g.order[1] > g.order[2];  // A is the higher of the two other axes
    if (!spectrum) {
        const int64_t s0 = as_field.stride[other0] / (int64_t)sizeof(double), s1 = as_field.stride[other1] / (int64_t)sizeof(double);
        a.response = response, a.ra = swap ? s1 : s0, a.rb = swap ? s0 : s1;
    } else {
        const int64_t s0 = extent[other1] * nh, s1 = nh;
        a.qa = swap ? s1 : s0, a.qb = swap ? s0 : s1, a.qp = extent[other0] * extent[other1] * nh;
    }
    const bool big = a.logn > FILTER_SMALL_LOG;
    const int64_t per_group = (int64_t)1 << ((big ? FILTER_MAX_LOG : FILTER_SMALL_LOG) - a.logn);
    int next = 0, first = 0;
    while (next_pair_batch(a, written, src, &next, nfields, elem_size, g.order)) {
        // 16-byte lanes on TILES: every line of every field of the launch starts on a 16-byte boundary and holds a multiple of 16 bytes
        bool wide = g.path == GT4MI_LINE_PATH_TILES && (n * elem_size) % 16 == 0;
        for (int k = first; k < next && wide; ++k)
            for (const gt4mi_field* f : {&written[k], &src[k]}) {
                wide = wide && reinterpret_cast<uintptr_t>(origin_ptr(*f)) % 16 == 0;
                for (int ax = 0; ax < 3; ++ax) wide = wide && (ax == axis || extent[ax] == 1 || f->stride[ax] % 16 == 0);
            }
        a.wide = wide;
        if (spectrum) a.result = result + (int64_t)first * 2 * a.qp;
        const dim3 grid((unsigned)cdiv(g.lines, per_group), (unsigned)a.nf);
        with_item_type(elem_size, [&](auto t) {
            using T = decltype(t);
            if (big) hipLaunchKernelGGL((line_filter_kernel<T, true>), grid, dim3(FILTER_BLOCK), 0, stream, a);
            else hipLaunchKernelGGL((line_filter_kernel<T, false>), grid, dim3(FILTER_BLOCK), 0, stream, a);
        });
        GT4MI_HIP_CHECK(hipGetLastError());
        first = next;
    }
    return GT4MI_OK;
}

}  // namespace gt4mi
