// Tridiagonal line solves along I, J or K: for every line of the box along `axis`, a[m] x[m-1] + b[m] x[m] + c[m] x[m+1] = d[m],
// m = 0 .. n-1, for up to 8 (out, rhs) pairs per launch that share ONE set of coefficients; optionally closed periodically.
//
// NEW component.  The reference has one Thomas solve, the K-only `tridiagonal_solver` stencil (tridiag.hip.h), which takes one
// right-hand side, rewrites its coefficients and has no periodic closure; GTScript cannot write a recurrence along I or J at all.
//
// THE ARITHMETIC CONTRACT (include/gt4py_amd.h states it, tests/line_solve_ref.py restates it in plain Python).  All arithmetic
// is in the fields' type T, one rounding per operation, no FMA (-ffp-contract=off and the pragma below), division is IEEE
// division, there is no reciprocal.  Not periodic:
//   m = 0 :  cp[0] = c[0] / b[0]                     dp[0] = d[0] / b[0]
//   m >= 1:  den = b[m] - a[m] * cp[m-1]
//            cp[m] = c[m] / den   (not for m = n-1)  dp[m] = (d[m] - a[m] * dp[m-1]) / den
//   x[n-1] = dp[n-1] ;  x[m] = dp[m] - cp[m] * x[m+1]   for m = n-2 .. 0
// (tridiag_kernel's arithmetic: one right-hand side gives the bits of the K solve on the permuted data).  a[0] and c[n-1] are
// never read.  Periodic (n >= 3; Sherman-Morrison with alpha = c[n-1], beta = a[0], gamma = -b[0]):
//   bb[0] = b[0] - gamma ;  bb[n-1] = b[n-1] - (alpha * beta) / gamma ;  bb[m] = b[m] otherwise
//   q = the non-periodic solution with diagonal bb and right-hand side (gamma, 0, ..., 0, alpha)     [once per line]
//   y = the same with right-hand side d                                                             [per field]
//   fact = (y[0] + (beta * y[n-1]) / gamma) / ((1 + q[0]) + (beta * q[n-1]) / gamma) ;  x[m] = y[m] - fact * q[m]
// c[n-1] is read as alpha only, cp[n-1] is not formed; the zeros of q's right-hand side take part as 0 - a[m] * qp[m-1].
//
// WHY IT ENDS AND STAYS IN ITS BOX WHATEVER THE DATA HOLDS: every loop counts to n (or to the items of a tile), which the host has
// checked against every field's shape; no loop bound and no address depends on field data.  A zero or NaN pivot gives that line
// the IEEE result and no other line reads it: a lane owns its line from the first load to the last store.
//
// THE WORKSPACE holds cp, and for a periodic call q behind it: item [m][line], lines contiguous (line = a + na * b over the two
// other axes, a the lane axis), a row of `pitch` items.  Lanes are lines, so both sweeps read and write it coalesced without LDS.
// A lane writes every item of its line before it reads it: the result does not depend on what the workspace held.  dp (y) lives
// in `out` itself, which is why out[n] may BE rhs[n] (the same box: pointer, strides) and may meet nothing else.
//
// THREE PATHS, chosen by the host from the strides (reported as GT4MI_LINE_PATH_*):
//   LANES  an axis OTHER than the line axis has unit stride in every field (0 = broadcast in a coefficient): lanes run along it,
//          every step of the march is a coalesced row segment as in tridiag_kernel; the loads of the next LINE_AHEAD steps are
//          issued before the dependent arithmetic; the field loop sits inside the step (den, cp once per step).
//   TILES  the LINE axis has unit stride in every field: a lane owns a line, a workgroup IS one wave and moves tiles of 64 lines
//          x one 128-byte run along the line through LDS (field_copy.hip.h's transposition and padded pitch: a row of R items
//          plus one, lane l on bank (l + r) mod 32), global access coalesced along the line.  Per tile the coefficients are
//          staged once (den replaces b in its tile), then every field in turn goes through ONE field tile.  The tiles are
//          private to the wave: the barriers are wave barriers (the workgroup has 64 lanes), none spans waves.
//   ITEMS  anything else (no common unit-stride axis, fields that disagree): one lane per line, item by item, uncoalesced: slow.
//          It is the LANES kernel without look-ahead.
// No scratch, no atomics, no ordering between workgroups, no host synchronisation.
#pragma once

#include <type_traits>

#include "common.hip.h"
#include "field_args.hip.h"

#pragma clang fp contract(off)

namespace gt4mi {

constexpr int LINE_BLOCK = 256;      // lanes (= lines) of a workgroup on the LANES / ITEMS paths
constexpr int LINE_AHEAD = 4;        // steps whose loads are in flight on the LANES path
constexpr int LINE_TILE_LINES = 64;  // TILES: lines of a tile = lanes of the wave that owns it
constexpr int LINE_TILE_BYTES = 128; // TILES: the run along the line a tile covers

// Every stride (ITEMS) is permuted by the host: [0] the line axis, [1] the lane axis A, [2] the remaining axis B.
struct LineArgs {
    PairEntry e[PAIR_MAX_FIELDS];  // dst / d: out and its strides, src / s: rhs and its strides
    SharedField lo, di, up;        // stride 0 along A / B broadcasts a 1-d coefficient
    char* cp;       // workspace: cp[m * pitch + line]
    char* q;        // periodic: q[m * pitch + line]
    int64_t pitch;  // items of a workspace row
    int n, na, nb, nf, periodic;
};

// LANES (AHEAD = LINE_AHEAD) and ITEMS (AHEAD = 1).  NF: entries the kernel has registers for (a.nf <= NF).
template <typename T, int NF, int AHEAD>
__global__ void __launch_bounds__(LINE_BLOCK)
line_solve_march_kernel(const LineArgs a) {
    const int64_t line = (int64_t)blockIdx.x * LINE_BLOCK + threadIdx.x;
    if (line >= (int64_t)a.na * a.nb) return;
    const int64_t ib = line / a.na, ia = line - ib * a.na;
    const int n = a.n, nf = a.nf;
    const bool periodic = a.periodic != 0;
    const T* const pa = reinterpret_cast<const T*>(a.lo.p) + ia * a.lo.s[1] + ib * a.lo.s[2];
    const T* const pb = reinterpret_cast<const T*>(a.di.p) + ia * a.di.s[1] + ib * a.di.s[2];
    const T* const pc = reinterpret_cast<const T*>(a.up.p) + ia * a.up.s[1] + ib * a.up.s[2];
    const int64_t sa = a.lo.s[0], sb = a.di.s[0], sc = a.up.s[0], pitch = a.pitch;
    T* const cp = reinterpret_cast<T*>(a.cp) + line;
    T* const qq = reinterpret_cast<T*>(a.q) + line;  // (only touched when periodic)
    const T* rhs[NF];
    T* out[NF];
    T dprev[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        rhs[f] = nullptr, out[f] = nullptr, dprev[f] = T(0);
        if (f < nf) {
            rhs[f] = reinterpret_cast<const T*>(a.e[f].src) + ia * a.e[f].s[1] + ib * a.e[f].s[2];
            out[f] = reinterpret_cast<T*>(a.e[f].dst) + ia * a.e[f].d[1] + ib * a.e[f].d[2];
        }
    }

    // ---- forward, m = 0 ----
    T alpha = T(0), beta = T(0), gamma = T(1), cprev = T(0), qprev = T(0);
    {
        const T b0 = pb[0];
        T bb0 = b0;
        if (periodic) {
            gamma = -b0, beta = pa[0], alpha = pc[(int64_t)(n - 1) * sc];
            bb0 = b0 - gamma;
            qprev = gamma / bb0;
            qq[0] = qprev;
        }
        if (n > 1) {
            cprev = pc[0] / bb0;
            cp[0] = cprev;
        }
#pragma unroll
        for (int f = 0; f < NF; ++f)
            if (f < nf) {
                dprev[f] = rhs[f][0] / bb0;
                out[f][0] = dprev[f];
            }
    }
    // ---- forward, m >= 1: the loads of AHEAD steps, then their arithmetic ----
    for (int m0 = 1; m0 < n; m0 += AHEAD) {
        T va[AHEAD], vb[AHEAD], vc[AHEAD], vd[NF][AHEAD];
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const int m = m0 + u;
            va[u] = vb[u] = vc[u] = T(0);
            if (m < n) {
                va[u] = pa[(int64_t)m * sa], vb[u] = pb[(int64_t)m * sb];
                if (m < n - 1) vc[u] = pc[(int64_t)m * sc];
            }
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                vd[f][u] = T(0);
                if (f < nf && m < n) vd[f][u] = rhs[f][(int64_t)m * a.e[f].s[0]];
            }
        }
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const int m = m0 + u;
            if (m < n) {
                const bool last = m == n - 1;
                T bm = vb[u];
                if (periodic && last) bm = vb[u] - (alpha * beta) / gamma;
                const T den = bm - va[u] * cprev;
                if (!last) {
                    cprev = vc[u] / den;
                    cp[(int64_t)m * pitch] = cprev;
                }
#pragma unroll
                for (int f = 0; f < NF; ++f)
                    if (f < nf) {
                        dprev[f] = (vd[f][u] - va[u] * dprev[f]) / den;
                        out[f][(int64_t)m * a.e[f].d[0]] = dprev[f];
                    }
                if (periodic) {
                    const T um = last ? alpha : T(0);
                    qprev = (um - va[u] * qprev) / den;
                    qq[(int64_t)m * pitch] = qprev;
                }
            }
        }
    }

    // ---- backward: x[n-1] = dp[n-1] is in place already; y[n-1] and q[n-1] stay in registers for fact ----
    T x[NF], ylast[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) x[f] = ylast[f] = dprev[f];
    T qx = qprev;
    const T qlast = qprev;
    for (int m0 = n - 2; m0 >= 0; m0 -= AHEAD) {
        T wc[AHEAD], wq[AHEAD], wd[NF][AHEAD];
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const int m = m0 - u;
            wc[u] = wq[u] = T(0);
            if (m >= 0) {
                wc[u] = cp[(int64_t)m * pitch];
                if (periodic) wq[u] = qq[(int64_t)m * pitch];
            }
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                wd[f][u] = T(0);
                if (f < nf && m >= 0) wd[f][u] = out[f][(int64_t)m * a.e[f].d[0]];
            }
        }
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const int m = m0 - u;
            if (m >= 0) {
#pragma unroll
                for (int f = 0; f < NF; ++f)
                    if (f < nf) {
                        x[f] = wd[f][u] - wc[u] * x[f];
                        out[f][(int64_t)m * a.e[f].d[0]] = x[f];
                    }
                if (periodic) {
                    qx = wq[u] - wc[u] * qx;
                    qq[(int64_t)m * pitch] = qx;
                }
            }
        }
    }
    if (!periodic) return;

    // ---- the periodic correction: a third pass over the line ----
    const T qden = (T(1) + qx) + (beta * qlast) / gamma;
    T fact[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) fact[f] = (x[f] + (beta * ylast[f]) / gamma) / qden;
    for (int m0 = 0; m0 < n; m0 += AHEAD) {
        T wq[AHEAD], wy[NF][AHEAD];
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const int m = m0 + u;
            wq[u] = T(0);
            if (m < n) wq[u] = qq[(int64_t)m * pitch];
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                wy[f][u] = T(0);
                if (f < nf && m < n) wy[f][u] = out[f][(int64_t)m * a.e[f].d[0]];
            }
        }
#pragma unroll
        for (int u = 0; u < AHEAD; ++u) {
            const int m = m0 + u;
            if (m < n) {
#pragma unroll
                for (int f = 0; f < NF; ++f)
                    if (f < nf) out[f][(int64_t)m * a.e[f].d[0]] = wy[f][u] - fact[f] * wq[u];
            }
        }
    }
}

// ---- TILES ------------------------------------------------------------------------------------------------------------------
// One wave = one workgroup = LINE_TILE_LINES consecutive lines.  tile[l][r]: line l of the wave, item r of the run.
template <typename T>
struct LineTile {
    static constexpr int R = LINE_TILE_BYTES / (int)sizeof(T);   // items of a run: 32 (float) / 16 (double)
    static constexpr int PITCH = R + 1;                          // odd in items of 4 / 8 bytes: see the header
    static constexpr int LINES_PER_PASS = LINE_TILE_LINES / R;   // lines one load / store instruction of the wave covers
    static constexpr int PASSES = R;                             // = LINE_TILE_LINES / LINES_PER_PASS
};

// Move the run [m0, m0 + R) of the wave's lines between global memory and a tile; `off` is THIS lane's line offset (items) in the
// field (the line axis has item stride 1 on this path), `ok` whether this lane's line exists.  Lane l moves item (l % R) of line
// (pass * LINES_PER_PASS + l / R): consecutive lanes on consecutive items.  Item `skip` of the line (-1: none) is not moved: a[0] and
// c[n-1], which the contract never reads, stay out of the tile (their slots are never used).  A load takes a pointer to const.
template <typename T, bool LOAD>
__device__ __forceinline__ void line_tile_move(T (*tile)[LineTile<T>::PITCH], std::conditional_t<LOAD, const T, T>* base, int64_t off, bool ok,
                                               int m0, int n, int skip = -1) {
    using L = LineTile<T>;
    const int lane = (int)threadIdx.x;
    const int r = lane % L::R, sub = lane / L::R;
    // (offsets as two 32-bit halves through the cross-lane read)
    const int off_lo = (int)(uint32_t)(uint64_t)off, off_hi = (int)(uint32_t)((uint64_t)off >> 32);
    // every load of the move is issued before the first LDS store (a wave is alone on its SIMD: nothing else hides the latency)
    T v[L::PASSES];
    uint32_t there = 0;
#pragma unroll
    for (int p = 0; p < L::PASSES; ++p) {
        const int l = p * L::LINES_PER_PASS + sub;
        const int64_t o = (int64_t)(((uint64_t)(uint32_t)__shfl(off_hi, l) << 32) | (uint64_t)(uint32_t)__shfl(off_lo, l));
        const bool here = __shfl((int)ok, l) != 0 && m0 + r < n && m0 + r != skip;
        there |= (uint32_t)here << p;
        if constexpr (LOAD) {
            v[p] = T(0);
            if (here) v[p] = base[o + (m0 + r)];
        } else {
            if (here) base[o + (m0 + r)] = tile[l][r];
        }
    }
    if constexpr (LOAD) {
#pragma unroll
        for (int p = 0; p < L::PASSES; ++p)
            if (there >> p & 1u) tile[p * L::LINES_PER_PASS + sub][r] = v[p];
    }
}

template <typename T, int NF>
__global__ void __launch_bounds__(LINE_TILE_LINES)
line_solve_tile_kernel(const LineArgs a) {
    using L = LineTile<T>;
    constexpr int R = L::R;
    __shared__ T ta[LINE_TILE_LINES][L::PITCH];  // a
    __shared__ T tb[LINE_TILE_LINES][L::PITCH];  // b, then den
    __shared__ T tc[LINE_TILE_LINES][L::PITCH];  // c; cp / q of the run in the later passes
    __shared__ T tf[LINE_TILE_LINES][L::PITCH];  // the field in hand
    const int lane = (int)threadIdx.x;
    const int64_t lines = (int64_t)a.na * a.nb;
    const int64_t line = (int64_t)blockIdx.x * LINE_TILE_LINES + lane;
    const bool ok = line < lines;
    const int64_t mine = ok ? line : 0;  // (a lane without a line computes on line 0's addresses and neither loads nor stores)
    const int64_t ib = mine / a.na, ia = mine - ib * a.na;
    const int n = a.n, nf = a.nf;
    const bool periodic = a.periodic != 0;
    const int64_t pitch = a.pitch;
    T* const cp = reinterpret_cast<T*>(a.cp) + mine;
    T* const qq = reinterpret_cast<T*>(a.q) + mine;
    const int64_t oa = ia * a.lo.s[1] + ib * a.lo.s[2], ob = ia * a.di.s[1] + ib * a.di.s[2], oc = ia * a.up.s[1] + ib * a.up.s[2];
    const T* const ga = reinterpret_cast<const T*>(a.lo.p);
    const T* const gb = reinterpret_cast<const T*>(a.di.p);
    const T* const gc = reinterpret_cast<const T*>(a.up.p);
    int64_t orhs[NF], oout[NF];
    T dprev[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        orhs[f] = oout[f] = 0, dprev[f] = T(0);
        if (f < nf) orhs[f] = ia * a.e[f].s[1] + ib * a.e[f].s[2], oout[f] = ia * a.e[f].d[1] + ib * a.e[f].d[2];
    }
    const int tiles = (n + R - 1) / R;

    // ---- forward ----
    T alpha = T(0), beta = T(0), gamma = T(1), cprev = T(0), qprev = T(0);
    if (periodic && ok) {
        beta = ga[oa];
        alpha = gc[oc + (n - 1)];
    }
    for (int t = 0; t < tiles; ++t) {
        const int m0 = t * R;
        __syncthreads();  // (the marches of the tile before are done with the tiles)
        line_tile_move<T, true>(ta, ga, oa, ok, m0, n, 0);      // (a[0]: read as beta only, above)
        line_tile_move<T, true>(tb, gb, ob, ok, m0, n);
        line_tile_move<T, true>(tc, gc, oc, ok, m0, n, n - 1);  // (c[n-1]: read as alpha only)
        __syncthreads();
        if (ok) {
            for (int r = 0; r < R && m0 + r < n; ++r) {
                const int m = m0 + r;
                const bool last = m == n - 1;
                T den;
                if (m == 0) {
                    den = tb[lane][0];
                    if (periodic) {
                        gamma = -den;
                        den = den - gamma;
                    }
                } else {
                    T bm = tb[lane][r];
                    if (periodic && last) bm = bm - (alpha * beta) / gamma;
                    den = bm - ta[lane][r] * cprev;
                }
                tb[lane][r] = den;
                if (!last) {
                    cprev = tc[lane][r] / den;
                    cp[(int64_t)m * pitch] = cprev;
                }
                if (periodic) {
                    if (m == 0) qprev = gamma / den;
                    else qprev = ((last ? alpha : T(0)) - ta[lane][r] * qprev) / den;
                    qq[(int64_t)m * pitch] = qprev;
                }
            }
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            if (f < nf) {
                __syncthreads();  // (tf is free: the stores of the field before have read it)
                line_tile_move<T, true>(tf, reinterpret_cast<const T*>(a.e[f].src), orhs[f], ok, m0, n);
                __syncthreads();
                if (ok) {
                    for (int r = 0; r < R && m0 + r < n; ++r) {
                        if (m0 + r == 0) dprev[f] = tf[lane][0] / tb[lane][0];
                        else dprev[f] = (tf[lane][r] - ta[lane][r] * dprev[f]) / tb[lane][r];
                        tf[lane][r] = dprev[f];
                    }
                }
                __syncthreads();
                line_tile_move<T, false>(tf, reinterpret_cast<T*>(a.e[f].dst), oout[f], ok, m0, n);
            }
        }
    }

    // ---- backward: q in the workspace (lanes are lines: coalesced as it is), the fields tile by tile ----
    T x[NF], ylast[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) x[f] = ylast[f] = dprev[f];
    T qx = qprev;
    const T qlast = qprev;
    for (int t = tiles - 1; t >= 0; --t) {
        const int m0 = t * R;
        __syncthreads();
        if (ok) {  // cp (and the finished q) of the run into this lane's own row of tc: no hand-over between lanes
            for (int r = R - 1; r >= 0; --r) {
                const int m = m0 + r;
                if (m >= n - 1) continue;
                const T c = cp[(int64_t)m * pitch];
                tc[lane][r] = c;
                if (periodic) {
                    qx = qq[(int64_t)m * pitch] - c * qx;
                    qq[(int64_t)m * pitch] = qx;
                }
            }
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            if (f < nf) {
                __syncthreads();
                line_tile_move<T, true>(tf, reinterpret_cast<const T*>(a.e[f].dst), oout[f], ok, m0, n);
                __syncthreads();
                if (ok) {
                    for (int r = R - 1; r >= 0; --r) {
                        const int m = m0 + r;
                        if (m >= n - 1) continue;  // (x[n-1] = dp[n-1] is what the tile holds)
                        x[f] = tf[lane][r] - tc[lane][r] * x[f];
                        tf[lane][r] = x[f];
                    }
                }
                __syncthreads();
                line_tile_move<T, false>(tf, reinterpret_cast<T*>(a.e[f].dst), oout[f], ok, m0, n);
            }
        }
    }
    if (!periodic) return;

    // ---- the periodic correction ----
    const T qden = (T(1) + qx) + (beta * qlast) / gamma;
    T fact[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) fact[f] = (x[f] + (beta * ylast[f]) / gamma) / qden;
    for (int t = 0; t < tiles; ++t) {
        const int m0 = t * R;
        __syncthreads();
        if (ok)
            for (int r = 0; r < R && m0 + r < n; ++r) tc[lane][r] = qq[(int64_t)(m0 + r) * pitch];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            if (f < nf) {
                __syncthreads();
                line_tile_move<T, true>(tf, reinterpret_cast<const T*>(a.e[f].dst), oout[f], ok, m0, n);
                __syncthreads();
                if (ok)
                    for (int r = 0; r < R && m0 + r < n; ++r) tf[lane][r] = tf[lane][r] - fact[f] * tc[lane][r];
                __syncthreads();
                line_tile_move<T, false>(tf, reinterpret_cast<T*>(a.e[f].dst), oout[f], ok, m0, n);
            }
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
const BoxChecks LINE_CHECKS = {"line_solve", "extent", "only a rhs or a coefficient may be broadcast", false, false};
const PairRoles LINE_ROLES = {"out", "rhs", true};  // an out may BE its own rhs (the same box), and meet nothing else

template <typename T>
inline void line_launch(const LineArgs& a, int path, hipStream_t stream) {
    const int64_t lines = (int64_t)a.na * a.nb;
    with_pair_entries(a.nf, [&](auto nf) {
        constexpr int NF = decltype(nf)::value;
        if (path == GT4MI_LINE_PATH_TILES)
            hipLaunchKernelGGL((line_solve_tile_kernel<T, NF>), dim3((unsigned)cdiv(lines, LINE_TILE_LINES)), dim3(LINE_TILE_LINES), 0, stream, a);
        else if (path == GT4MI_LINE_PATH_LANES)
            hipLaunchKernelGGL((line_solve_march_kernel<T, NF, LINE_AHEAD>), dim3((unsigned)cdiv(lines, LINE_BLOCK)), dim3(LINE_BLOCK), 0, stream, a);
        else
            hipLaunchKernelGGL((line_solve_march_kernel<T, NF, 1>), dim3((unsigned)cdiv(lines, LINE_BLOCK)), dim3(LINE_BLOCK), 0, stream, a);
    });
}

// The path of a call and its lane axis: `unit[ax]` = every field of the call has unit item stride along ax (a coefficient may
// also be broadcast along an axis that is not the line axis).  `coef`: the `ncoef` fields every pair reads (line_scan: its weight, or none).
inline int line_plan(const gt4mi_field* out, const gt4mi_field* rhs, int nfields, const gt4mi_field* const* coef, int ncoef,
                     const int64_t extent[3], int axis, int elem_size, int* lane_axis) {
    const int other0 = axis == 0 ? 1 : 0, other1 = axis == 2 ? 1 : 2;
    bool unit[3];
    for (int ax = 0; ax < 3; ++ax) {
        unit[ax] = true;
        for (int n = 0; n < nfields; ++n)
            if (out[n].stride[ax] != elem_size || rhs[n].stride[ax] != elem_size) unit[ax] = false;
        for (int c = 0; c < ncoef; ++c)
            if (coef[c]->stride[ax] != elem_size && !(ax != axis && coef[c]->stride[ax] == 0)) unit[ax] = false;
    }
    *lane_axis = other0;
    if (unit[axis] && extent[axis] > 1) return GT4MI_LINE_PATH_TILES;
    for (int ax : {other0, other1})
        if (unit[ax] && extent[ax] > 1) {
            *lane_axis = ax;
            return GT4MI_LINE_PATH_LANES;
        }
    return GT4MI_LINE_PATH_ITEMS;
}

// every check, then (unless `flags` carries GT4MI_LINE_DRY_RUN) the launches
inline int line_solve(const gt4mi_field* out, const gt4mi_field* rhs, int nfields, const gt4mi_field* lower, const gt4mi_field* diag,
                      const gt4mi_field* upper, const int64_t extent[3], int axis, int elem_size, int flags, void* workspace,
                      int64_t workspace_bytes, hipStream_t stream, int64_t* workspace_needed, int* path, int* launches) {
    if (launches) *launches = 0;
    if (workspace_needed) *workspace_needed = 0;
    if (path) *path = -1;
    if (out == nullptr || rhs == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "line_solve: %s is null", out == nullptr ? "out" : "rhs");
    if (lower == nullptr || diag == nullptr || upper == nullptr)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "line_solve: %s is null", lower == nullptr ? "lower" : diag == nullptr ? "diag" : "upper");
    if (extent == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "line_solve: extent is null");
    if (nfields < 1) return fail(GT4MI_ERR_INVALID_ARGUMENT, "line_solve: nfields = %d, at least one pair is needed", nfields);
    for (int ax = 0; ax < 3; ++ax)
        if (extent[ax] < 0 || extent[ax] > INT32_MAX)
            return fail(GT4MI_ERR_INVALID_ARGUMENT, "line_solve: invalid extent %lld along axis %d", (long long)extent[ax], ax);
    if (axis < 0 || axis > 2) return fail(GT4MI_ERR_INVALID_ARGUMENT, "line_solve: axis %d is not 0 (I), 1 (J) or 2 (K)", axis);
    if (flags & ~(GT4MI_LINE_PERIODIC | GT4MI_LINE_DRY_RUN))
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "line_solve: unknown bits in flags 0x%x", (unsigned)flags);
    if (elem_size != 4 && elem_size != 8)
        return fail(GT4MI_ERR_UNSUPPORTED, "line_solve: item size %d is not supported (float32 or float64)", elem_size);
    const bool periodic = (flags & GT4MI_LINE_PERIODIC) != 0, dry = (flags & GT4MI_LINE_DRY_RUN) != 0;
    const int64_t n = extent[axis];
    const bool empty = extent[0] == 0 || extent[1] == 0 || extent[2] == 0;
    if (periodic && !empty && n < 3)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "line_solve: a periodic line needs at least 3 points, the extent along axis %d is %lld", axis,
                    (long long)n);
    const int coef_free = 7 & ~(1 << axis);  // a 1-d coefficient: stride 0 along the two other axes, no shape to check there
    const gt4mi_field* const coef[3] = {lower, diag, upper};
    const char* const coef_names[3] = {"lower", "diag", "upper"};
    for (int k = 0; k < nfields; ++k) {
        if (int rc = check_box_field(LINE_CHECKS, "out", k, out[k], extent, elem_size, true)) return rc;
        if (int rc = check_box_field(LINE_CHECKS, "rhs", k, rhs[k], extent, elem_size, false)) return rc;
    }
    for (int c = 0; c < 3; ++c)
        if (int rc = check_box_field(LINE_CHECKS, coef_names[c], 0, *coef[c], extent, elem_size, false, coef_free)) return rc;
    if (empty) return GT4MI_OK;
    const NamedSpan shared[3] = {{"lower", box_span(*lower, extent, elem_size)}, {"diag", box_span(*diag, extent, elem_size)},
                                 {"upper", box_span(*upper, extent, elem_size)}};
    if (int rc = check_pairs_disjoint("line_solve", out, rhs, nfields, extent, extent, elem_size, elem_size, nullptr, shared, 3, &LINE_ROLES))
        return rc;
    int lane_axis = 0;
    const int which = line_plan(out, rhs, nfields, coef, 3, extent, axis, elem_size, &lane_axis);
    const int order[3] = {axis, lane_axis, 3 - axis - lane_axis};
    const int64_t lines = extent[order[1]] * extent[order[2]];
    if (lines > (int64_t)INT32_MAX - LINE_BLOCK) return fail(GT4MI_ERR_UNSUPPORTED, "line_solve: too many lines for one launch");
    // a workspace row: the lines rounded up to whole 256-byte segments
    const int64_t pitch = cdiv(lines, 256 / elem_size) * (256 / elem_size);
    const int64_t needed = pitch * n * elem_size * (periodic ? 2 : 1);
    if (workspace_needed) *workspace_needed = needed;
    if (path) *path = which;
    if (!dry && workspace == nullptr) return fail(GT4MI_ERR_INVALID_ARGUMENT, "line_solve: workspace is null");
    if (workspace != nullptr) {
        if (workspace_bytes < needed)
            return fail(GT4MI_ERR_INVALID_ARGUMENT, "line_solve: workspace of %lld bytes is too small, %lld are needed", (long long)workspace_bytes,
                        (long long)needed);
        if (reinterpret_cast<uintptr_t>(workspace) % 8 != 0) return fail(GT4MI_ERR_UNSUPPORTED, "line_solve: workspace is not aligned to 8 bytes");
        const ByteSpan w{reinterpret_cast<uintptr_t>(workspace), reinterpret_cast<uintptr_t>(workspace) + (uintptr_t)needed};
        for (int k = 0; k < nfields; ++k) {
            if (spans_overlap(w, box_span(out[k], extent, elem_size))) return fail(GT4MI_ERR_UNSUPPORTED, "line_solve: workspace overlaps out %d", k);
            if (spans_overlap(w, box_span(rhs[k], extent, elem_size))) return fail(GT4MI_ERR_UNSUPPORTED, "line_solve: workspace overlaps rhs %d", k);
        }
        for (int c = 0; c < 3; ++c)
            if (spans_overlap(w, shared[c].span)) return fail(GT4MI_ERR_UNSUPPORTED, "line_solve: workspace overlaps %s", coef_names[c]);
    }
    if (launches) *launches = (int)cdiv(nfields, PAIR_MAX_FIELDS);
    if (dry) return GT4MI_OK;
    LineArgs a{};
    a.lo = shared_field(*lower, elem_size, order), a.di = shared_field(*diag, elem_size, order), a.up = shared_field(*upper, elem_size, order);
    a.cp = static_cast<char*>(workspace);
    a.q = a.cp + (periodic ? pitch * n * elem_size : 0);
    a.pitch = pitch;
    a.n = (int)n, a.na = (int)extent[order[1]], a.nb = (int)extent[order[2]], a.periodic = periodic;
    // (a later launch of the call forms cp and q again, in the same workspace and to the same bits: launches are stream-ordered)
    int next = 0;
    while (next_pair_batch(a, out, rhs, &next, nfields, elem_size, order)) {
        with_item_type(elem_size, [&](auto t) { line_launch<decltype(t)>(a, which, stream); });
        GT4MI_HIP_CHECK(hipGetLastError());
    }
    return GT4MI_OK;
}

}  // namespace gt4mi
