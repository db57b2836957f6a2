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

#include "line_geometry.hip.h"

#pragma clang fp contract(off)

namespace gt4mi {

constexpr int LINE_BLOCK = 256;      // lanes (= lines) of a workgroup on the LANES / ITEMS paths
constexpr int LINE_AHEAD = 4;        // steps whose loads are in flight on the LANES path

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
    const LineLane l = line_lane(LINE_BLOCK, blockIdx.x, a.na, (int64_t)a.na * a.nb);
    if (!l.ok) return;
    const int64_t line = l.line, ia = l.ia(), ib = l.ib();
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

// ---- TILES (the tiles and their moves: line_geometry.hip.h) --------------------------------------------------------------
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
    const LineLane l = line_lane(LINE_TILE_LINES, blockIdx.x, a.na, (int64_t)a.na * a.nb);
    const bool ok = l.ok;
    const int64_t mine = l.mine(), ia = l.ia(), ib = l.ib();
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

// every check, then (unless `flags` carries GT4MI_LINE_DRY_RUN) the launches
inline int line_solve(const gt4mi_field* out, const gt4mi_field* rhs, int nfields, const gt4mi_field* lower, const gt4mi_field* diag,
                      const gt4mi_field* upper, const int64_t extent[3], int axis, int elem_size, int flags, void* workspace,
                      int64_t workspace_bytes, hipStream_t stream, int64_t* workspace_needed, int* path, int* launches) {
    if (launches) *launches = 0;
    if (workspace_needed) *workspace_needed = 0;
    if (path) *path = -1;
    const bool periodic = (flags & GT4MI_LINE_PERIODIC) != 0, dry = (flags & GT4MI_LINE_DRY_RUN) != 0;
    const char* const missing = lower == nullptr ? "lower" : diag == nullptr ? "diag" : upper == nullptr ? "upper" : nullptr;
    const auto empty = [&] { return extent[0] == 0 || extent[1] == 0 || extent[2] == 0; };
    int coef_free = 0;  // a 1-d coefficient
    if (int rc = line_front(
            LINE_CHECKS, LINE_ROLES, out, rhs, nfields, missing, extent, axis, elem_size,
            [&]() -> int {
                const bool unknown = (flags & ~(GT4MI_LINE_PERIODIC | GT4MI_LINE_DRY_RUN)) != 0;
                return unknown ? fail(GT4MI_ERR_INVALID_ARGUMENT, "line_solve: unknown bits in flags 0x%x", (unsigned)flags) : GT4MI_OK;
            },
            [&]() -> int {
                if (!periodic || empty() || extent[axis] >= 3) return GT4MI_OK;
                return fail(GT4MI_ERR_INVALID_ARGUMENT, "line_solve: a periodic line needs at least 3 points, the extent along axis %d is %lld",
                            axis, (long long)extent[axis]);
            },
            &coef_free))
        return rc;
    const int64_t n = extent[axis];
    const gt4mi_field* const coef[3] = {lower, diag, upper};
    const char* const coef_names[3] = {"lower", "diag", "upper"};
    for (int c = 0; c < 3; ++c)
        if (int rc = check_box_field(LINE_CHECKS, coef_names[c], 0, *coef[c], extent, elem_size, false, coef_free)) return rc;
    if (empty()) return GT4MI_OK;
    const NamedSpan shared[3] = {{"lower", box_span(*lower, extent, elem_size)}, {"diag", box_span(*diag, extent, elem_size)},
                                 {"upper", box_span(*upper, extent, elem_size)}};
    if (int rc = check_pairs_disjoint("line_solve", out, rhs, nfields, extent, extent, elem_size, elem_size, nullptr, shared, 3, &LINE_ROLES))
        return rc;
    LinePlan plan(axis, elem_size);
    for (int k = 0; k < nfields; ++k) plan.strict(out[k]), plan.strict(rhs[k]);
    for (int c = 0; c < 3; ++c) plan.loose(coef[c]);
    LineGrid g;
    if (int rc = line_grid("line_solve", plan, extent, LINE_BLOCK, &g)) return rc;
    // a workspace row: the lines rounded up to whole 256-byte segments
    const int64_t pitch = cdiv(g.lines, 256 / elem_size) * (256 / elem_size);
    const int64_t needed = pitch * n * elem_size * (periodic ? 2 : 1);
    if (workspace_needed) *workspace_needed = needed;
    if (path) *path = g.path;
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
    a.lo = shared_field(*lower, elem_size, g.order), a.di = shared_field(*diag, elem_size, g.order), a.up = shared_field(*upper, elem_size, g.order);
    a.cp = static_cast<char*>(workspace);
    a.q = a.cp + (periodic ? pitch * n * elem_size : 0);
    a.pitch = pitch;
    a.n = (int)n, a.na = g.na, a.nb = g.nb, a.periodic = periodic;
    // (a later launch of the call forms cp and q again, in the same workspace and to the same bits: launches are stream-ordered)
    int next = 0;
    while (next_pair_batch(a, out, rhs, &next, nfields, elem_size, g.order)) {
        with_item_type(elem_size, [&](auto t) {
            using T = decltype(t);
            with_pair_entries(a.nf, [&](auto nf) {
                constexpr int NF = decltype(nf)::value;
                line_launch(g.path, g.lines, LINE_BLOCK, line_solve_tile_kernel<T, NF>, line_solve_march_kernel<T, NF, LINE_AHEAD>,
                            line_solve_march_kernel<T, NF, 1>, a, stream);
            });
        });
        GT4MI_HIP_CHECK(hipGetLastError());
    }
    return GT4MI_OK;
}

}  // namespace gt4mi
