// How a fused distributed step (exchange + stencil, one C call) is laid out on the caller's stream and the plan's side stream:
// the ONE schedule driver behind gt4mi_dist_hdiff_* / gt4mi_dist_lap5_*, and the two time steppers (wide halo, time-skewed),
// which have a choreography of their own.  Host code only; the plan's event pair lives in comm.hip.h (fork_side / mark_done /
// join_side).  Included by gt4mi.hip after the kernel headers.
#pragma once

#include "comm.hip.h"
#include "hdiff.hip.h"
#include "hdiff_ring.hip.h"
#include "lap5.hip.h"
#include "lap5_edge.hip.h"
#include "lap5_push.hip.h"
#include "lap5_ring.hip.h"

namespace gt4mi {

// `f` with its origin moved by (i0, j0): the same storage seen from a sub-domain.
inline gt4mi_field shifted(const gt4mi_field& f, int64_t i0, int64_t j0) {
    gt4mi_field g = f;
    g.origin[0] += i0;
    g.origin[1] += j0;
    return g;
}

// The 5-point stencil on the box [i0, i0 + ei) x [j0, j0 + ej) of the local domain; an empty box launches nothing.
template <typename T, typename W>
inline int lap5_on_box(const gt4mi_field* inp, const gt4mi_field* out, int64_t i0, int64_t j0, int64_t ei, int64_t ej, int64_t dk,
                       int variant, hipStream_t st) {
    if (ei <= 0 || ej <= 0 || dk <= 0) return GT4MI_OK;
    const gt4mi_field a = shifted(*inp, i0, j0), b = shifted(*out, i0, j0);
    const int64_t d[3] = {ei, ej, dk};
    return lap5_run<T, W>(d, &a, &b, variant, st);
}

// What a single-launch shortcut of the "inline" schedule has covered.
enum FusedLaunch { FUSED_NOTHING, FUSED_PACK_AND_INTERIOR, FUSED_WHOLE_STEP };
struct NoShortcut {
    int operator()(hipStream_t, FusedLaunch*) const { return GT4MI_OK; }
};

// One fused step from its four stages, each a closure that enqueues on the stream it is given:
//   pack_first(st)                  pack (direct transport: push) the faces of the first phase
//   interior(st)                    the points that read no ghost cell
//   exchange(st, first_pack_done)   the rest of the exchange
//   ring(st)                        the points that read ghost cells
// ms = the caller's stream, side = plan->stream; everything is complete in ms's order when the step returns, unless the plan
// defers the final join (GT4MI_PLAN_DEFER_JOIN).  The callers have validated their arguments (an empty ring launch) before:
// a step is refused before anything of it is enqueued.  Timelines of every schedule on the 1-GPU self-loop:
// profiles/r1_dist_step_timeline.txt, profiles/r3_dist_*_timeline*.txt.
template <typename PackFirst, typename Interior, typename Exchange, typename Ring, typename Shortcut = NoShortcut>
inline int run_schedule(gt4mi_halo_plan* plan, int schedule, hipStream_t ms, PackFirst&& pack_first, Interior&& interior,
                        Exchange&& exchange, Ring&& ring, Shortcut&& shortcut = Shortcut()) {
    const hipStream_t side = plan->stream;
    switch (schedule) {
        case GT4MI_SCHEDULE_INLINE: {
            // ONE stream, no event: pack (direct transport: the faces are on their way when it ends), the interior, then whatever
            // is left of the exchange (direct: the unpack, whose data arrived long ago) and the ring.  A family may cover the
            // pack and the interior, or the whole step, with a single launch of its own.
            FusedLaunch fused = FUSED_NOTHING;
            if (int rc = shortcut(ms, &fused)) return rc;
            if (fused == FUSED_WHOLE_STEP) return GT4MI_OK;
            if (fused == FUSED_NOTHING) {
                if (int rc = pack_first(ms)) return rc;
                if (int rc = interior(ms)) return rc;
            }
            if (int rc = exchange(ms, /*first_pack_done=*/true)) return rc;
            return ring(ms);
        }
        case GT4MI_SCHEDULE_SWAP:
            // The CALLER's stream carries the chain pack -> send/recv -> unpack -> ring back to back (no cross-stream wait inside
            // it, and it starts at once); the interior runs beside it on the side stream; the caller joins the interior at the end.
            if (int rc = fork_side(plan, ms)) return rc;
            if (int rc = interior(side)) return rc;
            if (int rc = mark_done(plan)) return rc;
            if (int rc = exchange(ms, /*first_pack_done=*/false)) return rc;
            if (int rc = ring(ms)) return rc;
            return join_side(plan, ms);
        case GT4MI_SCHEDULE_SWAP_PACKED:
            // "swap", but the interior forks off AFTER the pack: the send/recv kernel gets a head start on the interior's ramp-up
            // and the pack of strided I faces (8-10 us next to the interior) runs alone.  Host order: the interior is enqueued
            // BEFORE the ring, so that the device has it one launch earlier; the ring depends on the exchange only.
            if (int rc = pack_first(ms)) return rc;
            if (int rc = fork_side(plan, ms)) return rc;
            if (int rc = exchange(ms, /*first_pack_done=*/true)) return rc;
            if (int rc = interior(side)) return rc;
            if (int rc = mark_done(plan)) return rc;
            if (int rc = ring(ms)) return rc;
            return join_side(plan, ms);
        case GT4MI_SCHEDULE_CHAIN:
            // The caller's stream carries NOTHING but the interior; pack -> send/recv -> unpack -> ring run in order on the side
            // stream (the ring writes the output's ring, the interior its interior).  No cross-stream wait lies on the critical
            // path: the join after the interior is already satisfied when the chain fits under it, and back-to-back applies run
            // their interiors back to back (profiles/r3_dist_hdiff_timeline_*.txt).
            if (int rc = fork_side(plan, ms)) return rc;
            if (int rc = interior(ms)) return rc;
            if (int rc = exchange(side, /*first_pack_done=*/false)) return rc;
            if (int rc = ring(side)) return rc;
            if (int rc = mark_done(plan)) return rc;
            return join_side(plan, ms);
        default:  // GT4MI_SCHEDULE_JOIN
            // 1. the first faces are packed ON THE CALLER's STREAM, ahead of the interior: alone the pack takes ~5 us; launched next
            //    to the interior's thousands of workgroups it took 22 us and delayed the whole exchange past the end of the
            //    interior (profiles/r1_dist_step_timeline.txt).  The side stream then only waits for this pack.
            if (int rc = pack_first(ms)) return rc;
            if (int rc = fork_side(plan, ms)) return rc;
            // 2. caller's stream: the interior, which reads no ghost cell
            if (int rc = interior(ms)) return rc;
            // 3. side stream: send / receive / unpack (and the second phase of a two-phase plan) next to the interior
            if (int rc = exchange(side, /*first_pack_done=*/true)) return rc;
            if (int rc = mark_done(plan)) return rc;
            // 4. caller's stream: join (never deferred: the ring needs the ghost cells), then the ring -- one launch
            if (int rc = join_side_now(plan, ms)) return rc;
            return ring(ms);
    }
}

// What every fused step checks about its plan before it looks at the fields.
inline int dist_step_begin(gt4mi_halo_plan* plan, const char* who, int item_size, hipStream_t ms) {
    if (plan->elem_size != item_size)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "%s: the plan moves %d-byte items, the fields hold %d-byte items", who, plan->elem_size,
                    item_size);
    if (int rc = direct_failed(plan)) return rc;
    return ensure_concurrent_stream(plan, ms);
}

// One distributed apply of horizontal diffusion (gt4mi_dist_hdiff_f64 / _f32).
template <typename T>
int dist_hdiff(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* in_field, const gt4mi_field* out_field,
               const gt4mi_field* coeff, double coeff_scalar, int flags, int sides, void* main_stream) {
    if (plan == nullptr || in_field == nullptr || out_field == nullptr || domain == nullptr)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "dist_hdiff: null argument");
    hipStream_t ms = static_cast<hipStream_t>(main_stream);
    if (int rc = dist_step_begin(plan, "dist_hdiff", (int)sizeof(T), ms)) return rc;
    const int none[4] = {0, 0, 0, 0};  // an empty ring validates only (bounds, aliases)
    if (int rc = hdiff_ring_run<T>(domain, in_field, out_field, coeff, coeff_scalar, flags, none, ms)) return rc;

    const int64_t di = domain[0], dj = domain[1], dk = domain[2];
    constexpr int64_t H = 2;  // the stencil's reach
    // W / E: the ring takes a box EW >= 2 columns wide (whole cache lines, J-march strips; hdiff_ring.hip.h) off the interior
    // kernel -- even, so that both parts keep their 16-byte alignment; only where the interior keeps at least as much
    int64_t EW = plan_edge_columns(plan, 16);
    EW = EW < H ? H : EW - EW % 2;
    if (di < 4 * EW) EW = H;
    int64_t lo_i = (sides & 1) ? EW : 0, hi_i = (sides & 2) ? EW : 0, lo_j = (sides & 4) ? H : 0, hi_j = (sides & 8) ? H : 0;
    lo_i = lo_i < di ? lo_i : di;
    hi_i = hi_i < di - lo_i ? hi_i : di - lo_i;
    lo_j = lo_j < dj ? lo_j : dj;
    hi_j = hi_j < dj - lo_j ? hi_j : dj - lo_j;
    const int widths[4] = {(int)lo_i, (int)hi_i, (int)lo_j, (int)hi_j};

    return run_schedule(
        plan, plan_schedule(plan, GT4MI_SCHEDULE_CHAIN), ms,
        [&](hipStream_t st) { return halo_pack_first(plan, in_field, st); },
        [&](hipStream_t st) -> int {
            const int64_t sub[3] = {di - lo_i - hi_i, dj - lo_j - hi_j, dk};
            if (!(sub[0] > 0 && sub[1] > 0 && dk > 0)) return GT4MI_OK;
            const gt4mi_field a = shifted(*in_field, lo_i, lo_j), b = shifted(*out_field, lo_i, lo_j);
            const gt4mi_field c = coeff ? shifted(*coeff, lo_i, lo_j) : gt4mi_field{};
            // 2 of 4 workgroups per CU: the send/recv kernel next to it takes 59 us instead of 190 (3 of 4: 77;
            // profiles/r3_dist_hdiff_timeline_by_schedule_and_throttle.txt, r3_dist_hdiff_edge_width_sweep.txt)
            ScopedLaunchLds throttle(lds_for_workgroups_per_cu(plan_interior_wg_per_cu(plan, 2)));
            return hdiff_run<T>(sub, &a, &b, coeff ? &c : nullptr, coeff_scalar, flags, st);
        },
        [&](hipStream_t st, bool first_pack_done) { return halo_exchange_on(plan, in_field, st, first_pack_done); },
        [&](hipStream_t st) { return hdiff_ring_run<T>(domain, in_field, out_field, coeff, coeff_scalar, flags, widths, st); });
}

// Whether a fused 5-point step on these fields runs its unpack and ring as edge units (gt4mi_dist_lap5_query; nothing is enqueued).
template <typename T>
inline int lap5_edge_units_qualify(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* inp, const gt4mi_field* out, int sides,
                                   bool* ok) {
    View<T> vi, vo;
    EdgeFaces g;
    EdgeCopies cp;
    int phase = 0;
    return lap5_edge_prepare<T>(plan, domain, inp, out, sides, &vi, &vo, &g, &cp, &phase, ok);
}

// One distributed apply of a 5-point stencil (gt4mi_dist_lap5_f64 / _f32): T the fields' type, W the type its literals have.
template <typename T, typename W>
int dist_lap5(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* inp, const gt4mi_field* out, int variant,
              int sides, void* main_stream) {
    if (plan == nullptr || inp == nullptr || out == nullptr || domain == nullptr)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "dist_lap5: null argument");
    hipStream_t ms = static_cast<hipStream_t>(main_stream);
    if (int rc = dist_step_begin(plan, "dist_lap5", (int)sizeof(T), ms)) return rc;

    const int64_t di = domain[0], dj = domain[1], dk = domain[2];
    // W / E: the ring takes a box EW columns wide off the interior kernel (whole cache lines; and the interior then starts
    // on a 16-byte boundary -- one column in, it ran on 8-byte lanes at 85 us instead of 51 for the 128 x 256 x 512 share)
    int64_t EW = plan_edge_columns(plan, 16);
    EW = EW < 1 ? 1 : (EW > 16 ? 16 : EW);
    if (EW > 1) EW -= EW % (int64_t)(16 / sizeof(T));  // whole 16-byte lanes: the interior kernel keeps its alignment
    if (EW < 1) EW = 1;
    if (di < 16 * EW) EW = di >= 64 ? (EW < 8 ? EW : 8) : 1;  // narrow local domains keep most of their columns in the interior
    // Where the plan and the layout allow it the unpack and the ring are ONE kernel of wave-sized units that read the receive
    // buffers themselves (lap5_edge.hip.h); the interior then keeps every column but the first / last one (masked 16-byte
    // lanes: lap5_launch_variant) instead of giving 8-16 columns to a ring of 64-byte pieces.
    bool edge_units = false;
    if (int rc = lap5_edge_units_qualify<T>(plan, domain, inp, out, sides, &edge_units)) return rc;
    if (edge_units) EW = 16 / (int64_t)sizeof(T);  // one 16-byte lane: what a column unit computes (lap5_edge.hip.h)
    const int64_t lo_i = (sides & 1) ? EW : 0, hi_i = (sides & 2) ? EW : 0;
    const int64_t lo_j = (sides & 4) ? 1 : 0, hi_j = (sides & 8) ? 1 : 0;
    const int outer[4] = {0, 0, 0, 0};
    const int inner[4] = {(int)(lo_i <= di ? lo_i : di), (int)(hi_i && di - hi_i >= lo_i ? hi_i : 0), (int)lo_j,
                          (int)(hi_j && dj - 1 >= lo_j ? 1 : 0)};
    if (int rc = lap5_ring_run<T, W>(domain, inp, out, variant, outer, outer, ms)) return rc;  // an empty ring validates only

    const bool direct = plan->transport == GT4MI_TRANSPORT_DIRECT;
    // default: the fastest on every share of 8 ranks measured (1 x 8, 2 x 4, 4 x 2) -- "swap" with RCCL,
    // "inline" when the pack kernel is the transfer (direct transport)
    return run_schedule(
        plan, plan_schedule(plan, direct ? GT4MI_SCHEDULE_INLINE : GT4MI_SCHEDULE_SWAP), ms,
        [&](hipStream_t st) { return halo_pack_first(plan, inp, st); },
        [&](hipStream_t st) {
            ScopedLaunchLds throttle(lds_for_workgroups_per_cu(plan_interior_wg_per_cu(plan, 0)));
            return lap5_on_box<T, W>(inp, out, lo_i, lo_j, di - lo_i - hi_i, dj - lo_j - hi_j, dk, variant, st);
        },
        [&](hipStream_t st, bool first_pack_done) {
            return halo_exchange_on(plan, inp, st, first_pack_done, /*skip_last_unpack=*/edge_units);
        },
        [&](hipStream_t st) -> int {
            if (!edge_units) return lap5_ring_run<T, W>(domain, inp, out, variant, outer, inner, st);
            bool done = false;  // ONE launch: the unpack rides along with the edge units
            if (int rc = lap5_edge_run<T, W>(plan, domain, inp, out, variant, sides, st, &done)) return rc;
            if (done) return GT4MI_OK;
            if (direct) plan->direct.broken = "the edge units of a fused step could not be launched";
            return fail(GT4MI_ERR_HIP, "dist_lap5: the edge units qualified before the exchange and no longer do");
        },
        // "inline" on the direct transport, where the pack kernel is the transfer: with edge units ONE launch is the whole step
        // (push | interior | copies and edge units: lap5_step_kernel); else the push rides in the interior's launch
        // (lap5_push.hip.h: 8-9 us off the step)
        [&](hipStream_t st, FusedLaunch* fused) -> int {
            const int p0 = first_phase(plan);
            if (!direct || p0 > 1) return GT4MI_OK;
            bool launched = false;
            const int rc = direct_first_push(plan, /*whole_exchange=*/edge_units, &launched, [&](bool* done) {
                if (edge_units) return lap5_step_run<T, W>(plan, domain, inp, out, variant, sides, st, done);
                const gt4mi_field a = shifted(*inp, lo_i, lo_j), b = shifted(*out, lo_i, lo_j);
                const int64_t sub[3] = {di - lo_i - hi_i, dj - lo_j - hi_j, dk};
                return lap5_interior_with_push<T, W>(plan, sub, &a, &b, variant, inp, p0, st, done);
            });
            if (launched) *fused = edge_units ? FUSED_WHOLE_STEP : FUSED_PACK_AND_INTERIOR;
            return rc;
        });
}

// ---- the two time steppers: several stencil steps per exchange ------------------------------------------------------------------

// Join the exchange that delivered the input's ghost cells (started by the previous cycle, or by gt4mi_halo_exchange_begin).
inline int join_primed_exchange(gt4mi_halo_plan* plan, hipStream_t ms) {
    if (!(plan->probed && plan->probed_main == ms)) {
        // the probe synchronises: keep the exchange in flight ordered before it
        if (int rc = wait_done(plan, ms)) return rc;
        if (int rc = ensure_concurrent_stream(plan, ms)) return rc;
        if (int rc = mark_done(plan)) return rc;
    }
    return wait_done(plan, ms);
}

// gt4mi_dist_lap5_f64_wide: step `phase` of a cycle of `halo` steps on ghost cells `halo` deep, one exchange per cycle.
inline int dist_lap5_wide(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* inp, const gt4mi_field* out, int variant,
                          int sides, int halo, int phase, void* main_stream) {
    if (plan == nullptr || inp == nullptr || out == nullptr || domain == nullptr)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "dist_lap5_wide: null argument");
    if (halo < 1 || phase < 0 || phase >= halo)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "dist_lap5_wide: need halo >= 1 and 0 <= phase < halo");
    if (!plan->primed)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "dist_lap5_wide: the ghost cells of the first input were never exchanged "
                                                "(call gt4mi_halo_exchange_begin on it once before the first step)");
    hipStream_t ms = static_cast<hipStream_t>(main_stream);
    const int64_t di = domain[0], dj = domain[1], dk = domain[2], H = halo;
    const bool w = sides & 1, e = sides & 2, s = sides & 4, n = sides & 8;
    if ((w || e) && di < 2 * H) return fail(GT4MI_ERR_UNSUPPORTED, "dist_lap5_wide: local I extent smaller than 2*halo");
    if ((s || n) && dj < 2 * H) return fail(GT4MI_ERR_UNSUPPORTED, "dist_lap5_wide: local J extent smaller than 2*halo");
    // region [i0, i1) x [j0, j1) relative to the local compute-domain origin
    auto run = [&](int64_t i0, int64_t i1, int64_t j0, int64_t j1) {
        return lap5_on_box<double, double>(inp, out, i0, j0, i1 - i0, j1 - j0, dk, variant, ms);
    };
    if (phase == 0)  // (the exchange started `halo` steps ago)
        if (int rc = join_primed_exchange(plan, ms)) return rc;
    const int64_t ext = H - 1 - phase;  // how far this step still reaches into the ghost region
    if (ext > 0) {
        // redundant-compute step: one launch over the domain grown by `ext` towards every neighbour;
        // its ghost results are valid inputs for the next step, no communication
        return run(w ? -ext : 0, di + (e ? ext : 0), s ? -ext : 0, dj + (n ? ext : 0));
    }
    // last step of the cycle: `out`'s faces (H deep) are what the neighbours need next
    const int64_t lo_i = w ? H : 0, hi_i = e ? H : 0, lo_j = s ? H : 0, hi_j = n ? H : 0;
    {  // the H-deep ring of `out` in ONE launch (lap5_ring.hip.h)
        const int outer[4] = {0, 0, 0, 0};
        const int inner[4] = {(int)lo_i, (int)hi_i, (int)lo_j, (int)hi_j};
        if (int rc = lap5_ring_run<double, double>(domain, inp, out, variant, outer, inner, ms)) return rc;
    }
    // pack on the main stream (before the interior kernel floods the CUs), then fork
    if (int rc = halo_pack_first(plan, out, ms)) return rc;
    if (int rc = fork_side(plan, ms)) return rc;
    // interior on the main stream, RCCL send/recv + unpack of `out`'s ghost cells next to it; nobody
    // waits for them until phase 0 of the next cycle (where `out` is the input)
    if (int rc = run(lo_i, di - hi_i, lo_j, dj - hi_j)) return rc;
    if (int rc = halo_exchange_on(plan, out, plan->stream, /*first_pack_done=*/true)) return rc;
    return mark_done(plan);
}

// gt4mi_dist_lap5_f64_skewed: one cycle of `halo` steps between field_a and field_b, bands first, one exchange next to all interiors.
inline int dist_lap5_skewed(gt4mi_halo_plan* plan, const int64_t domain[3], const gt4mi_field* field_a, const gt4mi_field* field_b,
                            int variant, int sides, int halo, void* main_stream) {
    if (plan == nullptr || field_a == nullptr || field_b == nullptr || domain == nullptr)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "dist_lap5_skewed: null argument");
    if (halo < 1) return fail(GT4MI_ERR_INVALID_ARGUMENT, "dist_lap5_skewed: need halo >= 1");
    if (!plan->primed)
        return fail(GT4MI_ERR_INVALID_ARGUMENT, "dist_lap5_skewed: the ghost cells of the first input were never exchanged "
                                                "(call gt4mi_halo_exchange_begin on it once before the first cycle)");
    hipStream_t ms = static_cast<hipStream_t>(main_stream);
    const int64_t di = domain[0], dj = domain[1], dk = domain[2];
    const int H = halo;
    const bool w = sides & 1, e = sides & 2, s = sides & 4, n = sides & 8;
    // the band of step 1 reaches 2H - 1 points into the domain from every side that has a neighbour
    if ((w || e) && di < (int64_t)(2 * H - 1) * ((w ? 1 : 0) + (e ? 1 : 0)))
        return fail(GT4MI_ERR_UNSUPPORTED, "dist_lap5_skewed: local I extent too small for a ghost depth of %d", H);
    if ((s || n) && dj < (int64_t)(2 * H - 1) * ((s ? 1 : 0) + (n ? 1 : 0)))
        return fail(GT4MI_ERR_UNSUPPORTED, "dist_lap5_skewed: local J extent too small for a ghost depth of %d", H);
    if (int rc = join_primed_exchange(plan, ms)) return rc;
    auto src_of = [&](int step) { return (step % 2 == 1) ? field_a : field_b; };  // step 1 reads a, writes b
    auto dst_of = [&](int step) { return (step % 2 == 1) ? field_b : field_a; };
    // 1. the bands, outermost first: step st on [-(H - st), 2H - st) points from every side with a neighbour
    for (int st = 1; st <= H; ++st) {
        const int g = H - st, d = 2 * H - st;
        const int outer[4] = {w ? g : 0, e ? g : 0, s ? g : 0, n ? g : 0};
        const int inner[4] = {w ? d : 0, e ? d : 0, s ? d : 0, n ? d : 0};
        if (int rc = lap5_ring_run<double, double>(domain, src_of(st), dst_of(st), variant, outer, inner, ms)) return rc;
    }
    // 2. the H-deep faces of the result are final: pack them on the main stream (before the interior kernels flood the
    //    device), then the side stream sends / receives / unpacks next to ALL H interior kernels
    const gt4mi_field* result = dst_of(H);
    // (chain schedule: the pack runs on the side stream as well, next to the first interior kernel)
    const bool pack_on_side = plan_schedule(plan, GT4MI_SCHEDULE_JOIN) == GT4MI_SCHEDULE_CHAIN;
    if (!pack_on_side)
        if (int rc = halo_pack_first(plan, result, ms)) return rc;
    if (int rc = fork_side(plan, ms)) return rc;
    // 3. the interiors: step st on the domain shrunk by 2H - st
    for (int st = 1; st <= H; ++st) {
        const int64_t d = 2 * H - st;
        const int64_t i0 = w ? d : 0, i1 = di - (e ? d : 0), j0 = s ? d : 0, j1 = dj - (n ? d : 0);
        {
            ScopedLaunchLds throttle(lds_for_workgroups_per_cu(plan_interior_wg_per_cu(plan, 0)));
            if (int rc = lap5_on_box<double, double>(src_of(st), dst_of(st), i0, j0, i1 - i0, j1 - j0, dk, variant, ms)) return rc;
        }
        if (st == 1) {  // enqueued after the first interior launch so that the device has work while the host talks to RCCL
            if (int rc = halo_exchange_on(plan, result, plan->stream, /*first_pack_done=*/!pack_on_side)) return rc;
            if (int rc = mark_done(plan)) return rc;
        }
    }
    return GT4MI_OK;
}

}  // namespace gt4mi
