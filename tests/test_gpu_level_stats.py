"""``diagnostics.LevelStats`` on the GPU: all nine rows BIT FOR BIT against the numpy restatement of the documented order
(tests/level_stats_ref.py); the bits of a level a function of its plane alone -- whatever nk, the level, the layout, the
alignment, the position in the launch or the number of entries; counts, extremes and integer-valued sums against
``field_stats`` of each plane; special values; the profile handed to a stencil on the device; and the time loop.  The buffers hold
a NaN sentinel outside the domain: a read outside the box turns the result NaN."""

import functools
import gc
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_util as G  # noqa: E402
import level_stats_ref as R  # noqa: E402
from device_layouts import DOMAINS, LAYOUTS  # noqa: E402
from gt4py_amd.cartesian.gtscript import PARALLEL, Field, K, computation, interval  # noqa: E402, F401
from oracle import ref_numpy as ORACLE  # noqa: E402  (oracle = checker only)

DOMAINS = DOMAINS + [(128, 128, 64), (700, 5, 3)]
SEVERAL_ROWS_PER_WAVE = [(5, 1030, 3), (3, 771, 2)]


def _rows(frozen):
    """One call; the (n, 9, nk) result on the host, and the same through get()."""
    frozen()
    profiles = frozen.get()
    rows = frozen.result.get()
    assert rows.shape == (len(profiles), 9, frozen.nk)
    for block, p in zip(rows, profiles):
        assert R.same_bits(np.array([getattr(p, name) for name in ("count", "nonfinite", "sum", "sum_abs", "sum_sq", "min", "max",
                                                                  "dot", "mean")], dtype=np.float64), block)
    return rows


@functools.lru_cache(maxsize=None)
def _case(domain, dtype_name):
    """Data and the restatement's three profiles of a domain (a field, a pair, a pair with an IJ weight): computed once, shared,
    read-only."""
    dtype = np.dtype(dtype_name).type
    rng = np.random.default_rng([*domain, np.dtype(dtype_name).itemsize])
    a, b = G.data(rng, domain, dtype), G.data(rng, domain, dtype)
    w = rng.uniform(0.5, 2.0, domain[:2] + (1,)).astype(dtype)
    want = [R.profile(a), R.profile(a, b), R.profile(a, w)]
    for x in (a, b, w, *want):
        x.setflags(write=False)
    return a, b, w, want


def _three_entries(domain, dtype, layout, halo):
    """A LevelStats of three entries in one launch over fresh device copies of the case's data; also what keeps them alive."""
    from gt4py_amd import diagnostics

    a, b, w, _ = _case(domain, np.dtype(dtype).name)
    devs = [G.device(x, layout, halo) for x in (a, b, w)]
    arrays = [G.wrap(d) for d in devs]
    weight = arrays[2][:, :, 0] if domain[2] > 1 else arrays[2]  # Field[IJ] against Field[IJK]
    frozen = diagnostics.LevelStats([arrays[0]] * 3, others=[None, arrays[1], weight], halo=halo)
    return frozen, devs, (arrays, weight)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("halo", [0, 2])
def test_every_row_bit_for_bit_against_the_restatement(dtype, halo):
    """One field, a pair, and a pair whose second field is an IJ weight (K stride 0), in one launch of three entries; the
    whole buffers are bit-unchanged afterwards."""
    import torch

    for domain in DOMAINS:
        want = _case(domain, np.dtype(dtype).name)[3]
        for layout in LAYOUTS:
            frozen, devs, keep = _three_entries(domain, dtype, layout, halo)
            before = [G.bits(d._flat).clone() for d in devs]
            assert frozen.domain == domain and frozen.launches == 2 and frozen.nk == domain[2]
            assert frozen._workspace_bytes == 3 * domain[2] * R.geometry(*domain[:2])[1] * 64
            got = _rows(frozen)
            for n, what in enumerate(("field", "pair", "weight")):
                assert R.same_bits(got[n], want[n]), f"{domain} {dtype.__name__} {layout} halo {halo} {what}:\n{got[n]}\n!=\n{want[n]}"
            torch.cuda.synchronize()
            assert all(torch.equal(G.bits(d._flat), x) for d, x in zip(devs, before)), "a field buffer changed"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("halo", [0, 2])
def test_every_row_bit_for_bit_with_several_rows_per_wave(dtype, halo):
    """The order beyond one row per wave -- a lane's chain over its wave's rows, a last tile whose waves have fewer rows or
    none, an odd value carried up the halving -- on data whose sums depend on that order.  The geometry is asserted from the
    restatement: a change of the constant must not move these cases back to one row per wave."""
    for domain in SEVERAL_ROWS_PER_WAVE:
        rw, tiles, chunks = R.geometry(*domain[:2])
        assert rw > 1 and any(n % 2 for n in R.halvings(tiles)[:-1]), (domain, rw, tiles)
        last = [min(max(domain[1] - (4 * (tiles - 1) + w) * rw, 0), rw) for w in range(4)]
        assert last[0] > 0 and min(last) < rw, (domain, last)  # a short last tile
        want = _case(domain, np.dtype(dtype).name)[3]
        assert len({x.tobytes() for x in want}) == 3
        for layout in ("ifirst", "kfirst"):
            frozen, devs, keep = _three_entries(domain, dtype, layout, halo)
            assert frozen._workspace_bytes == 3 * domain[2] * tiles * 64  # the library derived the same partition
            got = _rows(frozen)
            for n, what in enumerate(("field", "pair", "weight")):
                assert R.same_bits(got[n], want[n]), f"{domain} {dtype.__name__} {layout} halo {halo} {what}:\n{got[n]}\n!=\n{want[n]}"
    if R.MAX_TILES == 32:
        assert R.geometry(5, 1030)[:2] == (9, 29) and R.halvings(29)[:3] == [29, 15, 8]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_bits_of_a_level_depend_on_its_plane_alone(dtype):
    """Without the restatement: the same plane (of a pair) gives the same nine values as level 0 of nk = 1, as level 3 of 7, as
    an IJ field, in all four layouts, at two alignments of the origin column, as entry 1, 5 or 8 of a full launch, as entry 9
    of nine (two launches), and twice in a row."""
    from gt4py_amd import diagnostics

    rng = np.random.default_rng(7)
    halo = 2
    for plane in [(65, 63), (300, 37), (5, 1030)]:
        a, b = G.data(rng, plane + (1,), dtype), G.data(rng, plane + (1,), dtype)
        box_a, box_b = G.data(rng, plane + (7,), dtype), G.data(rng, plane + (7,), dtype)
        box_a[:, :, 3:4], box_b[:, :, 3:4] = a, b
        fillers = [G.wrap(G.device(G.data(rng, plane + (1,), dtype), "ifirst", halo)) for _ in range(8)]
        deep_fillers = [G.wrap(G.device(G.data(rng, plane + (7,), dtype), "ifirst", halo)) for _ in range(8)]
        seen = {}

        def run(tag, fields, others, entry, level=0, **kwargs):
            frozen = diagnostics.LevelStats(fields, others=others, **kwargs)
            assert frozen.launches == (len(fields) + 7) // 8 + 1
            first, second = _rows(frozen)[entry, :, level].copy(), _rows(frozen)[entry, :, level].copy()
            assert not np.isnan(first).any(), (tag, first)
            assert first.tobytes() == second.tobytes(), f"{tag}: two calls differ"
            seen[tag] = first.tobytes()

        for layout in LAYOUTS:
            for align in (halo, halo + 1):  # the origin column on a 256-byte boundary / one item past it (no 16-byte lanes)
                da, db = G.wrap(G.device(a, layout, halo, align)), G.wrap(G.device(b, layout, halo, align))
                run((layout, align, "nk = 1"), [da], [db], 0, halo=halo)
                deep_a, deep_b = G.wrap(G.device(box_a, layout, halo, align)), G.wrap(G.device(box_b, layout, halo, align))
                run((layout, align, "level 3 of 7"), [deep_a], [deep_b], 0, level=3, halo=halo)
                flat_a, flat_b = da[:, :, 0], db[:, :, 0]
                assert flat_a.ndim == 2
                run((layout, align, "IJ"), [flat_a], [flat_b], 0, halo=halo)
                if layout == "ifirst" or align == halo:
                    for position in (0, 4, 7):
                        fields, others = list(fillers), [None] * 8
                        fields[position], others[position] = da, db
                        run((layout, align, position), fields, others, position, halo=halo)
                    run((layout, align, "ninth"), deep_fillers + [deep_a], [None] * 8 + [deep_b], 8, level=3, halo=halo)
        # levels 2 ... 4 of the deep box through origin[2] / domain[2]: profile index 1 is level 3
        deep_a, deep_b = G.wrap(G.device(box_a, "ifirst", halo)), G.wrap(G.device(box_b, "ifirst", halo))
        run("origin[2] = 2", [deep_a], [deep_b], 0, level=1, origin=(halo, halo, 2), domain=plane + (3,))
        assert len(set(seen.values())) == 1, f"{plane} {dtype.__name__}: {len(set(seen.values()))} different results: {sorted(map(str, seen))}"
        assert len(seen) == 8 * 3 + 5 * 4 + 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_against_field_stats_of_every_plane(dtype):
    """field_stats is verified on its own (tests/test_gpu_diagnostics.py).  Per level, COUNT, NONFINITE, MIN and MAX do not
    depend on the order and equal field_stats of that plane exactly.  On integer-valued data with |x| <= 2^20 (|a|, |b| <=
    2^19) every partial sum in any order is an integer below 2^53 (x * x <= 2^40, at most 5200 < 2^13 points a level), so every
    sum equals numpy's int64 per-level sum and field_stats of the plane exactly."""
    from gt4py_amd import diagnostics

    rng = np.random.default_rng(21)
    halo = 1
    for domain in [(65, 63, 7), (130, 40, 3)]:
        ni, nj, nk = domain
        for integers in (False, True):
            if integers:
                a, b = (rng.integers(-2 ** 19, 2 ** 19, domain, endpoint=True).astype(dtype) for _ in range(2))
            else:
                a, b = G.data(rng, domain, dtype), G.data(rng, domain, dtype)
                a[3, 4, 1], b[5, 6, 2] = np.inf, np.nan  # (non-finite counts, NaN extremes of one level)
            da, db = G.wrap(G.device(a, "ifirst", halo)), G.wrap(G.device(b, "ifirst", halo))
            single, pair = diagnostics.level_stats(da, da, other=[None, db], halo=halo)
            for k in range(nk):
                planes = diagnostics.field_stats(da, da, other=[None, db], origin=(halo, halo, k), domain=(ni, nj, 1))
                for p, s, what in ((single, planes[0], "field"), (pair, planes[1], "pair")):
                    got = p[k]
                    assert (got.count, got.nonfinite) == (s.count, s.nonfinite) == (ni * nj, got.nonfinite), (domain, k, what)
                    assert R.same_bits([got.min, got.max], [s.min, s.max]), (domain, k, what, got, s)
                    if integers:
                        assert got == s, (domain, k, what, got, s)
            if integers:
                a64, b64 = a.astype(np.int64), b.astype(np.int64)
                for p, x, dot in ((single, a64, np.zeros(nk)), (pair, a64 - b64, (a64 * b64).sum(axis=(0, 1)))):
                    want = [x.sum(axis=(0, 1)), np.abs(x).sum(axis=(0, 1)), (x * x).sum(axis=(0, 1)), x.min(axis=(0, 1)), x.max(axis=(0, 1)), dot]
                    assert max(int(np.abs(v).max()) for v in want) < 2 ** 53
                    got = [p.sum, p.sum_abs, p.sum_sq, p.min, p.max, p.dot]
                    assert all(np.array_equal(g, np.asarray(v, dtype=np.float64)) for g, v in zip(got, want)), (domain, got, want)
                    assert np.array_equal(p.mean, p.sum / (ni * nj)) and p.first_nonfinite is None
            else:
                assert single.nonfinite.tolist() == [1 if k == 1 else 0 for k in range(nk)] and single.first_nonfinite == 1
                assert pair.nonfinite.tolist() == [1 if k in (1, 2) else 0 for k in range(nk)] and math.isnan(pair.min[2])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_special_values(dtype):
    from gt4py_amd import diagnostics

    rng = np.random.default_rng(9)
    domain = (130, 40, 5)
    a = G.data(rng, domain, dtype)
    a[-1, -1, 3] = np.nan  # one NaN, the last point of level 3
    a[0, 0, 1], a[7, 9, 1] = np.inf, -np.inf  # level 1: both infinities
    a[:, :, 4] = 0.0
    a[::3, :, 4] = -0.0  # level 4: only zeros, of either sign
    a[:, :, 0] = (rng.integers(-7, 8, domain[:2]) * np.finfo(dtype).smallest_subnormal).astype(dtype)  # denormals are numbers
    dev = G.wrap(G.device(a, "ifirst", 1))
    p, = diagnostics.level_stats(dev, halo=1)
    want = R.profile(a)
    rows = np.array([getattr(p, name) for name in diagnostics.PROFILE_ROWS], dtype=np.float64)
    assert R.same_bits(rows, want), (rows, want)
    assert p.count.tolist() == [130 * 40] * 5 and p.nonfinite.tolist() == [0, 2, 0, 1, 0]
    assert p.first_nonfinite == 1 and p.all_finite.tolist() == [True, False, True, False, True]
    # only level 3 is NaN
    for name in ("sum", "sum_abs", "sum_sq", "min", "max", "mean"):
        assert np.isnan(getattr(p, name)).tolist() == [False, name in ("sum", "mean"), False, True, False], name
    assert math.isnan(p.max_abs[3]) and math.isnan(p[3].max_abs) and p.dot.tolist() == [0.0] * 5
    # +-Inf in level 1: non-finite there, inf - inf = NaN in the sum, not in the extremes
    assert (p.min[1], p.max[1], p.sum_abs[1], p.max_abs[1]) == (-math.inf, math.inf, math.inf, math.inf)
    # a level of -0 and +0 only
    assert (p.min[4], p.max[4], p.sum_abs[4]) == (0, 0, 0) and np.signbit(p.min[4]) and not np.signbit(p.max[4])
    assert p.nonfinite[0] == 0 and p.sum_abs[0] > 0 and p.max[0] == float(a[:, :, 0].max()) and abs(p.max[0]) < np.finfo(dtype).tiny
    a[-1, -1, 3] = 1.0
    q, = diagnostics.level_stats(G.wrap(G.device(a, "kfirst", 1)), halo=1)
    assert q.first_nonfinite == 1 and not np.isnan(q.min).any() and R.same_bits(q.sum, R.profile(a)[R.SUM])
    # all-(-0) and all-(+0) levels keep their sign in both extremes
    z = np.zeros((9, 5, 2), dtype)
    z[:, :, 1] = -0.0
    s, = diagnostics.level_stats(G.wrap(G.device(z, "ifirst", 0)))
    assert np.signbit(s.min).tolist() == [False, True] and np.signbit(s.max).tolist() == [False, True]


def anomaly(u: Field[np.float64], m: Field[K, np.float64], out: Field[np.float64]):
    with computation(PARALLEL), interval(...):
        out = u - m


def test_profile_feeds_a_stencil_in_the_same_stream_without_synchronisation():
    """watch() on a side stream, then out = u - m with m: Field[K] fed watch.profile("mean") in the same stream, nothing in
    between: out is bit-equal to u - mean[k] of the restatement."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import diagnostics
    from gt4py_amd.cartesian import gtscript

    backend, domain = "hip:mi300", (65, 63, 7)
    stencil = gtscript.stencil(backend=backend, definition=anomaly, device_sync=False)
    rng = np.random.default_rng(17)
    host = G.data(rng, domain, np.float64) + 3.0
    u = gt_storage.from_array(host, backend=backend)
    out = gt_storage.zeros(domain, backend=backend)
    watch = diagnostics.LevelStats([u])
    with pytest.raises(RuntimeError, match="not been called"):
        watch.get()
    mean = watch.profile("mean")
    assert mean.shape == (7,) and mean.dtype == np.float64 and mean.strides == (8,)
    assert mean.ptr == watch.result.ptr + 8 * 7 * 8 and watch.profile("max", 0).ptr == watch.result.ptr + 6 * 7 * 8
    with pytest.raises(ValueError, match="no profile"):
        watch.profile("median")
    with pytest.raises(IndexError):
        watch.profile("mean", 1)
    stencil(u, mean, out)  # (compiled and loaded before the timed order matters)
    torch.cuda.synchronize()
    out.tensor.fill_(float("nan"))
    watch.result.tensor.fill_(float("nan"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        watch()
        stencil(u, mean, out)
    p, = watch.get()  # synchronises the stream both went to
    want = R.profile(host)
    assert R.same_bits(p.mean, want[R.MEAN]) and R.same_bits(mean.get(), want[R.MEAN])
    assert R.same_bits(out.get(), host - want[R.MEAN][None, None, :])


def test_time_loop_with_level_stats_read_a_step_late():
    """HaloFill -> Laplacian -> swap for 20 steps, LevelStats of the new field after every step, read one step late (a
    device-side copy keeps it); against numpy.pad + the oracle's Laplacian + the restatement on the host, every row of every
    step.  Then a field dies and the frozen call refuses to run."""
    import gt4py_amd.storage as gt_storage
    from gt4py_amd import boundary, diagnostics
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates

    backend, domain, steps = "hip:mi300", (96, 64, 6), 20
    rng = np.random.default_rng(31)
    shape = (domain[0] + 2, domain[1] + 2, domain[2])
    u0 = np.zeros(shape)
    u0[1:-1, 1:-1] = rng.uniform(-1, 1, domain)
    lap = gtscript.stencil(backend=backend, definition=hip_templates.lap_notebook, dtypes={"T": np.float64}, device_sync=False)
    d_a, d_b = (gt_storage.from_array(u0, backend=backend, aligned_index=(1, 1, 0)) for _ in range(2))
    fills = {id(d): boundary.HaloFill([d], halo=1, mode="periodic") for d in (d_a, d_b)}
    watch = {id(d): diagnostics.LevelStats([d], halo=1) for d in (d_a, d_b)}
    src, dst = d_a, d_b
    snapshots, late = [], []
    for step in range(steps):
        fills[id(src)]()
        lap(src, dst, origin=(1, 1, 0), domain=domain)
        watch[id(dst)]()
        snapshots.append(watch[id(dst)].result.tensor.clone())
        if step > 0:
            late.append(snapshots[step - 1].cpu().numpy()[0])  # the result of step n - 1, read after step n was enqueued
        src, dst = dst, src
    late.append(watch[id(src)].get()[0])
    h_src, h_dst = u0.copy(), u0.copy()
    for step in range(steps):
        h_src[...] = np.pad(h_src[1:-1, 1:-1], ((1, 1), (1, 1), (0, 0)), mode="wrap")
        ORACLE.laplacian(h_src, h_dst)
        want = R.profile(h_dst[1:-1, 1:-1])
        got = late[step]
        if step == steps - 1:
            assert got.first_nonfinite is None and got.total().count == np.prod(domain)
            got = np.array([getattr(got, name) for name in diagnostics.PROFILE_ROWS], dtype=np.float64)
        assert R.same_bits(got, want), f"step {step}:\n{got}\n!=\n{want}"
        assert (got[R.COUNT] == domain[0] * domain[1]).all() and not got[R.NONFINITE].any()
        h_src, h_dst = h_dst, h_src
    dead = watch[id(d_b)]
    del d_b, src, dst, fills
    gc.collect()
    with pytest.raises(RuntimeError, match="no longer exists"):
        dead()
    watch[id(d_a)]()  # the other one still runs
