"""``gt4py_amd.diagnostics`` on the GPU: all eight slots BIT FOR BIT against the numpy restatement of the documented order
(tests/stats_ref.py), identical bits whatever the layout, alignment, position in the launch or number of entries, exact results
on integer-valued full-size fields, the derived error bound against ``math.fsum``, special values, and the time loop.  The
buffers hold a NaN sentinel outside the domain: a read outside the box turns the result NaN.

Wall time of this file on one MI355X: 23 s, 16 s of them the ten math.fsum passes over the two full-size fields."""

import gc
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_util as G  # noqa: E402
import stats_ref as R  # noqa: E402
from device_layouts import DOMAINS, LAYOUTS  # noqa: E402
from oracle import ref_numpy as ORACLE  # noqa: E402  (oracle = checker only)

DOMAINS = DOMAINS + [(128, 128, 64), (700, 5, 3)]  # (700 columns: more than the 256 a wave covers at once; all of them: one row per wave)
U = 2.0 ** -53


def _rows(frozen):
    frozen()
    frozen.get()
    return frozen.result.get()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("halo", [0, 2])
def test_every_slot_bit_for_bit_against_the_restatement(dtype, halo):
    """One field, a pair, and a pair whose second field is an IJ weight (K stride 0), in one launch of three entries; the
    whole buffers are bit-unchanged afterwards."""
    import torch

    from gt4py_amd import diagnostics

    rng = np.random.default_rng(40 + halo)
    for domain in DOMAINS:
        a, b = G.data(rng, domain, dtype), G.data(rng, domain, dtype)
        w = rng.uniform(0.5, 2.0, domain[:2] + (1,)).astype(dtype)
        want = [R.stats(a), R.stats(a, b), R.stats(a, w)]
        for layout in LAYOUTS:
            da, db, dw = (G.device(x, layout, halo) for x in (a, b, w))
            before = [G.bits(d._flat).clone() for d in (da, db, dw)]
            arrays = [G.wrap(da), G.wrap(db), G.wrap(dw)]
            weight = arrays[2][:, :, 0] if domain[2] > 1 else arrays[2]  # Field[IJ] against Field[IJK]
            frozen = diagnostics.FieldStats([arrays[0]] * 3, others=[None, arrays[1], weight], halo=halo)
            assert frozen.domain == domain and frozen.launches == 2
            got = _rows(frozen)
            for n, what in enumerate(("field", "pair", "weight")):
                assert R.same_bits(got[n], want[n]), f"{domain} {dtype.__name__} {layout} halo {halo} {what}: {got[n]} != {want[n]}"
            torch.cuda.synchronize()
            assert all(torch.equal(G.bits(d._flat), x) for d, x in zip((da, db, dw), before)), "a field buffer changed"


# domain -> (rows, rows per wave, tiles, tiles per finish leaf, finish leaves): 2 and 3 rows per wave, 17 and 22 tiles per leaf, an odd
# number of leaves on the way up (125; 126 -> 63), a last tile whose last waves have fewer rows than the others
SEVERAL_ROWS_PER_WAVE = {(5, 130, 130): (16900, 2, 2113, 17, 125), (3, 257, 129): (33153, 3, 2763, 22, 126)}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("halo", [0, 2])
def test_every_slot_bit_for_bit_with_several_rows_per_wave(dtype, halo):
    """The order of the additions beyond one row per wave -- a lane's chain over its wave's rows, leaves of more than 16 tiles,
    an odd leaf carried up the halving tree -- on data whose sums depend on that order; single field, pair, pair with an IJ
    weight.  The geometry is asserted: a change of the constants must not move these cases back to one row per wave."""
    from gt4py_amd import diagnostics

    rng = np.random.default_rng(50 + halo)
    for domain, geometry in SEVERAL_ROWS_PER_WAVE.items():
        rows, rw, tiles, _, per_leaf, leaves = R.geometry(domain)
        assert (rows, rw, tiles, per_leaf, leaves) == geometry and rw > 1, R.geometry(domain)
        a, b = G.data(rng, domain, dtype), G.data(rng, domain, dtype)
        w = rng.uniform(0.5, 2.0, domain[:2] + (1,)).astype(dtype)
        want = [R.stats(a), R.stats(a, b), R.stats(a, w)]
        assert len({x.tobytes() for x in want}) == 3
        for layout in ("ifirst", "kfirst"):
            arrays = [G.wrap(G.device(x, layout, halo)) for x in (a, b, w)]
            weight = arrays[2][:, :, 0]  # Field[IJ] against Field[IJK]; (the frozen call holds its arrays weakly: keep it)
            frozen = diagnostics.FieldStats([arrays[0]] * 3, others=[None, arrays[1], weight], halo=halo)
            assert frozen.domain == domain and frozen.launches == 2
            assert frozen._workspace_bytes == 3 * tiles * 64  # the library derived the same partition: 64 bytes per tile and entry
            got = _rows(frozen)
            for n, what in enumerate(("field", "pair", "weight")):
                assert R.same_bits(got[n], want[n]), f"{domain} {dtype.__name__} {layout} halo {halo} {what}: {got[n]} != {want[n]}"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_identical_bits_whatever_the_geometry(dtype):
    """Without the restatement: the same domain data gives the same bits in all four layouts, at two alignments of the origin
    column, alone or as entry 1, 5 or 8 of a full launch, as entry 9 of nine, from a plain torch tensor, and twice in a row."""
    import torch

    from gt4py_amd import diagnostics

    rng = np.random.default_rng(7)
    halo = 2
    for domain in [(65, 63, 7), (300, 37, 2), (128, 128, 64), (700, 5, 3)]:
        a, b = G.data(rng, domain, dtype), G.data(rng, domain, dtype)
        fillers = [G.wrap(G.device(G.data(rng, domain, dtype), "ifirst", halo)) for _ in range(8)]
        seen = {}

        def run(tag, fields, others, entry, **kwargs):
            frozen = diagnostics.FieldStats(fields, others=others, **kwargs)
            assert frozen.launches == (len(fields) + 7) // 8 + 1
            first, second = _rows(frozen)[entry].copy(), _rows(frozen)[entry].copy()
            assert not np.isnan(first).any(), (tag, first)
            assert first.tobytes() == second.tobytes(), f"{tag}: two calls differ"
            seen[tag] = first.tobytes()

        for layout in LAYOUTS:
            for align in (halo, halo + 1):  # the origin column on a 256-byte boundary / one item past it (no 16-byte lanes)
                da, db = G.wrap(G.device(a, layout, halo, align)), G.wrap(G.device(b, layout, halo, align))
                run((layout, align, "alone"), [da], [db], 0, halo=halo)
                if layout == "ifirst" or align == halo:
                    for position in (0, 4, 7):
                        fields, others = list(fillers), [None] * 8
                        fields[position], others[position] = da, db
                        run((layout, align, position), fields, others, position, halo=halo)
                    run((layout, align, "ninth"), fillers + [da], [None] * 8 + [db], 8, halo=halo)
        box = np.full((domain[0] + 3, domain[1] + 1, domain[2]), np.nan, dtype=dtype)
        box[3:, 1:] = a
        tb = torch.from_numpy(np.ascontiguousarray(np.pad(b, ((3, 0), (1, 0), (0, 0))))).cuda()
        run("torch", [torch.from_numpy(box).cuda()], [tb], 0, origin=(3, 1, 0), domain=domain)
        assert len(set(seen.values())) == 1, f"{domain} {dtype.__name__}: {sorted(k for k in seen)} gave {len(set(seen.values()))} different results"
        assert len(seen) == 8 + 5 * 4 + 1  # alone; three positions and the ninth for five of the buffers; torch


@pytest.mark.parametrize("shape, dtype", [((512, 512, 128), np.float64), ((1024, 1024, 80), np.float32)])
def test_integer_valued_full_size_fields_are_exact(shape, dtype):
    """Without the restatement: |x| <= 1000, every partial sum in any order is an integer below 2^53, so every slot equals
    numpy's int64 arithmetic exactly."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import diagnostics

    gen = torch.Generator(device="cuda").manual_seed(3)
    fields = []
    for _ in range(2):
        d = gt_storage.empty(tuple(s + 2 if ax < 2 else s for ax, s in enumerate(shape)), dtype, backend="hip:mi300", aligned_index=(1, 1, 0))
        d.tensor.fill_(float("nan"))
        d.tensor[1:-1, 1:-1].copy_(torch.randint(-1000, 1001, shape, generator=gen, device="cuda").to(d.tensor.dtype))
        fields.append(d)
    got = diagnostics.field_stats(fields[0], fields[0], other=[None, fields[1]], halo=1)
    a, b = (f.tensor[1:-1, 1:-1].cpu().numpy().astype(np.int64) for f in fields)
    for s, x, dot in ((got[0], a, 0), (got[1], a - b, int((a * b).sum()))):
        want = (x.size, 0, int(x.sum()), int(np.abs(x).sum()), int((x * x).sum()), int(x.min()), int(x.max()), dot)
        assert tuple(s) == tuple(float(v) for v in want), (tuple(s), want)


@pytest.mark.parametrize("shape, dtype, pair", [((512, 512, 128), np.float64, True), ((1024, 1024, 80), np.float32, False)])
def test_full_size_sums_are_within_the_derived_bound_of_fsum(shape, dtype, pair):
    """(depth + 3) u times the sum of the |terms|: `depth` additions plus the roundings of the difference and of the product."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import diagnostics

    gen = torch.Generator(device="cuda").manual_seed(4)
    fields = []
    for _ in range(2 if pair else 1):
        d = gt_storage.empty(shape, dtype, backend="hip:mi300")
        d.tensor.copy_(torch.randn(shape, generator=gen, device="cuda", dtype=d.tensor.dtype) * 3.0 + 0.25)
        fields.append(d)
    got, = diagnostics.field_stats(fields[0], other=fields[1] if pair else None)
    depth = R.depth(shape)
    assert depth ** 2 < 2 ** 53
    x, ax, sq, prod = R.terms(*(f.get() for f in fields))
    scale_x = math.fsum(ax.ravel())
    for name, value, exact, scale in (("sum", got.sum, math.fsum(x.ravel()), scale_x), ("sum_abs", got.sum_abs, scale_x, scale_x),
                                      ("sum_sq", got.sum_sq, None, None), ("dot", got.dot, None, None)):
        if name == "sum_sq":
            exact = scale = math.fsum(sq.ravel())
        if name == "dot":
            if prod is None:
                assert value == 0.0
                continue
            exact, scale = math.fsum(prod.ravel()), math.fsum(np.abs(prod).ravel())
        bound = (depth + 3) * U * scale
        print(f"{shape} {np.dtype(dtype).name} {name}: {value!r} against fsum {exact!r}: |error| {abs(value - exact):.3e}, bound {bound:.3e}")
        assert abs(value - exact) <= bound, name
    assert (got.count, got.nonfinite, got.min, got.max) == (x.size, 0, x.min(), x.max())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_special_values(dtype):
    from gt4py_amd import diagnostics

    rng = np.random.default_rng(9)
    domain = (130, 40, 3)  # 120 rows: 30 tiles
    tiny = np.finfo(dtype).tiny

    def both(a, b=None):
        fields = [G.wrap(G.device(x, "ifirst", 1)) for x in ((a,) if b is None else (a, b))]
        got = diagnostics.field_stats(fields[0], other=None if b is None else fields[1], halo=1)[0]
        want = R.stats(a, b)
        assert R.same_bits(tuple(got), want), (tuple(got), want)
        return got

    a = G.data(rng, domain, dtype)
    a[-1, -1, -1] = np.nan  # the last point of the last tile
    s = both(a)
    assert s.nonfinite == 1 and s.count == a.size and all(math.isnan(v) for v in (s.sum, s.sum_abs, s.sum_sq, s.min, s.max))
    assert math.isnan(s.max_abs) and not s.all_finite
    a[-1, -1, -1] = np.inf
    s = both(a)
    assert s.nonfinite == 1 and s.max == math.inf and s.sum == math.inf and math.isfinite(s.min)
    a[0, 0, 0] = -np.inf
    s = both(a)
    assert s.nonfinite == 2 and (s.min, s.max) == (-math.inf, math.inf) and math.isnan(s.sum) and s.sum_abs == math.inf
    s = both(a, a)  # inf - inf
    assert s.nonfinite == 2 and math.isnan(s.min) and math.isnan(s.max) and s.dot == math.inf
    # only zeros of either sign, wherever they are: min is -0, max is +0
    for positions in (slice(0, 1), slice(-1, None), slice(None, None, 3)):
        z = np.zeros(domain, dtype)
        z[positions] = -0.0
        s = both(z)
        assert (s.min, s.max, s.sum_abs) == (0, 0, 0) and math.copysign(1, s.min) == -1 and math.copysign(1, s.max) == 1
        s = both(-z)
        assert math.copysign(1, s.min) == -1 and math.copysign(1, s.max) == 1
    assert math.copysign(1, both(np.zeros(domain, dtype)).min) == 1 and math.copysign(1, both(-np.zeros(domain, dtype)).max) == -1
    # denormals are numbers
    d = (rng.integers(-7, 8, domain) * np.finfo(dtype).smallest_subnormal).astype(dtype)
    s = both(d)
    assert s.nonfinite == 0 and s.sum_abs > 0 and s.max == float(d.max()) and s.min == float(d.min()) and abs(s.max) < tiny
    s = both(d, (d * 0.5).astype(dtype))
    assert s.nonfinite == 0 and s.sum_abs > 0


def test_no_synchronisation_side_stream_and_late_read():
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import diagnostics

    rng = np.random.default_rng(12)
    host = rng.uniform(-1, 1, (200, 96, 16))
    d = gt_storage.from_array(host, backend="hip:mi300")
    watch = diagnostics.FieldStats([d])
    with pytest.raises(RuntimeError, match="not been called"):
        watch.get()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        watch()
    s, = watch.get()  # synchronises the stream the call went to
    want = R.stats(host)
    assert R.same_bits(tuple(s), want)
    # the result of step n, read after step n + 1 was enqueued: a device-side copy keeps it
    snapshots, wants = [], []
    for step in range(4):
        d.tensor.mul_(1.5)
        watch()
        snapshots.append(watch.result.tensor.clone())
        host = host * 1.5
        wants.append(R.stats(host))
        if step > 0:
            assert R.same_bits(snapshots[step - 1].cpu().numpy()[0], wants[step - 1]), step
    assert R.same_bits(watch.get()[0], wants[-1])


def test_frozen_stats_refuse_to_run_after_an_array_died():
    import gt4py_amd.storage as gt_storage
    from gt4py_amd import diagnostics

    a = gt_storage.zeros((12, 12, 4), backend="hip:mi300", aligned_index=(1, 1, 0))
    b = gt_storage.zeros((12, 12, 4), backend="hip:mi300", aligned_index=(1, 1, 0))
    watch = diagnostics.FieldStats([a], others=[b], halo=1)
    watch()
    assert watch.get()[0].count == 400
    del b
    gc.collect()
    with pytest.raises(RuntimeError, match="no longer exists"):
        watch()


def test_time_loop_with_periodic_fill_laplacian_and_stats_every_step():
    """HaloFill -> Laplacian -> swap for 20 steps, FieldStats of the new field after every step, read one step late; against
    numpy.pad + the oracle's Laplacian + the restatement on the host, every slot of every step; and the four quadrants of the
    domain joined with merge against the same join of the restatement's."""
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
    watch = {id(d): diagnostics.FieldStats([d], halo=1) for d in (d_a, d_b)}
    hi, hj = domain[0] // 2, domain[1] // 2
    quadrants = [((1 + qi * hi, 1 + qj * hj, 0), (hi, hj, domain[2])) for qj in (0, 1) for qi in (0, 1)]
    per_quadrant = {id(d): [diagnostics.FieldStats([d], origin=o, domain=dom) for o, dom in quadrants] for d in (d_a, d_b)}
    src, dst = d_a, d_b
    snapshots = []
    for _ in range(steps):
        fills[id(src)]()
        lap(src, dst, origin=(1, 1, 0), domain=domain)
        watch[id(dst)]()
        snap = [watch[id(dst)].result.tensor.clone()]
        for q in per_quadrant[id(dst)]:
            q()
            snap.append(q.result.tensor.clone())
        snapshots.append(snap)
        src, dst = dst, src
    got = [[t.cpu().numpy()[0] for t in snap] for snap in snapshots]
    h_src, h_dst = u0.copy(), u0.copy()
    for step in range(steps):
        h_src[...] = np.pad(h_src[1:-1, 1:-1], ((1, 1), (1, 1), (0, 0)), mode="wrap")
        ORACLE.laplacian(h_src, h_dst)
        inner = h_dst[1:-1, 1:-1]
        want = R.stats(inner)
        assert R.same_bits(got[step][0], want), f"step {step}: {got[step][0]} != {want}"
        assert got[step][0][R.COUNT] == np.prod(domain) and got[step][0][R.NONFINITE] == 0
        want_parts = [diagnostics.Stats.from_row(R.stats(inner[o[0] - 1: o[0] - 1 + dom[0], o[1] - 1: o[1] - 1 + dom[1]])) for o, dom in quadrants]
        got_parts = [diagnostics.Stats.from_row(row) for row in got[step][1:]]
        assert got_parts == want_parts, step
        merged = diagnostics.merge(got_parts)
        assert merged == diagnostics.merge(want_parts) and merged.count == np.prod(domain)
        assert (merged.min, merged.max) == (want[R.MIN], want[R.MAX])
        h_src, h_dst = h_dst, h_src
