"""``gt4py_amd.linescan`` on the GPU: against the contract's restatement (tests/line_scan_ref.py) over EVERY byte of every dst
buffer, compared as integers -- row padding, ghost cells outside the box and the allocation's slack keep a NaN-payload sentinel (or,
in place, the source); inside the box a NaN that an addition made (inf + -inf) counts as a NaN, the NaNs that max and min MOVE are
compared bit for bit in the test that plants them.  Every input must come back unchanged.

The extents cross every boundary of the three kernels: line lengths around the look-ahead of 4 steps (1 .. 5), below, at and above
one 128-byte tile run for both dtypes (16 float64 / 32 float32 items) and several runs with a tail (130); 1, 63, 64, 65 and 257
lines along the lane axis, i.e. one live lane, a partial wave, a full one, a wave plus one and several workgroups; a box that is
ONE line.  Every length has a line count of its own, so that the product stays small."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import device_layouts as L  # noqa: E402  (the layouts; test infrastructure)
import line_scan_ref as R  # noqa: E402
from oracle import ref_numpy as ORACLE  # noqa: E402  (oracle = checker only)

LANES, TILES, ITEMS = "lanes", "tiles", "items"
#: (line length, the extents of the two other axes)
EXTENTS = [(1, (64, 1)), (2, (63, 1)), (3, (257, 1)), (4, (65, 2)), (5, (5, 3)), (15, (5, 3)), (16, (65, 2)), (17, (5, 3)), (31, (3, 2)),
           (32, (64, 1)), (33, (65, 2)), (130, (3, 2)), (17, (1, 1)), (130, (1, 1))]  # (the last two: a box that is ONE line)
AXES = "IJK"
FLAG_SETS = [(False, False), (True, False), (False, True), (True, True)]  # (exclusive, reverse)


def _shape(n, others, axis):
    shape = list(others)
    shape.insert(axis, n)
    return tuple(shape)


def expected_path(strides, weight_strides, extent, axis):
    """The rule of include/gt4py_amd.h restated: strides in ITEMS of every field, of the weight (None: no weight or a 1-d one,
    which is unit along the line and broadcast elsewhere)."""
    def unit(ax):
        return all(s[ax] == 1 for s in strides) and (weight_strides is None or weight_strides[ax] == 1)

    if unit(axis) and extent[axis] > 1:
        return TILES
    return LANES if any(unit(ax) and extent[ax] > 1 for ax in range(3) if ax != axis) else ITEMS


def _values(rng, shape, dtype, f=0):
    """Mixed signs and magnitudes (almost every addition rounds), a few zeros of both signs."""
    v = (rng.uniform(-1, 1, shape) * 10.0 ** rng.integers(-2, 3, shape) * 10.0 ** (f % 3)).astype(dtype)
    v[rng.uniform(0, 1, shape) < 0.02] = dtype(-0.0)
    v[rng.uniform(0, 1, shape) < 0.02] = dtype(0.0)
    return v


def _run(extent, axis, op="sum", exclusive=False, reverse=False, *, dtype=np.float64, layout="ifirst", src_layout=None, nfields=1,
         inplace=False, weight=None, wide=False, halo=0, k0=0, seed=0, plant=None, want_path=None, data=None):
    """One call through ``linescan.LineScan``; every dst buffer is compared whole against the restatement, every input must come
    back unchanged.  ``extent`` is the box that is scanned (the halo included).  ``weight``: None, ``"ijk"``, ``"line"`` (1-d; or the
    1-d array itself) or ``"expanded"`` (the IJK field that holds the 1-d weight of ``"line"`` on every line).  ``data``: the boxes of the sources
    (default: seeded).  Returns the boxes as the device left them, and the LineScan."""
    from gt4py_amd import linescan

    rng = np.random.default_rng([seed, *extent, axis])
    wrng = np.random.default_rng([seed, *extent, axis, 1])  # (the weight does not depend on how many fields there are)
    # one ghost cell in front of the box on the low sides of I and J, one behind the array the product sees, k0 levels below
    shape = (extent[0] + 2, extent[1] + 2, extent[2] + k0)
    box = (slice(1, 1 + extent[0]), slice(1, 1 + extent[1]), slice(k0, None))
    origin = (1 + halo, 1 + halo, k0)
    n = extent[axis]
    xs = [_values(rng, shape, dtype, f) for f in range(nfields)]
    if data is not None:
        for x, d in zip(xs, data):
            x[box] = d
    if plant is not None:
        plant([x[box] for x in xs])
    d_weight = w_box = None
    given = isinstance(weight, np.ndarray)
    if given or weight in ("line", "expanded"):
        w_line = weight if given else wrng.uniform(0.5, 2, n).astype(dtype)
        w_box = w_line
        if given or weight == "line":
            d_weight = L.Line(w_line)
        else:
            w_full = wrng.uniform(0.5, 2, shape).astype(dtype)
            w_full[box] = np.broadcast_to(np.moveaxis(w_line.reshape(-1, 1, 1), 0, axis), extent)
            d_weight = L.Dev(shape, dtype, layout, w_full, 1)
    elif weight == "ijk":
        w_full = _values(wrng, shape, dtype)
        d_weight, w_box = L.Dev(shape, dtype, layout, w_full, 1), w_full[box]
    src_layout = src_layout or layout
    if inplace:
        dsts = srcs = [L.Dev(shape, dtype, layout, x, 1) for x in xs]
    else:
        srcs = [L.Dev(shape, dtype, src_layout, x, 1) for x in xs]
        dsts = [L.Dev(shape, dtype, layout, None, 1) for _ in xs]
    sc = linescan.LineScan([d.given for d in dsts], [s.given for s in srcs], axis=AXES[axis], op=op, exclusive=exclusive, reverse=reverse,
                           weight=None if d_weight is None else d_weight.given, wide=wide, halo=halo, origin=origin)
    lines = extent[(axis + 1) % 3] * extent[(axis + 2) % 3]
    assert (sc.n, sc.lines, sc.extent, sc.launches) == (n, lines, tuple(extent), -(-nfields // 8))
    if want_path is None:
        strides = [d.lay.strides for d in dsts] + [s.lay.strides for s in srcs]
        want_path = expected_path(strides, d_weight.lay.strides if isinstance(d_weight, L.Dev) else None, extent, axis)
    assert sc.path == want_path, (sc.path, want_path)
    sc()
    what = (f"axis {AXES[axis]} extent {extent} {op} exclusive {exclusive} reverse {reverse} wide {wide} weight {'given' if given else weight} {np.dtype(dtype)} "
            f"{layout} {nfields} field(s) inplace {inplace} {sc.path}")
    got = []
    for f, (d, x) in enumerate(zip(dsts, xs)):
        want = R.scan_along(x[box], axis, op, exclusive, reverse, w_box, wide)
        got.append(d.assert_box(box, want, f"{what}: dst {f}"))
    if not inplace:
        for f, s in enumerate(srcs):
            s.assert_unchanged(f"{what}: src {f}")
    if d_weight is not None:
        d_weight.assert_unchanged(f"{what}: weight")
    return got, sc


@pytest.mark.parametrize("layout", ["ifirst", "kfirst"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_extents_at_look_ahead_tile_wave_and_workgroup_boundaries(axis, layout):
    for k, (n, others) in enumerate(EXTENTS):
        for dtype in (np.float32, np.float64):
            _run(_shape(n, others, axis), axis, "sum", *FLAG_SETS[k % 4], dtype=dtype, layout=layout, seed=1)
            _run(_shape(n, others, axis), axis, ("max", "min")[k % 2], *FLAG_SETS[(k // 2 + 1) % 4], dtype=dtype, layout=layout, seed=1)


@pytest.mark.parametrize("layout", ["ifirst", "kfirst"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_every_op_exclusive_and_reverse_in_place_and_out_of_place(axis, layout):
    extent = _shape(33, (65, 2), axis)
    for op in R.OPS:
        for exclusive, reverse in FLAG_SETS:
            out, _ = _run(extent, axis, op, exclusive, reverse, dtype=np.float32, layout=layout, nfields=2, seed=2)
            inp, _ = _run(extent, axis, op, exclusive, reverse, dtype=np.float32, layout=layout, nfields=2, inplace=True, seed=2)
            for x, y in zip(out, inp):
                assert R.same_bits(x, y).all(), (op, exclusive, reverse)
    _run(_shape(130, (3, 2), axis), axis, "min", True, True, dtype=np.float64, layout=layout, nfields=2, inplace=True, seed=2)


@pytest.mark.parametrize("layout", ["ifirst", "kfirst"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_an_ijk_weight_and_a_1d_weight_that_is_broadcast_without_a_copy(axis, layout):
    extent = _shape(33, (65, 2), axis)
    for dtype in (np.float32, np.float64):
        for exclusive, reverse in ((False, False), (True, True)):
            _run(extent, axis, "sum", exclusive, reverse, dtype=dtype, layout=layout, nfields=2, weight="ijk", seed=3)
            line, sc = _run(extent, axis, "sum", exclusive, reverse, dtype=dtype, layout=layout, nfields=2, weight="line", seed=3)
            assert sc.path == (TILES if L.geometry((2, 2, 2), layout, 8, 0)[1][axis] == 1 else LANES)  # a 1-d weight keeps the fields' path
            full, _ = _run(extent, axis, "sum", exclusive, reverse, dtype=dtype, layout=layout, nfields=2, weight="expanded", seed=3)
            for x, y in zip(line, full):
                assert R.same_bits(x, y).all(), (dtype, exclusive, reverse)
    _run(extent, axis, "sum", False, True, dtype=np.float32, layout=layout, inplace=True, weight="line", wide=True, seed=3)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_wide_accumulates_float32_in_float64_and_rounds_once(axis):
    """4096 items of 1 + 2 ** -20: float32 loses every small term, the wide sum keeps them until the store."""
    extent = _shape(4096, (3, 2), axis)
    ones = [np.full(extent, 1.0 + 2.0 ** -20, dtype=np.float32)]
    for layout in ("ifirst", "kfirst"):
        narrow, _ = _run(extent, axis, "sum", dtype=np.float32, layout=layout, data=ones, seed=4)
        wide, _ = _run(extent, axis, "sum", dtype=np.float32, layout=layout, data=ones, wide=True, seed=4)
        last = [slice(None)] * 3
        last[axis] = -1
        assert (wide[0][tuple(last)] == np.float32(4096 * (1.0 + 2.0 ** -20))).all() and (narrow[0][tuple(last)] != wide[0][tuple(last)]).all()
    for layout in ("ifirst", "kfirst"):
        for weight in (None, "ijk"):
            _run(_shape(33, (65, 2), axis), axis, "sum", True, False, dtype=np.float32, layout=layout, nfields=3, weight=weight, wide=True, seed=4)
    # no effect on float64 fields, on max and on min
    for op, dtype in (("sum", np.float64), ("max", np.float32), ("min", np.float64)):
        a, _ = _run(_shape(17, (5, 3), axis), axis, op, dtype=dtype, wide=True, seed=4)
        b, _ = _run(_shape(17, (5, 3), axis), axis, op, dtype=dtype, wide=False, seed=4)
        assert R.same_bits(a[0], b[0]).all()


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_one_to_nine_pairs_and_float64_with_8_entries_on_each_path(axis):
    """9 pairs are two launches; a field has the same bits at every position and in every company."""
    extent = _shape(17, (5, 3), axis)
    for op, inplace in (("sum", False), ("max", True)):
        nine, sc = _run(extent, axis, op, dtype=np.float32, nfields=9, inplace=inplace, weight="ijk" if op == "sum" else None, seed=5)
        assert sc.launches == 2
        for count in (8, 5, 4, 2, 1):
            some, _ = _run(extent, axis, op, dtype=np.float32, nfields=count, inplace=inplace, weight="ijk" if op == "sum" else None, seed=5)
            for f in range(count):
                assert R.same_bits(some[f], nine[f]).all(), (op, count, f)
    big = _shape(33, (65, 2), axis)
    # float64 with all 8 entries (the largest register budgets) on each path: ifirst and kfirst between them reach LANES and TILES
    for layout in ("ifirst", "kfirst"):
        _run(big, axis, "sum", True, True, dtype=np.float64, layout=layout, nfields=8, weight="ijk", seed=5)
        _run(big, axis, "min", dtype=np.float64, layout=layout, nfields=9, inplace=True, seed=5)
    _run(big, axis, "sum", False, True, dtype=np.float64, layout="ifirst", src_layout="kfirst", nfields=8, weight="line", seed=5, want_path=ITEMS)
    _run(big, axis, "sum", dtype=np.float32, layout="ifirst", src_layout="kfirst", nfields=8, wide=True, seed=5, want_path=ITEMS)
    _run(extent, axis, "max", True, False, dtype=np.float32, layout="kfirst", src_layout="jfirst", nfields=4, seed=5, want_path=ITEMS)


@pytest.mark.parametrize("layout", ["jfirst", "ifirst_unaligned"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_halo_and_an_origin_off_zero(axis, layout):
    _run(_shape(17, (9, 7), axis), axis, "sum", True, True, dtype=np.float64, layout=layout, nfields=2, weight="ijk", halo=2, k0=1, seed=6)
    _run(_shape(17, (9, 7), axis), axis, "max", dtype=np.float32, layout=layout, nfields=2, inplace=True, halo=2, k0=1, seed=6)


def test_each_kernel_is_reached_by_the_layout_it_is_for():
    """The storage preset (padded rows, I contiguous), a C-ordered torch tensor, and a call whose fields disagree."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import linescan

    rng = np.random.default_rng(7)
    shape = (33, 9, 4)
    x, w = _values(rng, shape, np.float64), rng.uniform(0.5, 2, shape)
    preset = [gt_storage.from_array(v, backend="hip:mi300") for v in (x, w, np.zeros(shape))]
    assert preset[0].strides[0] == 8 and preset[0].strides[1] > 8 * shape[0]  # I contiguous, rows padded
    c_order = [torch.from_numpy(v).cuda() for v in (x, w, np.zeros(shape))]
    for fields, paths in ((preset, (TILES, LANES, LANES)), (c_order, (LANES, LANES, TILES))):
        for axis, path in enumerate(paths):
            sc = linescan.LineScan(fields[2], fields[0], axis=AXES[axis], weight=fields[1], reverse=True)
            assert sc.path == path
            sc()
            got = fields[2].get() if hasattr(fields[2], "get") else fields[2].cpu().numpy()
            assert R.same_bits(got, R.scan_along(x, axis, "sum", reverse=True, weight=w)).all(), (axis, path)
    for axis in range(3):
        _run(_shape(33, (65, 2), axis), axis, "sum", layout="ifirst", src_layout="kfirst", nfields=2, seed=7, want_path=ITEMS)
        _run(_shape(33, (65, 2), axis), axis, "min", True, True, layout="kfirst", src_layout="ifirst", nfields=2, seed=7, want_path=ITEMS)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_same_lines_through_every_path_and_axis_give_the_same_bits(dtype):
    rng = np.random.default_rng(8)
    lines = _values(rng, (33, 65, 2), dtype)  # the line axis first
    for op, weight in (("sum", rng.uniform(0.5, 2, 33).astype(dtype)), ("max", None)):
        seen, paths = [], set()
        for axis in range(3):
            extent = _shape(33, (65, 2), axis)
            data = [np.ascontiguousarray(np.moveaxis(lines, 0, axis))]
            for layout, src_layout in (("ifirst", None), ("kfirst", None), ("jfirst", None), ("ifirst", "kfirst")):
                got, sc = _run(extent, axis, op, False, True, dtype=dtype, layout=layout, src_layout=src_layout, weight=weight, data=data, seed=8,
                               want_path=ITEMS if src_layout else None)
                paths.add((axis, sc.path))
                seen.append(np.moveaxis(got[0], axis, 0))
        assert paths == {(axis, path) for axis in range(3) for path in (LANES, TILES, ITEMS)}
        for other in seen[1:]:
            assert R.same_bits(seen[0], other).all(), op


@pytest.mark.parametrize("layout", ["ifirst", "kfirst"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_nan_and_an_inf_reach_the_rest_of_their_line_and_no_other(axis, layout):
    extent = _shape(33, (65, 2), axis)
    payload = np.array([0x7FC0_1234], dtype=np.uint32).view(np.float32)[0]
    spots = []  # (point on the line, the line's two other indices, what is planted)
    for m, p, r, v in ((20, 64, 0, payload), (5, 3, 1, np.float32(np.inf))):
        point = [p, r]
        point.insert(axis, m)
        spots.append((tuple(point), v))

    def plant(boxes):
        for point, v in spots:
            boxes[0][point] = v

    for op in R.OPS:
        for reverse in (False, True):
            clean, _ = _run(extent, axis, op, False, reverse, dtype=np.float32, layout=layout, nfields=2, seed=9)
            dirty, _ = _run(extent, axis, op, False, reverse, dtype=np.float32, layout=layout, nfields=2, seed=9, plant=plant)
            touched = np.zeros(extent, dtype=bool)
            for point, _v in spots:
                line = list(point)
                line[axis] = slice(None)
                touched[tuple(line)] = True
            assert R.same_bits(clean[0][~touched], dirty[0][~touched]).all() and np.isfinite(dirty[0][~touched]).all()
            assert R.same_bits(clean[1], dirty[1]).all()  # the other field of the launch
            (nan_point, _), (inf_point, _) = spots
            # the NaN: from its point to the end of the scan, nowhere in front of it
            nan_line = np.moveaxis(dirty[0], axis, 0)[(slice(None),) + tuple(c for a, c in enumerate(nan_point) if a != axis)]
            m = nan_point[axis]
            after, before = (nan_line[:m + 1], nan_line[m + 1:]) if reverse else (nan_line[m:], nan_line[:m])
            assert np.isnan(after).all() and np.isfinite(before).all(), (op, reverse)
            if op != "sum":  # max and min MOVE the NaN: its payload arrives
                assert (R.bits(after) == 0x7FC0_1234).all(), (op, reverse)
            inf_line = np.moveaxis(dirty[0], axis, 0)[(slice(None),) + tuple(c for a, c in enumerate(inf_point) if a != axis)]
            m = inf_point[axis]
            after, before = (inf_line[:m + 1], inf_line[m + 1:]) if reverse else (inf_line[m:], inf_line[:m])
            assert np.isfinite(before).all()
            if op != "min":
                assert (after == np.inf).all(), (op, reverse)
            else:
                assert np.isfinite(after).all()  # (+inf is the minimum of nothing but itself, and the line does not start with it)


def test_hand_over_from_and_to_stencils_in_stream_order():
    """A device_sync=False stencil writes src, LineScan integrates it along I, a device_sync=False stencil reads dst; nothing in
    between.  Compared with the oracle route on the host."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import linescan
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates

    backend, (ni, nj, nk) = "hip:mi300", (96, 40, 6)
    rng = np.random.default_rng(10)
    shape = (ni + 2, nj + 2, nk)
    u, ring, dx = rng.uniform(-1, 1, shape), rng.uniform(-1, 1, shape), rng.uniform(0.5, 2, shape[0])
    lap = gtscript.stencil(backend=backend, definition=hip_templates.lap_notebook, dtypes={"T": np.float64}, device_sync=False)
    d_u, d_src = (gt_storage.from_array(v, backend=backend, aligned_index=(1, 1, 0)) for v in (u, ring))
    d_dx = torch.from_numpy(dx).cuda()
    d_int, d_out = (gt_storage.zeros(shape, backend=backend, aligned_index=(1, 1, 0)) for _ in range(2))
    # the box is the domain and its ghost ring; the stencil in front writes the domain of src, the ring keeps what it was given
    scan = linescan.LineScan(d_int, d_src, axis="I", weight=d_dx, halo=1)
    assert scan.extent == shape and scan.origin == (1, 1, 0) and scan.path == TILES
    for _ in range(2):  # (the second round finds everything already written: the same result)
        lap(d_u, d_src, origin=(1, 1, 0), domain=(ni, nj, nk))
        scan()
        lap(d_int, d_out, origin=(1, 1, 0), domain=(ni, nj, nk))
    torch.cuda.synchronize()
    src = ring.copy()
    ORACLE.laplacian(u, src)
    integral = np.cumsum(src * dx[:, None, None], axis=0)  # today's route on the host: the contract's bits
    want = np.zeros(shape)
    ORACLE.laplacian(integral, want)
    assert np.array_equal(d_src.get().view(np.uint64), src.view(np.uint64))
    assert np.array_equal(d_int.get().view(np.uint64), integral.view(np.uint64))
    assert np.array_equal(d_int.get().view(np.uint64), R.scan_along(src, 0, weight=dx).view(np.uint64))
    assert np.array_equal(d_out.get().view(np.uint64), want.view(np.uint64))
