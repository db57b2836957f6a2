"""``gt4py_amd.linefind`` on the GPU: against the contract's restatement (tests/line_find_ref.py) over EVERY byte of the result
buffer, compared as integers -- a NaN from ``missing`` or a NaN extremum counts as a NaN -- with a sentinel buffer in front of and
behind the result.  Every case goes through the C entry (the result inside the sentinel buffer) AND through ``linefind.LineFind``
(the result the object owns): the two blocks must hold the same bytes.  Every field and the coord must come back unchanged.

The extents cross every boundary of the three kernels, as in tests/test_gpu_line_scan.py: line lengths around the look-ahead of 4
steps (1 .. 5), below, at and above one 128-byte tile run for both dtypes (16 float64 / 32 float32 items) and several runs with a
tail (130); 1, 63, 64, 65 and 257 lines along the lane axis, i.e. one live lane, a partial wave, a full one, a wave plus one and
several workgroups; a box that is ONE line.  Every length has a line count of its own, so that the product stays small."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import device_layouts as L  # noqa: E402  (the layouts; test infrastructure)
import line_find_ref as R  # noqa: E402
from gt4py_amd import _lib  # noqa: E402
from gt4py_amd.cartesian.gtscript import IJ, PARALLEL, Field, computation, interval  # noqa: E402, F401

LANES, TILES, ITEMS = "lanes", "tiles", "items"
PATH_NAMES = {_lib.LINE_PATH_LANES: LANES, _lib.LINE_PATH_TILES: TILES, _lib.LINE_PATH_ITEMS: ITEMS}
#: (line length, the extents of the two other axes)
EXTENTS = [(1, (64, 1)), (2, (63, 1)), (3, (257, 1)), (4, (65, 2)), (5, (5, 3)), (15, (5, 3)), (16, (65, 2)), (17, (5, 3)), (31, (3, 2)),
           (32, (64, 1)), (33, (65, 2)), (130, (3, 2)), (17, (1, 1)), (130, (1, 1))]  # (the last two: a box that is ONE line)
AXES = "IJK"
MODES = [("crossing", "any"), ("crossing", "rising"), ("crossing", "falling"), ("argmax", "any"), ("argmin", "any")]
GUARD = 64  # doubles in front of and behind the result
MISSING = -999.25


def _shape(n, others, axis):
    shape = list(others)
    shape.insert(axis, n)
    return tuple(shape)


def expected_path(strides, coord_strides, extent, axis):
    """The rule of include/gt4py_amd.h restated: strides in ITEMS of every field, of the coord (None: no coord or a 1-d one, which
    is unit along the line and broadcast elsewhere)."""
    def unit(ax):
        return all(s[ax] == 1 for s in strides) and (coord_strides is None or coord_strides[ax] == 1)

    if unit(axis) and extent[axis] > 1:
        return TILES
    return LANES if any(unit(ax) and extent[ax] > 1 for ax in range(3) if ax != axis) else ITEMS


def _values(rng, shape, dtype, axis, f=0, coarse=False):
    """A random walk along the line axis around the levels 0.125 f: the first crossing can be anywhere on the line, some lines
    have none.  ``coarse``: multiples of 1/8, so that items equal to the level, pairs (L, L) and equal extrema are common."""
    v = np.cumsum(rng.uniform(-0.3, 0.3, shape), axis=axis) + rng.uniform(-0.6, 0.6, shape).take([0], axis=axis) + 0.125 * f
    return (np.round(v * 8) / 8 if coarse else v).astype(dtype)


def _native(t, start):
    size = t.element_size()
    return _lib.Field.make(t.data_ptr(), tuple(t.shape), tuple(s * size for s in t.stride()), start)


def _c_entry(fields, coord, extent, axis, size, what, direction, levels, reverse, start):
    """gt4mi_line_find on the current stream with the result inside a sentinel buffer: the guards are unchanged afterwards.
    Returns (the (nf, 3, nB, nA) result as the device left it, path, launches)."""
    import torch

    lib, nf = _lib.load(), len(fields)
    table = (_lib.Field * nf)(*[_native(t, start) for t in fields])
    if coord is None:
        z = None
    elif coord.dim() == 1:  # n items along the line axis: stride 0 along the two others
        shape, strides = [1, 1, 1], [0, 0, 0]
        shape[axis], strides[axis] = coord.shape[0], size
        z = ctypes.byref(_lib.Field.make(coord.data_ptr(), shape, strides, (0, 0, 0)))
    else:
        z = ctypes.byref(_native(coord, start))
    level = None if levels is None else (ctypes.c_double * nf)(*levels)
    a, b = (d for d in range(3) if d != axis)
    lines = extent[a] * extent[b]
    buf = torch.empty(nf * 3 * lines + 2 * GUARD, dtype=torch.int64, device="cuda")
    buf.fill_(L.SENTINEL[8])
    path, launches = ctypes.c_int(), ctypes.c_int()
    rc = lib.gt4mi_line_find(table, nf, z, _lib.domain3(extent), axis, size, _lib.FIND_CROSSING if what == "crossing" else
                             _lib.FIND_ARGMAX if what == "argmax" else _lib.FIND_ARGMIN, R.DIRECTIONS.index(direction), level, MISSING,
                             buf.data_ptr() + 8 * GUARD, _lib.FIND_REVERSE if reverse else 0, torch.cuda.current_stream().cuda_stream,
                             ctypes.byref(path), ctypes.byref(launches))
    _lib.check("gt4mi_line_find", rc)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (np.concatenate([host[:GUARD], host[-GUARD:]]).view(np.uint64) == L.SENTINEL[8]).all(), "the bytes around the result changed"
    return host[GUARD:-GUARD].view(np.float64).reshape(nf, 3, extent[b], extent[a]), PATH_NAMES[path.value], launches.value


def _run(extent, axis, what="crossing", direction="any", reverse=False, *, dtype=np.float64, layout="ifirst", coord=None, coord_layout=None,
         nfields=1, levels=None, halo=0, k0=0, seed=0, coarse=False, plant=None, want_path=None):
    """One search through the C entry and through ``linefind.LineFind``; every byte of both results is compared with the
    restatement, every input must come back unchanged.  ``extent`` is the box that is searched (the halo included).  ``coord``:
    None, ``"ijk"`` (in ``coord_layout``, default the fields') or ``"line"`` (1-d).  ``plant(boxes, coord_box)`` edits the boxes
    of the fields (and the coord's) in place.  Returns (the (nf, 3, nB, nA) result, the LineFind)."""
    import torch

    from gt4py_amd import linefind

    rng = np.random.default_rng([seed, *extent, axis])
    zrng = np.random.default_rng([seed, *extent, axis, 1])  # (the coord does not depend on how many fields there are)
    # one ghost cell in front of the box on the low sides of I and J, one behind the array the product sees, k0 levels below
    shape = (extent[0] + 2, extent[1] + 2, extent[2] + k0)
    box = (slice(1, 1 + extent[0]), slice(1, 1 + extent[1]), slice(k0, None))
    origin, start = (1 + halo, 1 + halo, k0), (1, 1, k0)
    n = extent[axis]
    xs = [_values(rng, shape, dtype, axis, f, coarse) for f in range(nfields)]
    if what == "crossing" and levels is None:
        levels = [0.125 * f for f in range(nfields)]
    z_full = z_box = d_coord = None
    if coord == "ijk":
        z_full = np.cumsum(zrng.uniform(0.5, 2, shape), axis=axis).astype(dtype)
        z_box = z_full[box]
    elif coord == "line":
        z_box = np.cumsum(zrng.uniform(0.5, 2, n)).astype(dtype)
    if plant is not None:
        plant([x[box] for x in xs], z_box)
    if coord == "ijk":
        d_coord = L.Dev(shape, dtype, coord_layout or layout, z_full, 1)
    elif coord == "line":
        d_coord = L.Line(z_box)
    devs = [L.Dev(shape, dtype, layout, x, 1) for x in xs]
    lf = linefind.LineFind([d.given for d in devs], axis=AXES[axis], what=what, level=levels, direction=direction, reverse=reverse,
                           coord=None if d_coord is None else d_coord.given, missing=MISSING, halo=halo, origin=origin)
    lines = extent[(axis + 1) % 3] * extent[(axis + 2) % 3]
    assert (lf.n, lf.lines, lf.extent, lf.launches) == (n, lines, tuple(extent), -(-nfields // 8))
    if want_path is None:
        want_path = expected_path([d.lay.strides for d in devs], d_coord.lay.strides if isinstance(d_coord, L.Dev) else None, extent, axis)
    assert lf.path == want_path, (lf.path, want_path)
    lf()
    torch.cuda.synchronize()
    owned = lf.result.tensor.cpu().numpy()
    got, path, launches = _c_entry([d.given for d in devs], None if d_coord is None else d_coord.given, extent, axis, np.dtype(dtype).itemsize,
                                   what, direction, levels, reverse, start)
    assert (path, launches) == (lf.path, lf.launches)
    about = (f"axis {AXES[axis]} extent {extent} {what} {direction} reverse {reverse} coord {coord} {np.dtype(dtype)} {layout} "
             f"{nfields} field(s) {lf.path}")
    assert owned.shape == got.shape and owned.tobytes() == got.tobytes(), f"{about}: the C entry and LineFind differ"
    for f, x in enumerate(xs):
        want = R.find_along(x[box], axis, what, None if levels is None else levels[f], direction, reverse, z_box, MISSING).transpose(0, 2, 1)
        ok = (got[f].view(np.uint64) == np.ascontiguousarray(want).view(np.uint64)) | (np.isnan(got[f]) & np.isnan(want))
        if not ok.all():
            bad = np.argwhere(~ok)
            raise AssertionError(f"{about}: field {f}: {len(bad)} of {ok.size} result items differ, first (row, b, a) {bad[:4].tolist()}: got "
                                 f"{[got[f][tuple(i)] for i in bad[:4]]}, want {[want[tuple(i)] for i in bad[:4]]}")
    for f, d in enumerate(devs):
        d.assert_unchanged(f"{about}: field {f}")
    if d_coord is not None:
        d_coord.assert_unchanged(f"{about}: coord")
    return got, lf


@pytest.mark.parametrize("layout", ["ifirst", "kfirst"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_extents_at_look_ahead_tile_wave_and_workgroup_boundaries(axis, layout):
    for k, (n, others) in enumerate(EXTENTS):
        for d, dtype in enumerate((np.float32, np.float64)):
            for m, (what, direction) in enumerate(MODES):
                _run(_shape(n, others, axis), axis, what, direction, bool((k + m + d) % 2), dtype=dtype, layout=layout,
                     coord=(None, "ijk", "line")[(k + m) % 3], coarse=bool((k + d) % 2), seed=1)


@pytest.mark.parametrize("layout", ["jfirst", "ifirst_unaligned"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_halo_with_live_data_outside_the_box_and_an_origin_off_zero(axis, layout):
    """The ghost cells around the box hold data like the box's; with halo 1 the box is the domain and its ghost ring."""
    for halo in (0, 1):
        _run(_shape(17, (9, 7), axis), axis, "crossing", "any", True, dtype=np.float64, layout=layout, nfields=2, coord="ijk", halo=halo, k0=1, seed=6)
        _run(_shape(17, (9, 7), axis), axis, "argmin", dtype=np.float32, layout=layout, nfields=2, halo=halo, k0=1, coarse=True, seed=6)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["ifirst", "kfirst"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_planted_crossings_at_every_pair_of_the_line(axis, layout, dtype):
    """Line l of 130 crosses the level 0 exactly once, upwards, in pair l mod 39: every pair of the line is some line's, the pairs
    that straddle a tile-run seam (items 15 | 16 for float64, 31 | 32 for float32), the look-ahead seam (3 | 4), the first and the
    last among them.  Some lines have no crossing, some start ON the level, some end on it -- all in the same waves."""
    n, others = 40, (65, 2)
    extent = _shape(n, others, axis)
    where, kind = {}, {}

    def plant(boxes, z):
        rng = np.random.default_rng(11)
        lines = np.empty((n, 130), dtype=dtype)  # line l = a * nB + b: the order of a section's [a, b] flattened
        for l in range(130):
            mag = rng.uniform(0.5, 1.5, n)
            where[l], kind[l] = l % (n - 1), "plain"
            lines[:, l] = np.where(np.arange(n) <= where[l], -mag, mag)
            if l % 7 == 3:
                lines[:, l], kind[l] = -mag, "none"
            elif l % 11 == 5:
                lines[0, l], kind[l] = 0.0, "first"  # item 0 of the forward scan is ON the level
            elif l % 13 == 6:
                lines[n - 1, l], kind[l] = 0.0, "last"  # item 0 of the reverse scan is
        np.moveaxis(boxes[0], axis, 0)[...] = lines.reshape(n, *others)

    for reverse in (False, True):
        got, lf = _run(extent, axis, "crossing", "any", reverse, dtype=dtype, layout=layout, coord="ijk", levels=[0.0], seed=11, plant=plant)
        position, crossings = got[0, 0].T.reshape(-1), got[0, 2].T.reshape(-1)
        for l, p in where.items():
            if kind[l] == "none":
                assert position[l] == MISSING and crossings[l] == 0, (l, reverse)
            elif kind[l] == "plain":
                assert p < position[l] < p + 1 and crossings[l] == 1, (l, p, reverse, position[l])
            elif kind[l] == "first" and not reverse:
                assert position[l] == 0, (l, position[l])
            elif kind[l] == "last" and reverse:
                assert position[l] == n - 1, (l, position[l])
    # in scan order the reverse search sees every one of them fall
    plain = [l for l in where if kind[l] == "plain"]
    got, _ = _run(extent, axis, "crossing", "rising", True, dtype=dtype, layout=layout, levels=[0.0], seed=11, plant=plant)
    assert (got[0, 0].T.reshape(-1)[plain] == MISSING).all()
    got, _ = _run(extent, axis, "crossing", "falling", True, dtype=dtype, layout=layout, levels=[0.0], seed=11, plant=plant)
    assert (got[0, 0].T.reshape(-1)[plain] != MISSING).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", ["ifirst", "kfirst"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_planted_extrema_on_both_sides_of_a_seam_and_nans(axis, layout, dtype):
    """Equal maxima in items s and s + 1, s = 3 (the look-ahead seam), 15 and 31 (the tile-run seams of float64 and float32):
    forward takes the first, reverse the last.  A NaN behind the maximum wins, also in the last item."""
    n, others = 40, (65, 2)
    extent = _shape(n, others, axis)
    seams = (3, 15, 31)

    def plant(boxes, z):
        lines = np.moveaxis(boxes[0], axis, 0).reshape(n, 130)  # (a copy) line l = a * nB + b
        for l in range(130):
            s = seams[l % 3]
            lines[s, l] = lines[s + 1, l] = 50.0
            if l % 5 == 1:
                lines[s + 3, l] = np.nan
            elif l % 5 == 2:
                lines[n - 1, l] = np.nan
        np.moveaxis(boxes[0], axis, 0)[...] = lines.reshape(n, *others)

    for reverse in (False, True):
        got, _ = _run(extent, axis, "argmax", "any", reverse, dtype=dtype, layout=layout, coord="line", seed=12, plant=plant)
        position, value = got[0, 0].T.reshape(-1), got[0, 2].T.reshape(-1)
        for l in range(130):
            s = seams[l % 3]
            if l % 5 == 1:
                assert position[l] == s + 3 and np.isnan(value[l]), (l, reverse)
            elif l % 5 == 2:
                assert position[l] == n - 1 and np.isnan(value[l]), (l, reverse)
            else:
                assert position[l] == (s + 1 if reverse else s) and value[l] == 50.0, (l, reverse, position[l])


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_one_to_nine_fields_with_distinct_levels(axis):
    """9 fields are two launches; a field's rows are those of the same field alone, at every position and in every company."""
    extent = _shape(17, (5, 3), axis)
    for what, coord in (("crossing", "ijk"), ("argmin", None)):
        nine, lf = _run(extent, axis, what, dtype=np.float32, nfields=9, coord=coord, seed=5)
        assert lf.launches == 2
        for count in (8, 4, 1):
            some, _ = _run(extent, axis, what, dtype=np.float32, nfields=count, coord=coord, seed=5)
            assert some.tobytes() == nine[:count].tobytes(), (what, count)
    big = _shape(33, (65, 2), axis)
    # float64 with all 8 entries (the largest register budgets) on each path: ifirst and kfirst between them reach LANES and TILES
    for layout in ("ifirst", "kfirst"):
        _run(big, axis, "crossing", "falling", True, dtype=np.float64, layout=layout, nfields=8, coord="ijk", seed=5)
        _run(big, axis, "argmax", dtype=np.float64, layout=layout, nfields=9, coord="line", coarse=True, seed=5)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_coord_of_another_layout_falls_back_to_items_and_a_1d_coord_keeps_the_path(axis, dtype):
    extent = _shape(33, (65, 2), axis)
    for layout, other in (("ifirst", "kfirst"), ("kfirst", "ifirst")):
        for what, reverse in (("crossing", False), ("crossing", True), ("argmax", True)):
            a, lf = _run(extent, axis, what, "any", reverse, dtype=dtype, layout=layout, coord="ijk", coord_layout=other, nfields=2, seed=7,
                         want_path=ITEMS)
            b, lf = _run(extent, axis, what, "any", reverse, dtype=dtype, layout=layout, coord="ijk", nfields=2, seed=7)
            assert lf.path != ITEMS and a.tobytes() == b.tobytes(), (layout, what, reverse)  # the same lines through two kernels
            _, lf = _run(extent, axis, what, "any", reverse, dtype=dtype, layout=layout, coord="line", nfields=2, seed=7)
            assert lf.path == (TILES if L.geometry((2, 2, 2), layout, 8, 0)[1][axis] == 1 else LANES)


def test_set_level_between_two_calls_moves_the_result_with_no_rebuild():
    import torch

    from gt4py_amd import linefind

    rng = np.random.default_rng(13)
    shape = (24, 9, 30)
    t = (280.0 - 6.5 * np.arange(30) + rng.uniform(-2, 2, shape)).astype(np.float32)  # a lapse rate with noise: not monotone
    z = np.cumsum(rng.uniform(0.2, 0.4, shape), axis=2).astype(np.float32)
    d_t, d_z = torch.from_numpy(t).cuda(), torch.from_numpy(z).cuda()
    fz = linefind.LineFind([d_t], axis="K", what="crossing", level=273.15, coord=d_z)
    before, result_ptr = fz._before, fz.result.ptr
    for level in (273.15, 250.0, 400.0, 273.15):
        fz.set_level(level)
        fz()
        found, = fz.get()
        want = R.find_along(t, 2, "crossing", level, coord=z)
        assert R.same_bits(found.position, want[0]).all() and R.same_bits(found.coord, want[1]).all(), level
        assert np.array_equal(found.crossings, want[2].astype(np.int64)) and found.value is None
        assert np.isnan(found.position).all() == (level == 400.0)
    assert fz._before is before and fz.result.ptr == result_ptr and fz.level == (273.15,)
    one, = linefind.find_lines(d_t, axis="K", what="crossing", level=273.15, coord=d_z)  # the one-shot form
    assert R.same_bits(one.coord, found.coord).all()
    jet, = linefind.find_lines(d_t, axis=1, what="argmax", reverse=True)
    want = R.find_along(t, 1, "argmax", reverse=True)
    assert R.same_bits(jet.position, want[0]).all() and R.same_bits(jet.value, want[2]).all() and jet.crossings is None


def below_the_surface(t: Field[np.float64], z: Field[np.float64], h0: Field[IJ, np.float64], out: Field[np.float64]):
    with computation(PARALLEL), interval(...):
        out = t if z < h0 else 0.0


def test_section_feeds_a_stencil_in_the_same_stream_without_synchronisation():
    """fz() on a side stream, then a device_sync=False stencil that takes fz.section("coord") as Field[IJ, np.float64] in the same
    stream, nothing in between: the stencil reads what the call wrote."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import linefind
    from gt4py_amd.cartesian import gtscript

    backend, domain = "hip:mi300", (40, 33, 20)
    stencil = gtscript.stencil(backend=backend, definition=below_the_surface, device_sync=False)
    rng = np.random.default_rng(17)
    host_t = 290.0 - 6.5 * np.arange(20) / 4 + rng.uniform(-3, 3, domain)
    host_z = np.cumsum(rng.uniform(200, 300, domain), axis=2)
    t, z = (gt_storage.from_array(v, backend=backend) for v in (host_t, host_z))
    out = gt_storage.zeros(domain, backend=backend)
    fz = linefind.LineFind([t], axis="K", what="crossing", level=273.15, coord=z, missing=-1.0)
    assert fz.path == LANES  # the storage preset is I-contiguous
    h0 = fz.section("coord")
    assert h0.shape == domain[:2] and h0.dtype == np.float64 and h0.strides == (8, 8 * domain[0]) and h0.ptr == fz.result.ptr + 8 * 40 * 33
    stencil(t, z, h0, out)  # (compiled and loaded before the order matters)
    torch.cuda.synchronize()
    out.tensor.fill_(float("nan"))
    fz.result.tensor.fill_(float("nan"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        fz()
        stencil(t, z, h0, out)
    found, = fz.get()  # synchronises the stream both went to
    want = R.find_along(host_t, 2, "crossing", 273.15, coord=host_z, missing=-1.0)
    assert R.same_bits(found.coord, want[1]).all() and R.same_bits(h0.get(), want[1]).all()
    assert (want[2] > 0).any() and (want[1] > 0).any()
    assert R.same_bits(out.get(), np.where(host_z < want[1][:, :, None], host_t, 0.0)).all()
