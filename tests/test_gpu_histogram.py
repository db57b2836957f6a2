"""``gt4py_amd.histogram`` on the GPU: against the contract's restatement (tests/histogram_ref.py) over EVERY byte of the result,
with sentinel words in front of and behind it.  Every case goes through the C entry (the result inside the sentinel buffer, which
also holds the sentinel where the result will be: the entry must zero it) AND through ``histogram.Histogram`` (the result the object
owns): the two blocks must hold the same bytes.  Every field must come back unchanged.

The pads of every buffer and the ghost cells around the box hold IN-RANGE values: a kernel that reads one of them miscounts.
The extents cross every boundary of the kernel: below, across and just past a 16-byte lane (ni = 1, 3, 5), a wave (63, 65) and a
pass of 256 units (257), several lines and levels, in the four layouts -- so that both paths and every unit-stride axis are hit."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import device_layouts as L  # noqa: E402  (the layouts; test infrastructure)
import histogram_ref as R  # noqa: E402
from gt4py_amd import _lib  # noqa: E402

ROWS, ITEMS = "rows", "items"
PATH_NAMES = {_lib.HISTOGRAM_PATH_ROWS: ROWS, _lib.HISTOGRAM_PATH_ITEMS: ITEMS}
GUARD = 64  # int64 words in front of and behind the result
NI, NJ, NK = (1, 3, 5, 63, 65, 257), (1, 2, 7), (1, 2, 5)


def uniform_edges(nb, lo=-2.0, hi=3.0):
    return np.linspace(lo, hi, nb + 1)


def log_edges(nb):
    return np.concatenate([[0.0], np.logspace(-4, 1, nb)]) if nb > 1 else np.array([1e-4, 10.0])


def ulp_edges(nb, seed=0):
    e = uniform_edges(nb)
    k = np.random.default_rng(seed).integers(0, 3, nb + 1) - 1
    return np.where(k < 0, np.nextafter(e, -np.inf), np.where(k > 0, np.nextafter(e, np.inf), e))


def expected_path(strides, extent, by_k):
    """include/gt4py_amd.h's rule restated: ROWS if every field has unit item stride along an axis of a row's box longer than 1."""
    row = (extent[0], extent[1], 1 if by_k else extent[2])
    return ROWS if all(any(s[ax] == 1 and row[ax] > 1 for ax in range(3)) for s in strides) else ITEMS


def _values(rng, shape, dtype, e):
    """Mostly inside the edges, some beyond either end, a few NaN and infinities."""
    lo, hi = float(e.min()), float(e.max())
    v = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), shape)
    flat = v.reshape(-1)
    n = flat.size
    for value in (np.nan, np.inf, -np.inf, lo, hi):
        flat[rng.integers(0, n, max(1, n // 97))] = value
    return v.astype(dtype)


def _device(shape, dtype, layout, values, fill, align_i=1):
    """A ``device_layouts.Dev`` whose every byte outside the view holds ``fill`` (an in-range value) instead of the NaN sentinel."""
    d = L.Dev(shape, dtype, layout, None, align_i)
    d.image.view(d.dtype)[:] = fill
    d.host(d.image)[...] = values
    d.lay.upload(d.image)
    return d


def _native(t, start):
    size = t.element_size()
    return _lib.Field.make(t.data_ptr(), tuple(t.shape), tuple(s * size for s in t.stride()), start)


def _c_entry(fields, start, extent, size, edges, by_k, flags=0, calls=1):
    """gt4mi_field_histogram on the current stream, ``calls`` times, with the result inside a buffer that holds the sentinel
    EVERYWHERE: the guards are unchanged afterwards.  Returns ((nf, nrows, nb + 3) int64 as the device left it, path, launches)."""
    import torch

    lib, nf = _lib.load(), len(fields)
    e = np.ascontiguousarray(edges, dtype=np.float64)
    nb = e.shape[-1] - 1
    if e.ndim == 2:
        flags |= _lib.HISTOGRAM_EDGES_PER_FIELD
    table = (_lib.Field * nf)(*[_native(t, start) for t in fields])
    nrows = extent[2] if by_k else 1
    words = nf * nrows * (nb + R.EXTRA)
    buf = torch.empty(words + 2 * GUARD, dtype=torch.int64, device="cuda")
    buf.fill_(L.SENTINEL[8])
    if flags & _lib.HISTOGRAM_ACCUMULATE:
        buf[GUARD: GUARD + words] = 0
    d_edges = torch.from_numpy(e).cuda()
    path, launches = ctypes.c_int(), ctypes.c_int()
    rc = lib.gt4mi_field_histogram(table, nf, _lib.domain3(extent), size, nb, d_edges.data_ptr(), e.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                   int(by_k), None, flags | _lib.HISTOGRAM_DRY_RUN, None, ctypes.byref(path), ctypes.byref(launches))
    _lib.check("gt4mi_field_histogram", rc)
    for _ in range(calls):
        rc = lib.gt4mi_field_histogram(table, nf, _lib.domain3(extent), size, nb, d_edges.data_ptr(), None, int(by_k), buf.data_ptr() + 8 * GUARD,
                                       flags, torch.cuda.current_stream().cuda_stream, None, None)
        _lib.check("gt4mi_field_histogram", rc)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (np.concatenate([host[:GUARD], host[-GUARD:]]).view(np.uint64) == L.SENTINEL[8]).all(), "the words around the result changed"
    assert np.array_equal(d_edges.cpu().numpy().view(np.uint64), e.view(np.uint64)), "the edges changed"
    return host[GUARD:-GUARD].reshape(nf, nrows, nb + R.EXTRA), PATH_NAMES[path.value], launches.value


def _run(extent, edges, *, dtype=np.float32, layout="ifirst", nfields=1, by=None, k0=0, seed=0, plant=None, make=None, want_path=None, align_i=1):
    """One histogram through the C entry and through ``histogram.Histogram``; every byte of both results is compared with the
    restatement, every field must come back unchanged.  ``extent`` is the box, which lies inside live data: one ghost cell in
    front of it on the low sides of I and J, one behind it (and the array's last row and column behind that), ``k0`` levels
    below.  ``plant(boxes)`` edits the fields' boxes in place; ``make(rng, shape, f)`` replaces the random values.  ``align_i``: the column
    of the array that lies on a 256-byte boundary in the ``ifirst`` layout (1: the box's first column).  Returns (the
    (nf, nrows, nb + 3) result, the Histogram)."""
    import torch

    from gt4py_amd import histogram

    e = np.asarray(edges, dtype=np.float64)
    rng = np.random.default_rng([seed, *extent])
    shape = (extent[0] + 3, extent[1] + 3, extent[2] + k0)  # (Dev gives the product all but the last row and column)
    box = (slice(1, 1 + extent[0]), slice(1, 1 + extent[1]), slice(k0, None))
    start = (1, 1, k0)
    sets = [e[f] if e.ndim == 2 else e for f in range(nfields)]
    xs = [(_values(rng, shape, dtype, sets[f]) if make is None else make(rng, shape, f).astype(dtype)) for f in range(nfields)]
    if plant is not None:
        plant([x[box] for x in xs])
    devs = [_device(shape, dtype, layout, x, 0.5 * (sets[f][0] + sets[f][1]), align_i) for f, x in enumerate(xs)]
    by_k = by == "K"
    h = histogram.Histogram([d.given for d in devs], edges=e, by=by, origin=start, domain=extent)
    if want_path is None:
        want_path = expected_path([d.lay.strides for d in devs], extent, by_k)
    assert (h.path, h.launches, h.domain, h.rows) == (want_path, 1, tuple(extent), extent[2] if by_k else 1), (h.path, want_path)
    h()
    torch.cuda.synchronize()
    owned = h.result.tensor.cpu().numpy()
    got, path, launches = _c_entry([d.given for d in devs], start, extent, np.dtype(dtype).itemsize, e, by_k)
    assert (path, launches) == (h.path, 1)
    about = f"extent {extent} {np.dtype(dtype)} {layout} {nfields} field(s) nb {e.shape[-1] - 1} by {by} {h.path}"
    assert owned.shape == got.shape and owned.tobytes() == got.tobytes(), f"{about}: the C entry and Histogram differ"
    items = extent[0] * extent[1] * (1 if by_k else extent[2])
    for f, x in enumerate(xs):
        want = R.count_box(x[box], sets[f], by_k)
        if got[f].tobytes() != want.tobytes():
            bad = np.argwhere(got[f] != want)
            raise AssertionError(f"{about}: field {f}: {len(bad)} of {want.size} counters differ, first (row, slot) {bad[:6].tolist()}: got "
                                 f"{[int(got[f][tuple(i)]) for i in bad[:6]]}, want {[int(want[tuple(i)]) for i in bad[:6]]}")
        assert (got[f].sum(axis=-1) == items).all(), f"{about}: a row does not sum to the {items} items of its box"
    for d in devs:
        d.assert_unchanged(f"{about}: a field")
    return got, h


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", L.LAYOUTS)
def test_every_small_shape_in_every_layout_on_both_paths(layout, dtype):
    e = uniform_edges(13)
    seen = set()
    for n, ni in enumerate(NI):
        for nj in NJ:
            for nk in NK:
                for by in (None, "K"):
                    _, h = _run((ni, nj, nk), e, dtype=dtype, layout=layout, by=by, k0=nj % 3, seed=n)
                    seen.add(h.path)
    # whole-box calls find a unit-stride axis in every layout once it is longer than 1; per level a K-contiguous field goes item by item
    assert seen == {ROWS, ITEMS}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("align_i", [0, 1, 2, 3])
def test_lines_that_start_off_a_16_byte_boundary_have_a_partial_lane_in_front(align_i, dtype):
    """In the ``ifirst`` layout the column ``align_i`` lies on a 256-byte boundary and the box starts at column 1: its lines start
    1 - align_i items (mod the lane) behind a 16-byte boundary, so the lanes path walks several lines with 3, 0, 1 and 2 float32
    items (1, 0, 1, 0 float64 items) in front of the first whole lane, and a partial lane behind the last."""
    e = uniform_edges(21)
    V = 16 // np.dtype(dtype).itemsize
    for ni in (2 * V, 2 * V + 1, 66, 67, 257):
        for by in (None, "K"):
            assert _run((ni, 5, 3), e, dtype=dtype, by=by, align_i=align_i, seed=ni)[1].path == ROWS


@pytest.mark.parametrize("case", ["items float32", "lanes float64", "one counter copy"])
def test_workgroups_that_make_several_passes(case):
    """8 fields and many rows leave few workgroups per row (one resident wave of workgroups over the whole call), so each walks
    its part of the row in several passes of 1024 units: 2 passes item by item (an odd pitch), 2 in 16-byte lanes, 3 above 1024
    bins (half as many workgroups).  The bound is restated here from csrc/field_histogram.hip.h's sizing."""
    extent, dtype, layout, by, nb, resident = {"items float32": ((300, 140, 5), np.float32, "ifirst_unaligned", "K", 40, 1536),
                                               "lanes float64": ((128, 50, 64), np.float64, "ifirst", "K", 40, 1536),
                                               "one counter copy": ((300, 140, 5), np.float32, "ifirst_unaligned", "K", 2000, 768)}[case]
    units = extent[0] * extent[1] // (2 if case == "lanes float64" else 1)
    chunks = max(1, min(resident // (extent[2] * 8), -(-units // 1024)))
    assert -(-units // chunks) > 1024, "the shape no longer forces a second pass"
    _run(extent, uniform_edges(nb), dtype=dtype, layout=layout, nfields=8, by=by)


def test_what_the_layouts_are_for():
    e = uniform_edges(8)
    for layout, whole, per_level in (("ifirst", ROWS, ROWS), ("ifirst_unaligned", ROWS, ROWS), ("jfirst", ROWS, ROWS), ("kfirst", ROWS, ITEMS)):
        for dtype in (np.float32, np.float64):
            assert _run((21, 6, 9), e, dtype=dtype, layout=layout)[1].path == whole
            assert _run((21, 6, 9), e, dtype=dtype, layout=layout, by="K")[1].path == per_level
    # a strided view of an I-contiguous parent (every second column): no unit stride anywhere
    import torch

    from gt4py_amd import histogram

    parent = np.random.default_rng(0).uniform(-2, 3, (40, 6, 4)).astype(np.float32)
    view = torch.from_numpy(parent).cuda().permute(2, 1, 0).contiguous().permute(2, 1, 0)[::2]  # I-contiguous parent, stride 2 along I
    assert view.stride()[0] == 2
    for by in (None, "K"):
        h = histogram.Histogram([view], edges=e, by=by)
        assert h.path == ITEMS
        h()
        got, = h.get()
        want = R.count_box(parent[::2], e, by == "K")
        assert np.array_equal(np.atleast_2d(got.counts), want[:, :8]) and np.array_equal(np.atleast_1d(got.nan), want[:, 8 + R.NAN])


@pytest.mark.parametrize("nfields", [1, 4, 8])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_several_fields_with_shared_and_per_field_edges(nfields, dtype):
    shared = log_edges(20)
    per_field = np.stack([uniform_edges(20, -1.0 - f, 2.0 + 0.5 * f) for f in range(nfields)])
    for e in (shared, per_field):
        for by in (None, "K"):
            for layout in ("ifirst", "kfirst"):
                _run((37, 5, 3), e, dtype=dtype, layout=layout, nfields=nfields, by=by)


@pytest.mark.parametrize("kind", [uniform_edges, log_edges, ulp_edges])
@pytest.mark.parametrize("nb", [1, 2, 64, 1000, _lib.HISTOGRAM_MAX_BINS])
def test_every_number_of_bins_and_kind_of_edges(nb, kind):
    e = kind(nb)
    for dtype in (np.float32, np.float64):
        # items ON edges and one ulp (of the item type) beside them are common: every edge rounded to the type, and its neighbours
        def make(rng, shape, f, dtype=dtype):
            near = e.astype(dtype)[rng.integers(0, nb + 1, shape)]
            step = rng.integers(-1, 2, shape)
            near = np.where(step < 0, np.nextafter(near, dtype(-np.inf)), np.where(step > 0, np.nextafter(near, dtype(np.inf)), near))
            return np.where(rng.integers(0, 2, shape) == 0, near, _values(rng, shape, dtype, e))

        _run((67, 9, 3), e, dtype=dtype, make=make)
        _run((67, 9, 3), e, dtype=dtype, by="K", layout="jfirst", make=make)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_directed_items_at_the_ends_of_a_line_and_across_a_lane_seam(dtype):
    e = np.array([-1.0, 0.0, float(np.float32(0.1)), 0.5, 2.0])
    tiny = np.finfo(dtype).smallest_subnormal
    special = [-1.0, 0.0, -0.0, 0.5, 2.0, np.nextafter(dtype(2.0), dtype(3)), np.nextafter(dtype(2.0), dtype(0)), np.nextafter(dtype(-1.0), dtype(-2)),
               np.inf, -np.inf, np.nan, tiny, -tiny, dtype(0.1), np.nextafter(dtype(0.5), dtype(0)), np.nextafter(dtype(0.5), dtype(1))]
    V = 16 // np.dtype(dtype).itemsize
    for layout in ("ifirst", "ifirst_unaligned", "kfirst"):
        for ni in (2 * V + 1, 67):
            for at in (0, ni - 1, V - 1, V, V + 1, 2 * V - 1, 2 * V):  # the first and last item of a line, both sides of the lane seams
                def plant(boxes, at=at):
                    for n, v in enumerate(special):
                        boxes[0][min(at, boxes[0].shape[0] - 1), n % boxes[0].shape[1], n % boxes[0].shape[2]] = v
                        boxes[0][n % boxes[0].shape[0], n % boxes[0].shape[1], min(at, boxes[0].shape[2] - 1)] = v  # (along K for kfirst)

                _run((ni, 4, 2 * V + 1), e, dtype=dtype, layout=layout, plant=plant, seed=at)
                _run((ni, 4, 3), e, dtype=dtype, layout=layout, plant=plant, by="K", seed=at)


@pytest.mark.parametrize("by", [None, "K"])
def test_the_hot_bin_cases(by):
    e = uniform_edges(32, 0.0, 8.0)
    extent = (130, 9, 4)
    constant = lambda rng, shape, f: np.full(shape, 2.6)  # noqa: E731  every lane of every wave in ONE bin
    mostly_zero = lambda rng, shape, f: np.where(rng.uniform(0, 1, shape) < 0.9, 0.0, rng.uniform(0, 8, shape))  # noqa: E731
    all_differ = lambda rng, shape, f: (np.arange(np.prod(shape)).reshape(shape[::-1]).T % 32) * 0.25 + 0.125  # noqa: E731  bin = item index mod 32
    two_hot = lambda rng, shape, f: np.where(rng.integers(0, 2, shape) == 0, 0.0, 7.9)  # noqa: E731  two bins: both peels are used
    three = lambda rng, shape, f: rng.integers(0, 3, shape) * 3.0  # noqa: E731  three bins: the per-lane adds follow the peels
    all_nan = lambda rng, shape, f: np.full(shape, np.nan)  # noqa: E731
    for make in (constant, mostly_zero, all_differ, two_hot, three, all_nan):
        for dtype, layout in ((np.float32, "ifirst"), (np.float64, "ifirst_unaligned"), (np.float32, "kfirst")):
            got, _ = _run(extent, e, dtype=dtype, layout=layout, by=by, make=make)
            if make is constant:
                assert got[0, :, 10].tolist() == [130 * 9 * (1 if by else 4)] * got.shape[1]
    _run(extent, uniform_edges(_lib.HISTOGRAM_MAX_BINS, 0.0, 8.0), by=by, make=mostly_zero)  # one counter copy per workgroup


def test_levels_with_disjoint_ranges_count_into_their_own_rows():
    nk, nb = 5, 10
    e = uniform_edges(nb, 0.0, 10.0)
    make = lambda rng, shape, f: rng.uniform(0.0, 2.0, shape) + 2.0 * (np.arange(shape[2]) % nk)  # noqa: E731  level k of the BOX in [2k, 2k+2)
    for dtype in (np.float32, np.float64):
        for layout in L.LAYOUTS:
            got, _ = _run((65, 7, nk), e, dtype=dtype, layout=layout, by="K", make=make)
            for k in range(nk):
                assert got[0, k, 2 * k: 2 * k + 2].sum() == 65 * 7 and got[0, k].sum() == 65 * 7, (layout, k, got[0, k])


def test_zeroing_accumulation_and_reset_in_stream_order():
    import torch

    from gt4py_amd import histogram

    e = uniform_edges(50)
    rng = np.random.default_rng(11)
    x = _values(rng, (70, 12, 6), np.float32, e)
    dev = _device(x.shape, np.float32, "ifirst", x, 0.0)
    field = dev.given  # (all but the last row and column of the buffer)
    want = R.count_box(x[:-1, :-1][1:-1, 2:-2], e, True)
    # halo alone sets the box: origin (1, 2, 0), what remains in front of the high ghost cells
    plain = histogram.Histogram([field], edges=e, by="K", halo=(1, 2))
    assert plain.origin == (1, 2, 0) and plain.domain == (67, 7, 6)
    plain()
    first = plain.result.tensor.clone()
    plain()
    torch.cuda.synchronize()
    assert first.cpu().numpy().tobytes() == want[None].tobytes(), "the first call"
    assert plain.result.tensor.cpu().numpy().tobytes() == want[None].tobytes(), "a second call without accumulate: the result is zeroed first"
    run = histogram.Histogram([field], edges=e, by="K", halo=(1, 2), accumulate=True)
    for calls in (1, 2, 3):
        run()
        assert run.result.tensor.cpu().numpy().tobytes() == (calls * want)[None].tobytes(), f"{calls} accumulating calls"
    run.reset()
    assert not run.result.tensor.any().item()
    run()
    got, = run.get()
    assert np.array_equal(got.counts, want[:, :50]) and np.array_equal(got.total, np.full(6, 67 * 7))
    assert np.array_equal(run.counts().tensor.cpu().numpy(), want[:, :50])
    # the C entry: two accumulating calls into a zeroed result double every counter, the guards stay
    twice, _, _ = _c_entry([field], (1, 2, 0), (67, 7, 6), 4, e, True, flags=_lib.HISTOGRAM_ACCUMULATE, calls=2)
    assert twice.tobytes() == (2 * want)[None].tobytes()
    again, _, _ = _c_entry([field], (1, 2, 0), (67, 7, 6), 4, e, True, calls=2)
    assert again.tobytes() == want[None].tobytes()
    # the one-shot form
    one, = histogram.histogram(field, edges=e, halo=(1, 2))
    assert np.array_equal(one.counts, want[:, :50].sum(axis=0)) and one.total == 67 * 7 * 6
    dev.assert_unchanged("the field")


def test_a_call_on_another_stream_is_ordered_with_torch_work_in_that_stream():
    import torch

    from gt4py_amd import histogram

    e = uniform_edges(16, 0.0, 16.0)
    side = torch.cuda.Stream()
    field = torch.zeros((129, 33, 8), dtype=torch.float32, device="cuda")
    h = histogram.Histogram([field], edges=e)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        field.fill_(3.5)            # written in the side stream ...
        h()                         # ... counted behind it in the same stream ...
        total = h.counts().tensor.sum()  # ... and read behind that by torch, with no synchronisation in between
        bin3 = h.counts().tensor[3].clone()
    side.synchronize()
    assert int(total) == field.numel() and int(bin3) == field.numel()


def test_the_four_quadrants_merge_into_the_whole_box():
    from gt4py_amd import histogram

    e = log_edges(40)
    rng = np.random.default_rng(21)
    x = _values(rng, (90, 50, 4), np.float64, e)
    dev = _device(x.shape, np.float64, "ifirst", x, 1.0)
    field = dev.given
    for by in (None, "K"):
        whole, = histogram.histogram(field, edges=e, by=by, origin=(2, 3, 0), domain=(85, 45, 4))
        parts = [histogram.histogram(field, edges=e, by=by, origin=(2 + oi, 3 + oj, 0), domain=(di, dj, 4))[0]
                 for oi, di in ((0, 41), (41, 44)) for oj, dj in ((0, 22), (22, 23))]
        merged = histogram.merge_histograms(parts)
        want = R.count_box(x[2:87, 3:48], e, by == "K")
        for name in ("counts", "below", "above", "nan"):
            assert np.array_equal(getattr(merged, name), getattr(whole, name)), (by, name)
        assert np.array_equal(np.atleast_2d(whole.counts), want[:, :40]) and np.array_equal(np.atleast_1d(whole.total), want.sum(axis=-1))
