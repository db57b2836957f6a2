"""``gt4mi_line_stats`` / ``diagnostics.LineStats`` on the GPU: every comparison is BIT EQUALITY of the whole result with the
restatement of the documented order (tests/line_stats_ref.py) -- every axis, both item types, every path, the line lengths at
which the order changes shape; the bytes around the fields, the workspace and the result; the same bits from every layout;
special values; the order-free slots against ``field_stats``; a section handed to a stencil on the device; a dead field."""

import ctypes
import functools
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import gpu_util as GU  # noqa: E402
import line_stats_ref as R  # noqa: E402
from device_layouts import LAYOUTS, SENTINEL, Dev  # noqa: E402
from gt4py_amd import _lib  # noqa: E402
from gt4py_amd.cartesian.gtscript import IJ, IK, JK, PARALLEL, Field, computation, interval  # noqa: E402, F401

G = _lib.LINE_STATS_SEGMENT
HALO = 1
GUARD = 64  # doubles in front of and behind the workspace and the result
#: (line length, lines along the lower of the two other axes, lines along the higher): every length at which the order changes
#: shape (a short set, a full segment, one item more, an odd number of segments: a carried value), every count at which a wave or a
#: workgroup of lanes fills up
CASES = [(1, 257, 5), (2, 65, 2), (3, 64, 1), (4, 63, 2), (5, 1, 5), (G - 1, 65, 1), (G, 64, 2), (G + 1, 63, 5), (2 * G + 3, 257, 1),
         (3 * G, 1, 2), (5 * G + 1, 65, 2)]


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_device_memory():
    """The few hundred small buffers of this file go back to the driver when it is done (what runs behind it in the same
    process finds no block of this file's in the caching allocator)."""
    yield
    import torch

    torch.cuda.empty_cache()


def _domain(case, axis):
    n, lower, higher = case
    domain = [lower, higher]
    domain.insert(axis, n)
    return tuple(domain)


@functools.lru_cache(maxsize=None)
def _case(case, axis, dtype_name):
    """Data and the restatement's three results of a case (a field, a pair, a pair with an IJ weight): computed once, shared,
    read-only."""
    dtype = np.dtype(dtype_name).type
    domain = _domain(case, axis)
    rng = np.random.default_rng([*domain, axis, np.dtype(dtype_name).itemsize])
    a, b = GU.data(rng, domain, dtype), GU.data(rng, domain, dtype)
    w = rng.uniform(0.5, 2.0, domain[:2] + (1,)).astype(dtype)
    want = np.stack([R.lines(a, None, axis, G), R.lines(a, b, axis, G), R.lines(a, w, axis, G)])
    for x in (a, b, w, want):
        x.setflags(write=False)
    return a, b, w, want


def _dev(box, layout, align=0):
    """A sentinel buffer (tests/device_layouts.py) whose view holds `box` behind HALO points on every side (NaN there), in one of
    the four layouts or "strided": I-contiguous rows of which every other item belongs to the field.  Returns (Dev, the tensor the
    product is given)."""
    ni, nj, nk = box.shape
    strided = layout == "strided"
    shape = ((ni + 2 * HALO) * (2 if strided else 1) + 1, nj + 2 * HALO + 1, nk)
    values = np.full(shape, np.nan, dtype=box.dtype)
    step = 2 if strided else 1
    values[HALO * step:(HALO + ni) * step:step, HALO:HALO + nj] = box
    dev = Dev(shape, box.dtype, "ifirst" if strided else layout, values, align_i=align)
    return dev, (dev.given[::2] if strided else dev.given)


def _describe(t, origin, weight=False):
    size = t.element_size()
    shape = tuple(t.shape) + (1,) * (3 - t.dim())
    strides = tuple(s * size for s in t.stride()) + (0,) * (3 - t.dim())
    return _lib.Field.make(t.data_ptr(), shape, strides, tuple(0 if weight and s == 0 else o for o, s in zip(origin, strides)))


def _guarded(doubles):
    import torch

    buf = torch.empty(doubles + 2 * GUARD, dtype=torch.int64, device="cuda")
    buf.fill_(SENTINEL[8])
    return buf


def _run(tensors, others, domain, axis):
    """gt4mi_line_stats on the current stream with a workspace and a result inside sentinel buffers: the guards around both are
    unchanged afterwards.  Returns (the (n, 9, nB, nA) result, path, launches)."""
    import torch

    lib, n = _lib.load(), len(tensors)
    size = tensors[0].element_size()
    origin = (HALO, HALO, 0)
    fields = (_lib.Field * n)(*[_describe(t, origin) for t in tensors])
    seconds = (_lib.Field * n)()
    for k, o in enumerate(others):
        if o is not None:
            seconds[k] = _describe(o, origin, weight=True)
    needed, launches, path = ctypes.c_int64(), ctypes.c_int(), ctypes.c_int()
    args = (fields, seconds, n, _lib.domain3(domain), axis, size)
    tail = (ctypes.byref(needed), ctypes.byref(launches), ctypes.byref(path))
    _lib.check("gt4mi_line_stats", lib.gt4mi_line_stats(*args, None, 0, None, _lib.STATS_DRY_RUN, None, *tail))
    lines = int(np.prod(domain)) // domain[axis]
    assert needed.value == n * lines * R.segments(domain[axis], G) * 64
    work, result = _guarded(needed.value // 8), _guarded(n * 9 * lines)
    _lib.check("gt4mi_line_stats", lib.gt4mi_line_stats(*args, work.data_ptr() + 8 * GUARD, needed.value, result.data_ptr() + 8 * GUARD, 0,
                                                        GU.stream_ptr(), *tail))
    torch.cuda.synchronize()
    for name, buf in (("workspace", work), ("result", result)):
        guards = torch.cat([buf[:GUARD], buf[-GUARD:]]).cpu().numpy()
        assert (guards.view(np.uint64) == SENTINEL[8]).all(), f"the bytes around the {name} changed"
    rest = [d for d in range(3) if d != axis]
    got = result[GUARD:-GUARD].view(torch.float64).cpu().numpy().reshape(n, 9, domain[rest[1]], domain[rest[0]])
    return got, path.value, launches.value


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_every_row_bit_for_bit_on_every_path(axis, dtype):
    """A field, a pair and a pair whose second field is an IJ weight (K stride 0), in one call of three entries, in the four
    layouts and a strided one: every path is taken, the path is the one the strides call for, and every byte of the field
    buffers is what it was.  ("ifirst" with a halo of 1 and "ifirst_unaligned" put the line origin off a 16-byte boundary.)"""
    size = np.dtype(dtype).itemsize
    seen = set()
    for case in CASES:
        domain = _domain(case, axis)
        a, b, w, want = _case(case, axis, np.dtype(dtype).name)
        for layout in LAYOUTS + ["strided"]:
            devs, tensors = zip(*[_dev(x, layout) for x in (a, b, w)])
            weight = tensors[2][:, :, 0]  # Field[IJ] against Field[IJK]
            got, path, launches = _run([tensors[0]] * 3, [None, tensors[1], weight], domain, axis)
            strides = [tuple(s * size for s in tensors[0].stride())]
            seconds = [tuple(s * size for s in tensors[1].stride()), tuple(s * size for s in weight.stride()) + (0,)]
            assert path == R.expected_path(strides, seconds, domain, axis, size), (domain, layout, path)
            assert launches == 1 + (domain[axis] > G)
            seen.add(path)
            for k, what in enumerate(("field", "pair", "weight")):
                assert R.same_bits(got[k], want[k]), f"{domain} axis {axis} {dtype.__name__} {layout} {what} (path {path})"
            # along K the weight is broadcast along the line and keeps the call off the tiles: the field and the pair without it
            if R.expected_path(strides, seconds[:1], domain, axis, size) != path:
                got, path, _ = _run([tensors[0]] * 2, [None, tensors[1]], domain, axis)
                assert path == R.expected_path(strides, seconds[:1], domain, axis, size), (domain, layout, path)
                seen.add(path)
                assert R.same_bits(got, want[:2]), f"{domain} axis {axis} {dtype.__name__} {layout} without the weight (path {path})"
            for dev, what in zip(devs, ("a", "b", "w")):
                dev.assert_unchanged(f"{domain} {layout}: the buffer of {what}")
    assert seen == {R.LANES, R.TILES, R.ITEMS}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_bits_do_not_depend_on_layout_position_or_repetition(dtype):
    """Without the restatement: the same data I-, J- and K-contiguous and padded to an odd pitch, at two alignments, as entry
    0 of 1 and as entry 8 of 9 (two pass launches), called twice: one result, byte for byte, per axis."""
    from gt4py_amd import diagnostics

    rng = np.random.default_rng(7)
    domain = (2 * G + 3, 65, 3)
    a, b = GU.data(rng, domain, dtype), GU.data(rng, domain, dtype)
    fillers = [GU.wrap(GU.device(GU.data(rng, domain, dtype), "ifirst", HALO)) for _ in range(8)]
    for axis in "IJK":
        seen, paths = {}, set()
        for layout in LAYOUTS:
            for align in (HALO, HALO + 1):
                da, db = GU.wrap(GU.device(a, layout, HALO, align)), GU.wrap(GU.device(b, layout, HALO, align))
                alone = diagnostics.LineStats([da], axis=axis, others=[db], halo=HALO)
                segments = R.segments(domain["IJK".index(axis)], G)
                assert alone.launches == 1 + (segments > 1) and alone.domain == domain
                alone()
                first = alone.result.get().tobytes()
                alone()
                assert alone.result.get().tobytes() == first, f"{axis} {layout}: two calls differ"
                seen[layout, align, "alone"] = first
                paths.add(alone.path)
                if layout == "ifirst" and align == HALO:
                    nine = diagnostics.LineStats(fillers + [da], axis=axis, others=[None] * 8 + [db], halo=HALO)
                    assert nine.launches == 2 + (segments > 1)
                    nine()
                    seen["ninth of nine"] = nine.result.get()[8:].tobytes()
        assert len(set(seen.values())) == 1 and len(seen) == 9, f"{axis} {dtype.__name__}: {len(set(seen.values()))} different results"
        assert not np.isnan(np.frombuffer(first, dtype=np.float64)).any() and len(paths) == 2, paths  # LANES and TILES gave them


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_special_values(dtype):
    """Lines made wholly of NaN, of -0.0 and of +inf; one NaN, in one accumulator set of the second segment alone (the NaN rule
    across the joins); denormals; both zeros."""
    from gt4py_amd import diagnostics

    rng = np.random.default_rng(9)
    n = 2 * G + 3
    for axis in range(3):
        domain = _domain((n, 7, 2), axis)
        a = GU.data(rng, domain, dtype)
        lines = np.moveaxis(a, axis, 0)  # [m, lower, higher]: a view
        lines[:, 0, 0], lines[:, 1, 0], lines[:, 2, 0] = np.nan, -0.0, np.inf
        lines[G + 6, 3, 0] = np.nan  # item 6 of segment 1: set 2
        lines[:, 4, 0] = (rng.integers(-7, 8, n) * np.finfo(dtype).smallest_subnormal).astype(dtype)
        lines[:, 5, 0] = 0.0
        lines[::3, 5, 0] = -0.0
        want = R.lines(a, None, axis, G)
        for layout in ("ifirst", "kfirst", "jfirst"):
            p, = diagnostics.line_stats(GU.wrap(GU.device(a, layout, HALO)), axis=axis, halo=HALO)
            rows = np.array([getattr(p, name) for name in diagnostics.LINE_ROWS], dtype=np.float64)  # [row, lower, higher]
            assert R.same_bits(rows.transpose(0, 2, 1), want), (axis, layout)
        assert p.count.tolist() == [[n, n]] * 7 and p.nonfinite[:, 0].tolist() == [n, 0, n, 1, 0, 0, 0] and not p.nonfinite[:, 1].any()
        assert p.first_nonfinite == (0, 0) and p.all_finite[:, 0].tolist() == [False, True, False, False, True, True, True]
        for name in ("sum", "sum_abs", "sum_sq", "min", "max", "mean"):
            assert np.isnan(getattr(p, name)[:, 0]).tolist() == [True, False, False, True, False, False, False], name
        assert np.isnan(p.max_abs[3, 0]) and not np.isnan(p.dot).any()
        assert (p.min[1, 0], p.max[1, 0], p.sum[1, 0]) == (0, 0, 0) and np.signbit(p.min[1, 0]) and np.signbit(p.max[1, 0]) and not np.signbit(p.sum[1, 0])
        assert (p.min[2, 0], p.max[2, 0], p.sum[2, 0], p.mean[2, 0]) == (np.inf,) * 4
        assert p.nonfinite[4, 0] == 0 and p.sum_abs[4, 0] > 0 and abs(p.max[4, 0]) < np.finfo(dtype).tiny
        assert (p.min[5, 0], p.max[5, 0]) == (0, 0) and np.signbit(p.min[5, 0]) and not np.signbit(p.max[5, 0])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_order_free_slots_against_field_stats_of_every_line(dtype):
    """field_stats is verified on its own (tests/test_gpu_diagnostics.py): COUNT, NONFINITE, MIN and MAX of a line do not depend
    on the order and equal field_stats on that line's box exactly."""
    from gt4py_amd import diagnostics

    rng = np.random.default_rng(21)
    domain = (9, 5, 3)
    a, b = GU.data(rng, domain, dtype), GU.data(rng, domain, dtype)
    a[3, 4, 1], b[5, 2, 2], a[0, 0, 0], a[1, 0, 0] = np.inf, np.nan, 0.0, -0.0
    da, db = GU.wrap(GU.device(a, "ifirst", HALO)), GU.wrap(GU.device(b, "ifirst", HALO))
    for axis in range(3):
        single, pair = diagnostics.line_stats(da, da, axis=axis, other=[None, db], halo=HALO)
        rest = [d for d in range(3) if d != axis]
        for ia, ib in np.ndindex(domain[rest[0]], domain[rest[1]]):
            origin, box = [HALO, HALO, 0], [1, 1, 1]
            origin[rest[0]] += ia
            origin[rest[1]] += ib
            box[axis] = domain[axis]
            boxes = diagnostics.field_stats(da, da, other=[None, db], origin=origin, domain=box)
            for p, s in ((single, boxes[0]), (pair, boxes[1])):
                got = p[ia, ib]
                assert (got.count, got.nonfinite) == (s.count, s.nonfinite) and got.count == domain[axis], (axis, ia, ib)
                assert R.same_bits([got.min, got.max], [s.min, s.max]), (axis, ia, ib, got, s)
        assert single.nonfinite.sum() == 1 and pair.nonfinite.sum() == 2


def anomaly_jk(u: Field[np.float64], m: Field[JK, np.float64], out: Field[np.float64]):
    with computation(PARALLEL), interval(...):
        out = u - m


def anomaly_ik(u: Field[np.float64], m: Field[IK, np.float64], out: Field[np.float64]):
    with computation(PARALLEL), interval(...):
        out = u - m


def anomaly_ij(u: Field[np.float64], m: Field[IJ, np.float64], out: Field[np.float64]):
    with computation(PARALLEL), interval(...):
        out = u - m


@pytest.mark.parametrize("axis, definition", [("I", anomaly_jk), ("J", anomaly_ik), ("K", anomaly_ij)])
def test_section_feeds_a_stencil_in_the_same_stream_without_synchronisation(axis, definition):
    """ls() on a side stream, then out = u - m with m fed ls.section("mean") in the same stream, nothing in between: out is
    bit-equal to u minus the restatement's mean along the axis."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import diagnostics
    from gt4py_amd.cartesian import gtscript

    backend, domain = "hip:mi300", (G + 5, 33, 7)
    stencil = gtscript.stencil(backend=backend, definition=definition, device_sync=False)
    rng = np.random.default_rng(17)
    host = GU.data(rng, domain, np.float64) + 3.0
    u = gt_storage.from_array(host, backend=backend)
    out = gt_storage.zeros(domain, backend=backend)
    ls = diagnostics.LineStats([u], axis=axis)
    with pytest.raises(RuntimeError, match="not been called"):
        ls.get()
    ax = "IJK".index(axis)
    na, nb = (domain[d] for d in range(3) if d != ax)
    mean = ls.section("mean")
    assert mean.shape == (na, nb) and mean.dtype == np.float64 and mean.strides == (8, 8 * na)
    assert mean.ptr == ls.result.ptr + 8 * na * nb * 8 and ls.section("max", 0).ptr == ls.result.ptr + 6 * na * nb * 8
    with pytest.raises(ValueError, match="no section"):
        ls.section("median")
    with pytest.raises(IndexError):
        ls.section("mean", 1)
    stencil(u, mean, out)  # (compiled and loaded before the order matters)
    torch.cuda.synchronize()
    out.tensor.fill_(float("nan"))
    ls.result.tensor.fill_(float("nan"))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ls()
        stencil(u, mean, out)
    p, = ls.get()  # synchronises the stream both went to
    want = R.lines(host, None, ax, G)[R.MEAN].T  # [a, b]
    assert R.same_bits(p.mean, want) and R.same_bits(mean.get(), want)
    assert R.same_bits(out.get(), host - np.expand_dims(want, ax))


def test_a_dead_field_is_refused():
    import gt4py_amd.storage as gt_storage
    from gt4py_amd import diagnostics

    a, b = (gt_storage.from_array(np.ones((8, 6, 4)), backend="hip:mi300") for _ in range(2))
    both, alone = diagnostics.LineStats([a, b], axis="I"), diagnostics.LineStats([a], axis="K")
    both()
    del b
    gc.collect()
    with pytest.raises(RuntimeError, match="no longer exists"):
        both()
    alone()  # the other one still runs
    assert alone.get()[0].sum.tolist() == [[4.0] * 6] * 8
