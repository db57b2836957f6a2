"""The capture-and-replay protocol of tests/test_gpu_graph_replay.py and one case builder per frozen utility class.  A case owns
its device buffers (tests/device_layouts.py), three input images A, B, C from one seeded generator, and ``check(n)``: the
comparison with the class's numpy restatement exactly as the class's own GPU file makes it.  No arithmetic is written here.
Test infrastructure; torch and the product are imported when a case is built."""

from __future__ import annotations

import numpy as np

import device_layouts as L

MISSING = -999.25  # (tests/test_gpu_line_find.py's)


class Case:
    """``load(n)`` uploads image n into the input buffers, ``clear()`` writes the sentinel to every buffer the call writes,
    ``buffers()`` are the flat device tensors whose every byte a snapshot keeps (written buffers and results), ``check(n, what)``
    compares what the device holds with the restatement of image n.  ``records`` flattens ``obj.get()`` into arrays."""

    def __init__(self, obj, load, clear, buffers, check, records=None, keep=None):
        self.obj, self.load, self.clear, self.buffers, self.check, self.records, self.keep = obj, load, clear, buffers, check, records, keep
        self.get_synchronises_device = False


def _bytes(arrays):
    return [np.ascontiguousarray(a).tobytes() for a in arrays]


def snapshot(case):
    import torch

    torch.cuda.synchronize()
    return _bytes(t.cpu().numpy() for t in case.buffers())


def same(now, then, what):
    """Two snapshots are the same bytes; otherwise: which buffer, how many words differ and the first of them."""
    for k, (x, y) in enumerate(zip(now, then)):
        if x != y:
            a, b = (np.frombuffer(v, dtype=np.uint32) for v in (x, y))
            bad = np.flatnonzero(a != b)
            raise AssertionError(f"{what}: buffer {k}: {bad.size} of {a.size} 32-bit words differ, first at {bad[:6].tolist()}: "
                                 f"{a[bad[:6]].tolist()} and {b[bad[:6]].tolist()}")


def protocol(case, what):
    """Steps 1 to 6 of the issue: eager on A against the restatement; a capture that enqueues nothing; a replay on B against the
    restatement and, bit for bit over every written byte, against an eager call; replays on C and on A again, the last one bit for
    bit the first eager call; ``get()`` straight after a replay, on the default stream and on a side stream."""
    import torch

    obj = case.obj

    def fresh(n):
        case.load(n)
        case.clear()
        torch.cuda.synchronize()

    fresh(0)
    obj()
    torch.cuda.synchronize()
    case.check(0, f"{what}: eager on A")
    eager_a = snapshot(case)

    fresh(0)
    before = snapshot(case)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        obj()
    same(snapshot(case), before, f"{what}: the capture wrote to a buffer or a result")

    fresh(1)
    graph.replay()
    torch.cuda.synchronize()
    case.check(1, f"{what}: replay on B")
    replay_b = snapshot(case)
    records_b = None if case.records is None else _bytes(case.records(obj.get()))
    fresh(1)
    obj()
    same(snapshot(case), replay_b, f"{what}: replay and eager differ on B")

    fresh(2)
    graph.replay()
    torch.cuda.synchronize()
    case.check(2, f"{what}: replay on C")
    replay_c = snapshot(case)
    records_c = None if case.records is None else _bytes(case.records(obj.get()))
    assert replay_c != replay_b, f"{what}: B and C give the same bytes: the images do not tell a stale result from a new one"
    fresh(0)
    graph.replay()
    same(snapshot(case), eager_a, f"{what}: something survived from one replay to the next")

    if case.records is not None:
        # the device holds A's results; nothing below synchronises but get() itself
        fresh(1)
        graph.replay()
        got = _bytes(case.records(obj.get()))
        assert got == records_b, f"{what}: get() after a replay on the default stream is not the replay's"
        torch.cuda.synchronize()
        fresh(2)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            graph.replay()
            got = _bytes(case.records(obj.get()))
        assert got == records_c, f"{what}: get() after a replay on a side stream is not the replay's"
        torch.cuda.synchronize()
        # get() with ANOTHER stream current than the replay's: the documented order -- get() waits for the stream of the last direct
        # call and for the current one, so the replay's stream is synchronised first; Histogram.get() synchronises the device itself
        fresh(1)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            graph.replay()
        if not case.get_synchronises_device:
            side.synchronize()
        got = _bytes(case.records(obj.get()))
        assert got == records_b, f"{what}: get() on the default stream after a replay on a side stream is not the replay's"
        torch.cuda.synchronize()
    return graph


# ---- buffers ---------------------------------------------------------------------------------------------------------------------
def boxed(extent):
    """A box with one ghost cell in front of it on the low sides of I and J and one behind the array the product sees (what ``Dev``
    keeps from it comes on top): (shape, box, origin), as the line utilities' GPU files lay their cases out."""
    shape = (extent[0] + 2, extent[1] + 2, extent[2])
    return shape, (slice(1, 1 + extent[0]), slice(1, 1 + extent[1]), slice(None)), (1, 1, 0)


def put(dev, values):
    dev.host(dev.image)[...] = values
    dev.lay.upload(dev.image)


def mixed(rng, shape, dtype, f=0):
    """Mixed signs and magnitudes (almost every addition rounds), a few zeros of both signs: tests/test_gpu_line_scan.py's."""
    v = (rng.uniform(-1, 1, shape) * 10.0 ** rng.integers(-2, 3, shape) * 10.0 ** (f % 3)).astype(dtype)
    v[rng.uniform(0, 1, shape) < 0.02] = dtype(-0.0)
    return v


def plain(rng, shape, dtype, f=0):
    return (rng.uniform(-1, 1, shape) * 10.0 ** (f % 3)).astype(dtype)


def sparse_specials(rng, v, values=(np.nan, np.inf, -np.inf)):
    for value in values:  # (through indices: ``v`` may be a view of a box)
        v[np.unravel_index(rng.integers(0, v.size, max(1, v.size // 97)), v.shape)] = value
    return v


def fields_case(make, want, extent, dtype, *, layout="ifirst", src_layout=None, nfields=1, values=mixed, specials=(), dst_extent=None,
                seed=0, shared=()):
    """A class that writes ``nfields`` destinations from as many sources: ``make(dsts, srcs, origin)`` builds the frozen object from
    the tensors, ``want(box of a source, f)`` is the restatement's box of destination f.  Image B holds ``specials``.  ``shared``:
    what else the object reads and the case keeps alive, each with ``assert_unchanged``."""
    rng = np.random.default_rng([seed, *extent, np.dtype(dtype).itemsize])
    shape, box, origin = boxed(extent)
    d_shape, d_box, _ = boxed(dst_extent or extent)
    images = [[values(rng, shape, dtype, f) for f in range(nfields)] for _ in range(3)]
    if specials:
        for x in images[1]:
            sparse_specials(rng, x[box], specials)
    srcs = [L.Dev(shape, dtype, src_layout or layout, x, 1) for x in images[0]]
    dsts = [L.Dev(d_shape, dtype, layout, None, 1) for _ in range(nfields)]
    obj = make([d.given for d in dsts], [s.given for s in srcs], origin)
    wants = {}

    def load(n):
        for s, x in zip(srcs, images[n]):
            put(s, x)

    def clear():
        for d in dsts:
            d.lay.upload(d.image)

    def check(n, what):
        if n not in wants:  # (computed once per image)
            with np.errstate(all="ignore"):
                wants[n] = [want(x[box], f) for f, x in enumerate(images[n])]
        for f, d in enumerate(dsts):
            d.assert_box(d_box, wants[n][f], f"{what}: dst {f}")
        for f, s in enumerate(srcs):
            s.assert_unchanged(f"{what}: src {f}")
        for k, x in enumerate(shared):
            x.assert_unchanged(f"{what}: shared input {k}")

    return Case(obj, load, clear, lambda: [d.lay.flat for d in dsts], check, keep=(srcs, dsts, shared))


def readers_case(make, want, compare, records, extent, dtype, *, layouts=("ifirst",), values=mixed, specials=(), seed=0, shared=()):
    """A class that reads fields and owns its ``result``: ``make(tensors, origin, extent)`` builds it, ``want(boxes)`` is the
    restatement of the whole result, ``compare(got, want)`` the class's own comparator."""
    rng = np.random.default_rng([seed, *extent, np.dtype(dtype).itemsize])
    shape, box, origin = boxed(extent)
    images = [[values(rng, shape, dtype, f) for f in range(len(layouts))] for _ in range(3)]
    if specials:
        for x in images[1]:
            sparse_specials(rng, x[box], specials)
    devs = [L.Dev(shape, dtype, layout, x, 1) for layout, x in zip(layouts, images[0])]
    obj = make([d.given for d in devs], origin, extent)
    wants = {}

    def load(n):
        for d, x in zip(devs, images[n]):
            put(d, x)

    def check(n, what):
        if n not in wants:
            with np.errstate(all="ignore"):
                wants[n] = want([x[box] for x in images[n]])
        got = obj.result.tensor.cpu().numpy()
        assert got.size == wants[n].size, (what, got.shape, wants[n].shape)
        assert compare(got, wants[n].reshape(got.shape)), f"{what}: the result differs from the restatement"
        for f, d in enumerate(devs):
            d.assert_unchanged(f"{what}: field {f}")
        for k, x in enumerate(shared):
            x.assert_unchanged(f"{what}: shared input {k}")

    case = Case(obj, load, lambda: None, lambda: [obj.result.tensor], check, records, keep=(devs, shared))
    case.images = images
    return case


# ---- the classes -------------------------------------------------------------------------------------------------------------------
def halo_fill(dtype, layout, nfields, seed=0):
    """In place: the fields are inputs and written buffers at once.  Whole buffers as integers, as tests/test_gpu_boundary.py."""
    import boundary_ref as R
    from gt4py_amd import boundary

    itemsize = np.dtype(dtype).itemsize
    domain, widths, modes = (17, 33, 5), (2, 2, 2, 2), ("periodic", "zero_gradient")
    origin = (widths[0] + 1, widths[2] + 1, 0)  # one ghost cell beyond the widths: it must stay as it is
    shape = (origin[0] + domain[0] + widths[1] + 1, origin[1] + domain[1] + widths[3] + 1, domain[2])
    rng = np.random.default_rng([seed, nfields, itemsize])
    lays = [L.Layout(shape, layout, itemsize, origin[0]) for _ in range(nfields)]
    box = tuple(slice(o, o + d) for o, d in zip(origin, domain))
    images = []
    for _ in range(3):  # random BITS in the domain (NaNs with payloads, infinities and both zeros among them), the sentinel elsewhere
        per = []
        for lay in lays:
            host = L.sentinel_image(lay.flat.numel(), itemsize)
            lay.host_view(host)[box] = L.random_image(int(np.prod(domain)), itemsize, rng).reshape(domain)
            per.append(host)
        images.append(per)
    tf = _float_type(itemsize)
    given = [lay.view.view(tf) for lay in lays]
    obj = boundary.HaloFill(given, halo=((widths[0], widths[1]), (widths[2], widths[3])), mode=modes, origin=origin, domain=domain)

    def load(n):
        for lay, host in zip(lays, images[n]):
            lay.upload(host)

    def check(n, what):
        for f, (lay, host) in enumerate(zip(lays, images[n])):
            want = host.copy()
            R.fill(lay.host_view(want), origin, domain, widths, modes, 0, R.ALL)
            assert np.array_equal(lay.download(), want), f"{what}: field {f}: {int((lay.download() != want).sum())} items of the whole buffer differ"

    return Case(obj, load, lambda: None, lambda: [lay.flat for lay in lays], check, keep=given)


def _float_type(itemsize):
    import torch

    return {4: torch.float32, 8: torch.float64}[itemsize]


def field_copy(dtype, dst_layout, src_layout, npairs, extent=(17, 33, 5), seed=0, strided=False):
    """Whole destination buffers as integers against ``transfer_ref.copy_box``, as tests/test_gpu_transfer.py.  ``strided``: every
    other column of a wider source, which has no unit stride."""
    import transfer_ref as R
    from gt4py_amd import transfer

    itemsize = np.dtype(dtype).itemsize
    rng = np.random.default_rng([seed, npairs, itemsize, *extent])
    origin = (1, 1, 0)
    shape = (extent[0] + 2, extent[1] + 2, extent[2])
    s_shape = (2 * shape[0], shape[1], shape[2]) if strided else shape
    srcs = [L.Layout(s_shape, src_layout, itemsize, origin[0]) for _ in range(npairs)]
    dsts = [L.Layout(shape, dst_layout, itemsize, origin[0]) for _ in range(npairs)]
    images = [[L.random_image(s.flat.numel(), itemsize, rng) for s in srcs] for _ in range(3)]  # (random bits: every special value)
    sentinels = [L.sentinel_image(d.flat.numel(), itemsize) for d in dsts]
    s_views = [s.view[::2] if strided else s.view for s in srcs]
    d_views = [d.view for d in dsts]
    obj = transfer.FieldCopy(d_views, s_views, origin=origin, domain=extent)

    def load(n):
        for s, image in zip(srcs, images[n]):
            s.upload(image)

    def clear():
        for d, image in zip(dsts, sentinels):
            d.upload(image)

    def check(n, what):
        for f, (s, d) in enumerate(zip(srcs, dsts)):
            want = sentinels[f].copy()
            view = s.host_view(images[n][f])
            R.copy_box(d.host_view(want), view[::2] if strided else view, origin, origin, extent)
            assert np.array_equal(d.download(), want), f"{what}: pair {f}: items of the whole buffer differ"
            assert np.array_equal(s.download(), images[n][f]), f"{what}: source {f} changed"

    case = Case(obj, load, clear, lambda: [d.flat for d in dsts], check, keep=(s_views, d_views))
    case.expected_paths = [R.expected_path(d.strides, tuple(2 * x if strided and ax == 0 else x for ax, x in enumerate(s.strides)), extent)
                           for d, s in zip(dsts, srcs)]
    return case


def _stat_rows(records):
    from gt4py_amd.diagnostics import PROFILE_ROWS, Stats

    return [np.array(r, dtype=np.float64) if isinstance(r, Stats) else np.stack([getattr(r, name).astype(np.float64) for name in PROFILE_ROWS])
            for r in records]


def stats(kind, dtype, entries, *, extent=(65, 63, 7), layouts=("ifirst", "ifirst"), axis=0, seed=0):
    """``FieldStats`` / ``LevelStats`` / ``LineStats`` of ``entries`` entries over two fields a and b: entry 0 is a alone, every
    other one the pair (a, b).  Bit for bit against the restatement with the file's own ``same_bits``."""
    import level_stats_ref
    import line_stats_ref
    import stats_ref
    from gt4py_amd import _lib, diagnostics

    others = [None] + [1] * (entries - 1)
    if kind == "field":
        R, one = stats_ref, stats_ref.stats
    elif kind == "level":
        R, one = level_stats_ref, level_stats_ref.profile
    else:
        R, one = line_stats_ref, lambda a, b=None: line_stats_ref.lines(a, b, axis, _lib.LINE_STATS_SEGMENT)

    def make(tensors, origin, extent):
        a, b = tensors
        kwargs = dict(others=[None if o is None else b for o in others], origin=origin, domain=extent)
        if kind == "field":
            return diagnostics.FieldStats([a] * entries, **kwargs)
        if kind == "level":
            return diagnostics.LevelStats([a] * entries, **kwargs)
        return diagnostics.LineStats([a] * entries, axis=axis, **kwargs)

    def want(boxes):
        alone, pair = one(boxes[0]), one(boxes[0], boxes[1])
        return np.stack([alone if o is None else pair for o in others])

    from gpu_util import data

    def values(rng, shape, dtype, f=0):  # NaN around the box, as the statistics' own files have it: a read outside turns the result NaN
        v = np.full(shape, np.nan, dtype=dtype)
        v[1:-1, 1:-1] = data(rng, (shape[0] - 2, shape[1] - 2, shape[2]), dtype)
        return v

    return readers_case(make, want, R.same_bits, _stat_rows, extent, dtype, layouts=layouts, seed=seed, values=values,
                        specials=(np.nan, np.inf, -np.inf))


def _same_or_both_nan(got, want):
    """tests/test_gpu_line_find.py's comparison of a result block."""
    want = np.ascontiguousarray(want)
    return bool(((got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))).all())


def _walk(axis):
    def values(rng, shape, dtype, f=0):  # tests/test_gpu_line_find.py's random walk around the levels 0.125 f
        v = np.cumsum(rng.uniform(-0.3, 0.3, shape), axis=axis) + rng.uniform(-0.6, 0.6, shape).take([0], axis=axis) + 0.125 * f
        return v.astype(dtype)

    return values


def line_find(dtype, axis, layout, nfields, extent, *, what="crossing", levels=None, seed=0):
    import line_find_ref as R
    from gt4py_amd import linefind

    if what == "crossing" and levels is None:
        levels = [0.125 * f for f in range(nfields)]

    def make(tensors, origin, extent):
        return linefind.LineFind(tensors, axis="IJK"[axis], what=what, level=levels, missing=MISSING, origin=origin)

    def want_with(levels):
        def want(boxes):
            return np.stack([R.find_along(x, axis, what, None if levels is None else levels[f], "any", False, None, MISSING).transpose(0, 2, 1)
                             for f, x in enumerate(boxes)])
        return want

    def records(found):
        return [a for r in found for a in (r.position, r.coord, r.crossings if r.value is None else r.value)]

    case = readers_case(make, want_with(levels), _same_or_both_nan, records, extent, dtype, layouts=(layout,) * nfields, values=_walk(axis),
                        specials=(np.nan,), seed=seed)
    case.want_with = want_with
    return case


def histogram(dtype, layout, nb, by, *, accumulate=False, extent=(65, 7, 5), nfields=2, seed=0):
    """Counters compared as integers against ``histogram_ref.count_box``; values as tests/test_gpu_histogram.py draws them: mostly
    inside the edges, some beyond either end, NaN and infinities, items on the outer edges -- in every image."""
    import histogram_ref as R
    from gt4py_amd import histogram as product

    e = np.linspace(-2.0, 3.0, nb + 1)

    def values(rng, shape, dtype, f=0):
        lo, hi = -2.0, 3.0
        v = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo), shape)
        return sparse_specials(rng, v, (np.nan, np.inf, -np.inf, lo, hi)).astype(dtype)

    def make(tensors, origin, extent):
        return product.Histogram(tensors, edges=e, by=by, accumulate=accumulate, origin=origin, domain=extent)

    def want(boxes):
        return np.stack([R.count_box(x, e, by == "K") for x in boxes])

    def records(hists):
        return [np.asarray(a) for h in hists for a in (h.counts, h.below, h.above, h.nan)]

    case = readers_case(make, want, lambda got, w: got.tobytes() == w.tobytes(), records, extent, dtype, layouts=(layout,) * nfields,
                        values=values, seed=seed)
    case.get_synchronises_device = True
    if accumulate:  # a call ADDS: the protocol clears the result as a caller does, with reset() in stream order
        case.clear = case.obj.reset
    return case


def line_scan(dtype, axis, layout, src_layout, nfields, extent, seed=0):
    import line_scan_ref as R
    from gt4py_amd import linescan

    return fields_case(lambda d, s, origin: linescan.LineScan(d, s, axis="IJK"[axis], op="sum", origin=origin),
                       lambda x, f: R.scan_along(x, axis, "sum", False, False, None, False), extent, dtype, layout=layout, src_layout=src_layout,
                       nfields=nfields, specials=(np.nan, np.inf, -np.inf), seed=seed)


def line_solve(dtype, axis, layout, src_layout, nfields, extent, periodic=False, seed=0):
    """1-d coefficients that every line shares (diagonally dominant, tests/test_gpu_line_solve.py's), the right-hand sides change
    from image to image."""
    import line_solve_ref as R
    from gt4py_amd import linesolve

    rng = np.random.default_rng([seed, 3])
    n = extent[axis]
    a, c = rng.uniform(-1, 1, n), rng.uniform(-1, 1, n)
    b = (2.0 * (np.abs(a) + np.abs(c)) + rng.uniform(0.1, 1, n)) * rng.choice([-1.0, 1.0], n)
    coefs = [v.astype(dtype) for v in (a, b, c)]
    lines = [L.Line(v) for v in coefs]
    return fields_case(lambda d, s, origin: linesolve.LineSolve(d, s, lower=lines[0].given, diag=lines[1].given, upper=lines[2].given,
                                                                axis="IJK"[axis], periodic=periodic, origin=origin),
                       lambda x, f: R.solve_along(*coefs, x, axis, periodic), extent, dtype, layout=layout, src_layout=src_layout,
                       nfields=nfields, values=plain, seed=seed, shared=lines)


def _response(n, seed):
    import torch

    rng = np.random.default_rng([seed, n, 1])
    r = rng.uniform(0, 1, n // 2 + 1)
    r[rng.uniform(0, 1, r.shape) < 0.2] = 0.0
    r[0] = 1.0
    return r, torch.from_numpy(r).cuda()


def line_filter(dtype, axis, layout, src_layout, nfields, extent, seed=0):
    import line_filter_ref as R
    from gt4py_amd import linefilter

    r, d_r = _response(extent[axis], seed)

    def want(x, f):
        return np.ascontiguousarray(np.moveaxis(R.filter(np.ascontiguousarray(np.moveaxis(x, axis, 0)), r.reshape(-1, 1, 1)), 0, axis))

    case = fields_case(lambda d, s, origin: linefilter.LineFilter(d, s, axis="IJK"[axis], response=d_r, origin=origin), want, extent, dtype,
                       layout=layout, src_layout=src_layout, nfields=nfields, seed=seed)
    case.keep += (d_r,)
    return case


def line_spectrum(dtype, axis, layout, nfields, extent, seed=0):
    import line_filter_ref as R
    from gt4py_amd import linefilter

    def want(boxes):  # (2, nh, ea, eb) of the restatement -> (2, ea, eb, nh)
        return np.stack([np.moveaxis(np.stack(R.spectrum(np.ascontiguousarray(np.moveaxis(x, axis, 0)))), 1, 3) for x in boxes])

    return readers_case(lambda tensors, origin, extent: linefilter.LineSpectrum(tensors, axis="IJK"[axis], origin=origin), want,
                        lambda got, w: bool(R.same_bits(got, w).all()), lambda c: [c.real, c.imag], extent, dtype, layouts=(layout,) * nfields,
                        seed=seed)


def vertical_remap(dtype, layout, nfields, seed=0):
    """``Field[K]`` edges that every column shares; the outer edges coincide."""
    import vertical_remap_ref as V
    from gt4py_amd import vertical

    ns, nd, method = 7, 5, "plm"
    rng = np.random.default_rng([seed, 11])
    zs = np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 2, ns))])
    zd = np.concatenate([[0.0], np.sort(rng.uniform(0.1, zs[-1] - 0.1, nd - 1)), [zs[-1]]])
    lines = [L.Line(zs), L.Line(zd)]
    return fields_case(lambda d, s, origin: vertical.VerticalRemap(d, s, src_edges=lines[0].given, dst_edges=lines[1].given, method=method,
                                                                   origin=origin),
                       lambda x, f: V.remap_as(x, zs, zd, method), (17, 33, ns), dtype, layout=layout, nfields=nfields, values=plain,
                       dst_extent=(17, 33, nd), seed=seed, shared=lines)


def vertical_interp(dtype, layout, nfields, seed=0):
    """``Field[K]`` coordinates that every column shares; targets in any order, some outside the source range (``outside="fill"``)."""
    import vertical_interp_ref as V
    from gt4py_amd import vertical

    ns, nd, method = 7, 6, "cubic_monotone"
    rng = np.random.default_rng([seed, 12])
    z = np.cumsum(rng.uniform(0.5, 2, ns))
    x = rng.permutation(np.concatenate([[z[0] - 1.0, z[-1] + 1.0], rng.uniform(z[0], z[-1], nd - 2)]))
    lines = [L.Line(z), L.Line(x)]
    return fields_case(lambda d, s, origin: vertical.VerticalInterp(d, s, src_coord=lines[0].given, dst_coord=lines[1].given, method=method,
                                                                    outside="fill", fill_value=-1.5, origin=origin),
                       lambda q, f: V.interp(q, z, x, method, V.FILL, -1.5), (17, 33, ns), dtype, layout=layout, nfields=nfields, values=plain,
                       dst_extent=(17, 33, nd), seed=seed, shared=lines)


def _positions(rng, extent, ndim):
    """Absolute positions inside and a little beyond the domain (those are clamped), as float64 IJK fields in the cases' buffers."""
    shape, box, _ = boxed(extent)
    out = []
    for ax in range(ndim):
        full = np.full(shape, 7.25)
        full[box] = rng.uniform(-1.5, extent[ax] + 0.5, extent)
        out.append(full)
    return out, box


def horizontal_interp(dtype, layout, nfields, seed=0):
    import horizontal_interp_ref as H
    from gt4py_amd import horizontal

    extent, method = (17, 33, 5), "cubic"
    fulls, box = _positions(np.random.default_rng([seed, 13]), extent, 2)
    pos = [L.Dev(p.shape, np.float64, layout, p, 1) for p in fulls]
    return fields_case(lambda d, s, origin: horizontal.HorizontalInterp(d, s, pos_i=pos[0].given, pos_j=pos[1].given, method=method, origin=origin),
                       lambda q, f: H.interp(q, fulls[0][box], fulls[1][box], method, False, (0, 0, 0, 0)), extent, dtype, layout=layout,
                       nfields=nfields, values=plain, seed=seed, shared=pos)


def departure_interp(dtype, layout, nfields, seed=0):
    import departure_interp_ref as D
    from gt4py_amd import departure

    extent, method = (17, 33, 5), "linear"
    fulls, box = _positions(np.random.default_rng([seed, 14]), extent, 3)
    pos = [L.Dev(p.shape, np.float64, layout, p, 1) for p in fulls]
    return fields_case(lambda d, s, origin: departure.DepartureInterp(d, s, pos_i=pos[0].given, pos_j=pos[1].given, pos_k=pos[2].given,
                                                                      method=method, origin=origin),
                       lambda q, f: D.interp3(q, fulls[0][box], fulls[1][box], fulls[2][box], method, False, (0, 0, 0, 0)), extent, dtype,
                       layout=layout, nfields=nfields, values=plain, seed=seed, shared=pos)


def horizontal_remap(dtype, layout, nfields, seed=0):
    """Two rectilinear grids with the same outer edges; the boxes start at (1, 1, 0) of fields with a ghost cell around them."""
    import horizontal_remap_ref as R
    from gt4py_amd import horizontal

    ns, nd, nk, method = (17, 12), (9, 14), 3, "plm"
    rng = np.random.default_rng([seed, 15])
    xs = [np.concatenate([[0.0], np.cumsum(rng.uniform(0.5, 2, n))]) for n in ns]
    xd = [np.concatenate([[0.0], np.sort(rng.uniform(0.1, s[-1] - 0.1, n - 1)), [s[-1]]]) for n, s in zip(nd, xs)]
    return fields_case(lambda d, s, origin: horizontal.HorizontalRemap(d, s, src_edges=tuple(xs), dst_edges=tuple(xd), method=method,
                                                                       src_origin=origin, dst_origin=origin),
                       lambda q, f: R.remap_as(q, tuple(xs), tuple(xd), method), ns + (nk,), dtype, layout=layout, nfields=nfields, values=plain,
                       dst_extent=nd + (nk,), seed=seed)


def sample(dtype, layout, nfields, point_mode, seed=0):
    """Column mode ``(nf, npoints, nk)`` or point mode ``(nf, npoints)`` at fixed positions; the fields change from image to image."""
    import torch

    import point_sample_ref as S
    from gt4py_amd import sampling

    extent, method, npoints = (17, 33, 5), "linear", 70
    rng = np.random.default_rng([seed, 16])
    p = [rng.uniform(-0.5, extent[ax] - 0.5, npoints) for ax in range(3 if point_mode else 2)]
    d_p = [torch.from_numpy(x).cuda() for x in p]

    def make(tensors, origin, extent):
        return sampling.Sample(tensors, pos_i=d_p[0], pos_j=d_p[1], pos_k=d_p[2] if point_mode else None, method=method, origin=origin)

    def want(boxes):
        return np.stack([S.sample(x, p[0], p[1], p[2] if point_mode else None, method) for x in boxes])

    case = readers_case(make, want, lambda got, w: bool(S.same_bits(got, w).all()), lambda a: [a], extent, dtype, layouts=(layout,) * nfields,
                        values=plain, seed=seed)
    case.keep += (d_p,)
    return case
