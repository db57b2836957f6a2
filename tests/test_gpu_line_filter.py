"""``gt4py_amd.linefilter`` on the GPU: against the contract's restatement (tests/line_filter_ref.py) over EVERY byte of every dst
buffer and of the spectrum's result, compared as integers -- row padding, ghost cells outside the box and the allocation's slack keep
a NaN-payload sentinel (or, in place, the source); inside the box a NaN counts as a NaN.  Every input, the response included, must
come back unchanged.

The lengths go from 2 over one wave (64) to the longest line (4096): one, two and three fused stages alone (2, 4, 8), a remainder
pass of one and of two stages in front of the threes (16, 32, 128, 256, 1024), threes only (64, 4096), the tile of 2048 points and the
one of 4096.  1, 63, 64, 65 and 257 lines cover one live lane, a partial wave, a full one, a wave plus one and several workgroups;
(16, (1, 1)) is a box that is ONE line.  Every length has a line count of its own, so that the product stays small.  The lines of a
case are made once, with the line axis first, and laid along I, J and K: every axis, layout and path is held against ONE reference."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import device_layouts as L  # noqa: E402  (the layouts; test infrastructure)
import line_filter_ref as R  # noqa: E402

LANES, TILES, ITEMS = "lanes", "tiles", "items"
#: (line length, the extents of the two other axes)
CASES = [(2, (64, 1)), (4, (65, 2)), (8, (5, 3)), (16, (63, 1)), (32, (257, 1)), (64, (3, 2)), (128, (3, 2)), (256, (2, 1)),
         (1024, (2, 1)), (4096, (1, 1)), (16, (1, 1))]
AXES = "IJK"
#: per path and line axis: (the layout of dst, the layout of src) that selects it
LAYOUTS = {TILES: [("ifirst", None), ("jfirst", None), ("kfirst", None)],
           LANES: [("kfirst", None), ("ifirst", None), ("ifirst", None)],
           ITEMS: [("ifirst", "kfirst"), ("kfirst", "ifirst"), ("jfirst", "ifirst")]}
FORMS = ("shared", "full", "a", "b")  # the response: (nh,), (ea, eb, nh), (ea, 1, nh), (1, eb, nh)


def _shape(n, others, axis):
    shape = list(others)
    shape.insert(axis, n)
    return tuple(shape)


def expected_path(strides, form, extent, axis):
    """The rule of include/gt4py_amd.h restated: strides in ITEMS of every field; the response (None: a spectrum) allows another axis
    only where it is broadcast along it."""
    others = [a for a in range(3) if a != axis]
    free = {None: (True, True), "shared": (True, True), "full": (False, False), "a": (False, True), "b": (True, False)}[form]

    def unit(ax):
        return all(s[ax] == 1 for s in strides) and (ax == axis or free[others.index(ax)])

    if unit(axis) and extent[axis] > 1:
        return TILES
    return LANES if any(unit(ax) and extent[ax] > 1 for ax in others) else ITEMS


_REFERENCE = {}


def _lines(n, others, dtype, nfields, form, seed):
    """The lines of a case with the line axis first, per field, the response (nh, ea or 1, eb or 1) and the restatement's results:
    made once per case and never changed."""
    key = (n, others, np.dtype(dtype).name, nfields, form, seed)
    if key not in _REFERENCE:
        rng = np.random.default_rng([seed, n, *others])
        shape = (n,) + tuple(others)
        xs = []
        for f in range(nfields):
            v = (rng.uniform(-1, 1, shape) * 10.0 ** rng.integers(-2, 3, shape) * 10.0 ** (f % 3)).astype(dtype)
            v[rng.uniform(0, 1, shape) < 0.02] = dtype(-0.0)
            xs.append(v)
        rshape = {"shared": (1, 1), "full": others, "a": (others[0], 1), "b": (1, others[1])}[form]
        rrng = np.random.default_rng([seed, n, *others, 1])  # (the response does not depend on how many fields there are)
        r = rrng.uniform(0, 1, (n // 2 + 1,) + tuple(rshape))
        r[rrng.uniform(0, 1, r.shape) < 0.2] = 0.0
        r[0] = 1.0
        for a in [*xs, r]:
            a.setflags(write=False)
        _REFERENCE[key] = (xs, r, [R.filter(x, r) for x in xs], [np.stack(R.spectrum(x)) for x in xs])
    return _REFERENCE[key]


def _along(lines_first, axis):
    return np.ascontiguousarray(np.moveaxis(lines_first, 0, axis))


def _run(n, others, axis, *, dtype=np.float64, layout="ifirst", src_layout=None, nfields=1, inplace=False, form="shared", halo=0, k0=0,
         seed=0, plant=None, want_path=None, spectrum=True):
    """One call through ``linefilter.LineFilter`` (and one through ``LineSpectrum`` on the same sources); every dst buffer and the
    spectrum's result are compared whole against the restatement, every input must come back unchanged.  Returns the filtered boxes
    with the line axis first, and the LineFilter."""
    import torch

    from gt4py_amd import linefilter

    extent = _shape(n, others, axis)
    xs, r, want, want_spectrum = _lines(n, others, dtype, nfields, form, seed)
    if plant is not None:
        xs = [x.copy() for x in xs]
        plant(xs)
        with np.errstate(all="ignore"):
            want, want_spectrum = [R.filter(x, r) for x in xs], [np.stack(R.spectrum(x)) for x in xs]
    # one ghost cell in front of the box on the low sides of I and J, one behind the array the product sees, k0 levels below
    shape = (extent[0] + 2, extent[1] + 2, extent[2] + k0)
    box = (slice(1, 1 + extent[0]), slice(1, 1 + extent[1]), slice(k0, None))
    origin = (1 + halo, 1 + halo, k0)
    rng = np.random.default_rng([seed, 7])
    fulls = []
    for x in xs:
        full = rng.uniform(-1, 1, shape).astype(dtype)
        full[box] = _along(x, axis)
        fulls.append(full)
    # the response as the product takes it: (nh,) or (ea, eb, nh), C-ordered
    r_host = np.array(r[:, 0, 0] if form == "shared" else np.moveaxis(r, 0, 2), order="C")
    d_r = torch.from_numpy(r_host).cuda()
    src_layout = src_layout or layout
    if inplace:
        dsts = srcs = [L.Dev(shape, dtype, layout, x, 1) for x in fulls]
    else:
        srcs = [L.Dev(shape, dtype, src_layout, x, 1) for x in fulls]
        dsts = [L.Dev(shape, dtype, layout, None, 1) for _ in fulls]
    what = f"axis {AXES[axis]} extent {extent} {np.dtype(dtype)} {layout}/{src_layout} {nfields} field(s) inplace {inplace} response {form}"
    strides = [d.lay.strides for d in dsts] + [s.lay.strides for s in srcs]
    if spectrum:  # (first: an in-place filter overwrites the sources)
        sp = linefilter.LineSpectrum([s.given for s in srcs], axis=AXES[axis], halo=halo, origin=origin)
        assert (sp.n, sp.lines, sp.extent, sp.launches) == (n, others[0] * others[1], extent, -(-nfields // 8))
        assert sp.path == expected_path([s.lay.strides for s in srcs], None, extent, axis), (what, sp.path)
        assert sp.result.shape == (nfields, 2, others[0], others[1], n // 2 + 1)
        sp.result.tensor.copy_(torch.full_like(sp.result.tensor, 7.5))  # (a call overwrites every item)
        sp()
        torch.cuda.synchronize()
        got = sp.result.tensor.cpu().numpy()
        for f in range(nfields):
            rows = np.moveaxis(want_spectrum[f], 1, 3)  # (2, nh, ea, eb) -> (2, ea, eb, nh)
            assert R.same_bits(got[f], rows).all(), f"{what} {sp.path}: spectrum of field {f}: {int((~R.same_bits(got[f], rows)).sum())} items differ"
        c = sp.get()
        assert c.dtype == np.complex128 and R.same_bits(c.real, got[:, 0]).all() and R.same_bits(c.imag, got[:, 1]).all()
        for f, s in enumerate(srcs):
            s.assert_unchanged(f"{what}: src {f} after the spectrum")
    lf = linefilter.LineFilter([d.given for d in dsts], [s.given for s in srcs], axis=AXES[axis], response=d_r, halo=halo, origin=origin)
    assert (lf.n, lf.lines, lf.extent, lf.launches) == (n, others[0] * others[1], extent, -(-nfields // 8))
    if want_path is None:
        want_path = expected_path(strides, form, extent, axis)
    assert lf.path == want_path, (what, lf.path, want_path)
    lf()
    what += f" {lf.path}"
    got = []
    for f, d in enumerate(dsts):
        got.append(np.moveaxis(d.assert_box(box, _along(want[f], axis), f"{what}: dst {f}"), axis, 0))
    if not inplace:
        for f, s in enumerate(srcs):
            s.assert_unchanged(f"{what}: src {f}")
    assert np.array_equal(d_r.cpu().numpy().view(np.uint64), r_host.view(np.uint64)), f"{what}: the response changed"
    return got, lf


@pytest.mark.parametrize("path", [TILES, LANES, ITEMS])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_every_length_and_line_count_on_each_path(axis, path):
    layout, src_layout = LAYOUTS[path][axis]
    for n, others in CASES:
        for dtype in (np.float32, np.float64):
            _, lf = _run(n, others, axis, dtype=dtype, layout=layout, src_layout=src_layout, seed=1)  # (the path is checked against the rule)
            if path != LANES or max(others) > 1:  # (a box that is one line has no other axis to run lanes along)
                assert lf.path == path, (n, others, lf.path)


def test_rows_that_start_on_odd_addresses_take_the_item_lanes_of_tiles():
    """``ifirst`` rows start on 256-byte boundaries and take 16-byte lanes; ``ifirst_unaligned`` rows start anywhere."""
    for n, others in ((2, (64, 1)), (8, (5, 3)), (64, (3, 2)), (256, (2, 1))):
        for dtype in (np.float32, np.float64):
            _, lf = _run(n, others, 0, dtype=dtype, layout="ifirst_unaligned", nfields=2, seed=1)
            assert lf.path == TILES
    for axis in (1, 2):
        _, lf = _run(32, (9, 3), axis, dtype=np.float32, layout="ifirst_unaligned", nfields=2, seed=2)
        assert lf.path == LANES


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_in_place_mixed_layouts_eight_and_nine_fields_a_halo_and_an_origin_off_zero(axis):
    out, _ = _run(32, (9, 3), axis, dtype=np.float32, layout="ifirst", nfields=2, seed=3)
    for layout in ("ifirst", "kfirst", "jfirst"):
        inp, _ = _run(32, (9, 3), axis, dtype=np.float32, layout=layout, nfields=2, inplace=True, seed=3)
        for x, y in zip(out, inp):
            assert R.same_bits(x, y).all(), layout
    _run(128, (3, 2), axis, dtype=np.float64, layout="kfirst", nfields=2, inplace=True, seed=3)
    _run(32, (9, 3), axis, dtype=np.float64, layout="ifirst", src_layout="kfirst", nfields=2, seed=3, want_path=ITEMS)
    # 9 pairs are two launches; a field has the same bits at every position and in every company
    nine, lf = _run(16, (5, 3), axis, dtype=np.float32, nfields=9, seed=4)
    assert lf.launches == 2
    for count in (8, 4, 1):
        some, _ = _run(16, (5, 3), axis, dtype=np.float32, nfields=count, seed=4, inplace=count == 8)
        for f in range(count):
            assert R.same_bits(some[f], nine[f]).all(), (count, f)
    _run(64, (3, 2), axis, dtype=np.float64, layout="kfirst", nfields=9, inplace=True, seed=4)
    _run(64, (3, 2), axis, dtype=np.float64, layout="ifirst", nfields=8, seed=4)
    # the box is the domain grown by a halo of 2 in I and J and starts at level 1
    for layout in ("jfirst", "ifirst_unaligned"):
        _run(16, (8, 8), axis, dtype=np.float64, layout=layout, nfields=2, halo=2, k0=1, seed=5)
        _run(16, (8, 8), axis, dtype=np.float32, layout=layout, nfields=2, inplace=True, halo=2, k0=1, seed=5)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_every_form_of_the_response_and_a_response_rewritten_between_two_calls(axis):
    import torch

    for form in FORMS:
        for layout in ("ifirst", "kfirst"):
            _run(16, (9, 5), axis, dtype=np.float32, layout=layout, nfields=2, form=form, seed=6, spectrum=False)
            _run(64, (3, 2), axis, dtype=np.float64, layout=layout, form=form, seed=6, spectrum=False)
    # the frozen object reads the response when the kernel runs
    from gt4py_amd import linefilter

    n, others = 32, (9, 3)
    xs, r, want, _ = _lines(n, others, np.float64, 1, "a", 7)
    x = torch.from_numpy(np.array(_along(xs[0], axis))).cuda()  # (a writable copy: the case's lines are read-only)
    out = torch.zeros_like(x)
    d_r = torch.from_numpy(np.ascontiguousarray(np.moveaxis(r, 0, 2))).cuda()
    lf = linefilter.LineFilter(out, x, axis=AXES[axis], response=d_r)
    lf()
    assert R.same_bits(out.cpu().numpy(), _along(want[0], axis)).all()
    other = np.linspace(1.0, 0.0, n // 2 + 1).reshape(-1, 1, 1) * np.ones((1, others[0], 1))
    d_r.copy_(torch.from_numpy(np.ascontiguousarray(np.moveaxis(other, 0, 2))))
    lf()
    got = out.cpu().numpy()
    assert R.same_bits(got, _along(R.filter(xs[0], other), axis)).all() and not R.same_bits(got, _along(want[0], axis)).all()
    # the one-shot forms
    linefilter.filter_lines(out, x, axis=AXES[axis], response=d_r)
    assert R.same_bits(out.cpu().numpy(), got).all()
    c = linefilter.spectrum_lines(x, axis=AXES[axis])
    re, im = R.spectrum(xs[0])
    assert c.dtype == np.complex128 and c.shape == (1, others[0], others[1], n // 2 + 1)
    assert R.same_bits(c[0].real, np.moveaxis(re, 0, 2)).all() and R.same_bits(c[0].imag, np.moveaxis(im, 0, 2)).all()
    sp = linefilter.LineSpectrum([x], axis=AXES[axis])
    sp()
    assert np.array_equal(sp.power(), R.power(c, n))


@pytest.mark.parametrize("layout", ["ifirst", "kfirst"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_nan_and_an_inf_stay_in_their_lines(axis, layout):
    n, others = 64, (65, 2)
    spots = [((20, 64, 0), np.nan), ((5, 3, 1), np.inf)]  # (point on the line, the line's two other indices)

    def plant(xs):
        for point, v in spots:
            xs[0][point] = v

    for dtype in (np.float32, np.float64):
        clean, _ = _run(n, others, axis, dtype=dtype, layout=layout, nfields=2, seed=8)
        dirty, _ = _run(n, others, axis, dtype=dtype, layout=layout, nfields=2, seed=8, plant=plant)
        touched = np.zeros((n,) + others, dtype=bool)
        for point, _v in spots:
            touched[(slice(None),) + point[1:]] = True
        assert R.same_bits(clean[0][~touched], dirty[0][~touched]).all() and np.isfinite(dirty[0][~touched]).all()
        assert not np.isfinite(dirty[0][touched]).any()
        assert R.same_bits(clean[1], dirty[1]).all()  # the other field of the launch


def test_the_same_lines_through_every_path_and_axis_give_the_same_bits():
    for dtype in (np.float32, np.float64):
        seen, paths = [], set()
        for axis in range(3):
            for layout, src_layout in (("ifirst", None), ("kfirst", None), ("jfirst", None), ("ifirst", "kfirst")):
                got, lf = _run(128, (5, 3), axis, dtype=dtype, layout=layout, src_layout=src_layout, seed=9, spectrum=False)
                paths.add((axis, lf.path))
                seen.append(got[0])
        assert paths == {(axis, path) for axis in range(3) for path in (LANES, TILES, ITEMS)}
        for other in seen[1:]:
            assert R.same_bits(seen[0], other).all()


def test_hand_over_from_and_to_stencils_in_stream_order():
    """A device_sync=False stencil writes the field, LineFilter damps it along I in place with one response per latitude, a
    device_sync=False stencil reads it; nothing in between.  Compared with the restatement on the host."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import linefilter
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates
    from oracle import ref_numpy as ORACLE  # (oracle = checker only)

    backend, (ni, nj, nk) = "hip:mi300", (64, 12, 3)
    rng = np.random.default_rng(10)
    u = rng.uniform(-1, 1, (ni + 2, nj + 2, nk))
    lap = gtscript.stencil(backend=backend, definition=hip_templates.lap_notebook, dtypes={"T": np.float64}, device_sync=False)
    d_u = gt_storage.from_array(u, backend=backend, aligned_index=(1, 1, 0))
    d_mid, d_out = (gt_storage.zeros((ni + 2, nj + 2, nk), backend=backend, aligned_index=(1, 1, 0)) for _ in range(2))
    damping = rng.uniform(0, 1, (nj, 1, ni // 2 + 1))
    d_r = torch.from_numpy(damping).cuda()
    inner = d_mid[1:-1, 1:-1]  # the periodic lines are the domain's, without the ghost cells: 64 points along I
    polar = linefilter.LineFilter(inner, inner, axis="I", response=d_r)
    assert polar.extent == (ni, nj, nk) and polar.path == TILES
    for _ in range(2):
        lap(d_u, d_mid, origin=(1, 1, 0), domain=(ni, nj, nk))
        polar()
        lap(d_mid, d_out, origin=(1, 1, 0), domain=(ni, nj, nk))  # (the ring of d_mid stays zero: the filter's box is the domain)
    torch.cuda.synchronize()
    mid = np.zeros_like(u)
    ORACLE.laplacian(u, mid)
    mid[1:-1, 1:-1] = R.filter_along(mid[1:-1, 1:-1], 0, damping)
    want = np.zeros_like(u)
    ORACLE.laplacian(mid, want)
    assert np.array_equal(d_mid.get().view(np.uint64), mid.view(np.uint64))
    assert np.array_equal(d_out.get().view(np.uint64), want.view(np.uint64))
