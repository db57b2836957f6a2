"""``gt4py_amd.linesolve`` on the GPU: bit for bit against the contract's restatement (tests/line_solve_ref.py), NaN compared as
NaN, over EVERY byte of every out buffer -- row padding, ghost cells outside the box and the allocation's slack keep a NaN-payload
sentinel (or, in place, the right-hand side), compared as integers.

The extents cross every boundary of the three kernels: line lengths below, at and above one 128-byte tile run for both dtypes (16
float64 / 32 float32 items) and several runs; 1, 63, 64, 65 and 257 lines along the lane axis, i.e. a single line (one live lane),
a partial wave, a full one, a wave plus one and more than a 256-lane workgroup; line lengths around the look-ahead of 4 steps.

Wall time of this file on one MI355X: 2.5 s (37 tests; the slowest 0.20 s)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import device_layouts as L  # noqa: E402  (the layouts; test infrastructure)
import line_solve_ref as R  # noqa: E402
from oracle import ref_numpy as ORACLE  # noqa: E402  (oracle = checker only)

LANES, TILES, ITEMS = "lanes", "tiles", "items"
#: (line length, the extents of the two other axes): every length with a line count of its own
EXTENTS = [(1, (64, 1)), (2, (63, 1)), (3, (257, 1)), (15, (5, 3)), (16, (65, 2)), (17, (5, 3)), (33, (65, 2)), (130, (3, 2)),
           (17, (1, 1)), (130, (1, 1))]  # (the last two: a box that is ONE line)
AXES = "IJK"


def _shape(n, others, axis):
    shape = list(others)
    shape.insert(axis, n)
    return tuple(shape)


def expected_path(layouts, coef_strides, extent, axis):
    """The rule of include/gt4py_amd.h restated: strides in ITEMS of every field, (stride or None for a 1-d coefficient) of the
    coefficients."""
    def unit(ax):
        if any(s[ax] != 1 for s in layouts):
            return False
        return all(s is None or s[ax] == 1 for s in coef_strides)  # (a contiguous 1-d coefficient: unit along the line, broadcast elsewhere)

    if unit(axis) and extent[axis] > 1:
        return TILES
    return LANES if any(unit(ax) and extent[ax] > 1 for ax in range(3) if ax != axis) else ITEMS


def _coefficients(rng, shape, dtype):
    """Diagonally dominant: |b| >= 2 (|a| + |c|), both signs."""
    a, c = rng.uniform(-1, 1, shape), rng.uniform(-1, 1, shape)
    b = (2.0 * (np.abs(a) + np.abs(c)) + rng.uniform(0.1, 1, shape)) * rng.choice([-1.0, 1.0], shape)
    return [v.astype(dtype) for v in (a, b, c)]


def _run(extent, axis, periodic, *, dtype=np.float64, layout="ifirst", rhs_layout=None, nfields=1, inplace=False, line_coefs=False,
         halo=0, k0=0, seed=0, plant=None, want_path=None, nan_workspace=False):
    """One call through ``linesolve.LineSolve``; every out buffer is compared whole against the restatement, every input must
    come back unchanged.  ``extent`` is the box that is solved (the halo included).  Returns the boxes as the device left them."""
    from gt4py_amd import linesolve

    rng = np.random.default_rng([seed, *extent, axis, int(periodic)])
    # one ghost cell in front of the box on the low sides of I and J, one behind the array the product sees, k0 levels below
    shape = (extent[0] + 2, extent[1] + 2, extent[2] + k0)
    box = (slice(1, 1 + extent[0]), slice(1, 1 + extent[1]), slice(k0, None))
    origin = (1 + halo, 1 + halo, k0)
    n = extent[axis]
    if line_coefs:
        coefs = _coefficients(rng, (n,), dtype)
        d_coefs = [L.Line(v) for v in coefs]
        boxes = coefs
    else:
        coefs = _coefficients(rng, shape, dtype)
        if plant is not None:
            plant(coefs)
        d_coefs = [L.Dev(shape, dtype, layout, v, 1) for v in coefs]
        boxes = [v[box] for v in coefs]
    ds = [rng.uniform(-1, 1, shape).astype(dtype) * dtype(10.0 ** (f % 3)) for f in range(nfields)]
    rhs_layout = rhs_layout or layout
    if inplace:
        outs = rhss = [L.Dev(shape, dtype, layout, d, 1) for d in ds]
    else:
        rhss = [L.Dev(shape, dtype, rhs_layout, d, 1) for d in ds]
        outs = [L.Dev(shape, dtype, layout, None, 1) for _ in ds]
    ls = linesolve.LineSolve([o.given for o in outs], [r.given for r in rhss], lower=d_coefs[0].given, diag=d_coefs[1].given,
                             upper=d_coefs[2].given, axis=AXES[axis], periodic=periodic, halo=halo, origin=origin)
    lines = extent[(axis + 1) % 3] * extent[(axis + 2) % 3]
    assert (ls.n, ls.lines, ls.extent, ls.launches) == (n, lines, tuple(extent), -(-nfields // 8))
    if want_path is None:
        strides = [o.lay.strides for o in outs] + [r.lay.strides for r in rhss]
        want_path = expected_path(strides, [None if line_coefs else c.lay.strides for c in d_coefs], extent, axis)
    assert ls.path == want_path, (ls.path, want_path)
    if nan_workspace:
        ls.workspace.tensor.fill_(float("nan"))
    ls()
    what = f"axis {AXES[axis]} extent {extent} periodic {periodic} {np.dtype(dtype)} {layout} {nfields} field(s) inplace {inplace} {ls.path}"
    got = []
    for f, (o, d) in enumerate(zip(outs, ds)):
        want = R.solve_along(*boxes, d[box], axis, periodic)
        got.append(o.assert_box(box, want, f"{what}: out {f}"))
    if not inplace:
        for f, r in enumerate(rhss):
            r.assert_unchanged(f"{what}: rhs {f}")
    for name, c in zip(("lower", "diag", "upper"), d_coefs):
        c.assert_unchanged(f"{what}: {name}")
    return got, ls


@pytest.mark.parametrize("layout", ["ifirst", "kfirst"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_extents_at_tile_wave_and_workgroup_boundaries(axis, layout):
    for n, others in EXTENTS:
        for dtype in (np.float32, np.float64):
            for periodic in (False, True) if n >= 3 else (False,):
                _run(_shape(n, others, axis), axis, periodic, dtype=dtype, layout=layout, seed=1)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_one_to_nine_pairs_in_place_and_out_of_place(axis):
    """9 pairs are two launches; a field has the same bits at every position and in every company."""
    extent = _shape(17, (5, 3), axis)
    for periodic in (False, True):
        for inplace in (False, True):
            nine, ls = _run(extent, axis, periodic, dtype=np.float32, nfields=9, inplace=inplace, seed=2)
            assert ls.launches == 2
            for count in (8, 4, 1):
                some, _ = _run(extent, axis, periodic, dtype=np.float32, nfields=count, inplace=inplace, seed=2)
                for f in range(count):
                    assert R.same_bits(some[f], nine[f]).all(), (periodic, inplace, count, f)
    _run(_shape(33, (65, 2), axis), axis, True, dtype=np.float64, layout="kfirst", nfields=9, inplace=True, seed=2)
    # float64 with all 8 entries (the largest register budgets), out of place and open; ITEMS in float32 with 8 entries
    _run(_shape(33, (65, 2), axis), axis, False, dtype=np.float64, layout="ifirst", nfields=8, seed=2)
    _run(_shape(33, (65, 2), axis), axis, True, dtype=np.float32, layout="ifirst", rhs_layout="kfirst", nfields=8, seed=2, want_path=ITEMS)
    _run(_shape(17, (5, 3), axis), axis, False, dtype=np.float32, layout="kfirst", rhs_layout="jfirst", nfields=4, seed=2, want_path=ITEMS)
    _run(_shape(17, (5, 3), axis), axis, False, dtype=np.float64, layout="kfirst", rhs_layout="jfirst", nfields=1, seed=2, want_path=ITEMS)


@pytest.mark.parametrize("layout", ["ifirst", "kfirst"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_one_dimensional_coefficients_are_broadcast_without_a_copy(axis, layout):
    for periodic in (False, True):
        for dtype in (np.float32, np.float64):
            _run(_shape(33, (65, 2), axis), axis, periodic, dtype=dtype, layout=layout, nfields=2, line_coefs=True, seed=3)


@pytest.mark.parametrize("layout", ["ifirst", "kfirst", "jfirst", "ifirst_unaligned"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_halo_and_an_origin_off_zero(axis, layout):
    for periodic in (False, True):
        _run(_shape(17, (9, 7), axis), axis, periodic, dtype=np.float64, layout=layout, nfields=2, halo=2, k0=1, seed=4)


@pytest.mark.parametrize("layout", ["ifirst", "kfirst"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_without_closure_the_first_lower_and_the_last_upper_item_cannot_reach_a_result(axis, layout):
    """NaN in a[0] and c[n-1] of every line: an open solve has the bits of the restatement, which never reads them."""
    def plant(coefs):
        first, last = [slice(None)] * 3, [slice(None)] * 3
        first[axis], last[axis] = (1 if axis < 2 else 0), (33 if axis < 2 else 32)  # (one ghost cell in front of the box in I and J)
        coefs[0][tuple(first)] = np.nan
        coefs[2][tuple(last)] = np.nan

    for dtype in (np.float32, np.float64):
        got, _ = _run(_shape(33, (65, 2), axis), axis, False, dtype=dtype, layout=layout, nfields=2, seed=9, plant=plant)
        assert not any(np.isnan(g).any() for g in got)


def test_each_kernel_is_reached_by_the_layout_it_is_for():
    """The storage preset (padded rows, I contiguous), a C-ordered torch tensor, and a call whose fields disagree."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import linesolve

    rng = np.random.default_rng(5)
    shape = (33, 9, 4)
    a, b, c = _coefficients(rng, shape, np.float64)
    d = rng.uniform(-1, 1, shape)
    preset = [gt_storage.from_array(v, backend="hip:mi300") for v in (a, b, c, d, np.zeros(shape))]
    assert preset[0].strides[0] == 8 and preset[0].strides[1] > 8 * shape[0]  # I contiguous, rows padded
    c_order = [torch.from_numpy(v).cuda() for v in (a, b, c, d, np.zeros(shape))]
    for fields, paths in ((preset, (TILES, LANES, LANES)), (c_order, (LANES, LANES, TILES))):
        for axis, path in enumerate(paths):
            ls = linesolve.LineSolve(fields[4], fields[3], lower=fields[0], diag=fields[1], upper=fields[2], axis=AXES[axis], periodic=True)
            assert ls.path == path
            ls()
            got = fields[4].get() if hasattr(fields[4], "get") else fields[4].cpu().numpy()
            assert R.same_bits(got, R.solve_along(a, b, c, d, axis, True)).all(), (axis, path)
    for axis in range(3):
        for periodic in (False, True):
            _run(_shape(33, (65, 2), axis), axis, periodic, layout="ifirst", rhs_layout="kfirst", nfields=2, seed=5, want_path=ITEMS)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_field_without_closure_has_the_bits_of_the_shipped_k_solve_on_the_permuted_copy(dtype):
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import linesolve
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates

    backend = "hip:mi300"
    tri = gtscript.stencil(backend=backend, definition=hip_templates.tridiagonal_solver, dtypes={"T": dtype})
    rng = np.random.default_rng(6)
    shape = (40, 33, 5)
    a, b, c = _coefficients(rng, shape, dtype)
    d = rng.uniform(-1, 1, shape).astype(dtype)
    for axis in (0, 1):
        permuted = [gt_storage.from_array(np.ascontiguousarray(np.moveaxis(v, axis, 2)), dtype, backend=backend) for v in (a, b, c, d)]
        x_k = gt_storage.zeros(permuted[0].shape, dtype, backend=backend)
        tri(*permuted, x_k)
        want = np.moveaxis(x_k.get(), 2, axis)
        fields = [gt_storage.from_array(v, dtype, backend=backend) for v in (a, b, c, d)]
        out = gt_storage.zeros(shape, dtype, backend=backend)
        linesolve.solve_lines(out, fields[3], lower=fields[0], diag=fields[1], upper=fields[2], axis=AXES[axis])
        torch.cuda.synchronize()
        assert R.same_bits(out.get(), want).all(), (axis, dtype)
        assert not np.isnan(want).any()


@pytest.mark.parametrize("layout", ["ifirst", "kfirst"])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_a_zero_pivot_and_a_nan_stay_in_their_lines_and_the_workspace_may_hold_anything(axis, layout):
    extent = _shape(33, (65, 2), axis)
    bad = []  # (point on the line, the line's two other indices) as points of the box
    for m, p, r in ((0, 3, 1), (20, 64, 0)):
        point = [p, r]
        point.insert(axis, m)
        bad.append(tuple(point))
    where = [(i + 1, j + 1, k) for i, j, k in bad]  # in the arrays: one ghost cell in front of the box in I and J

    def plant(coefs):
        coefs[1][where[0]] = 0.0     # a zero first pivot
        coefs[0][where[1]] = np.nan  # a NaN in the middle of a line

    for periodic in (False, True):
        clean, _ = _run(extent, axis, periodic, layout=layout, nfields=2, seed=7)
        dirty, _ = _run(extent, axis, periodic, layout=layout, nfields=2, seed=7, plant=plant, nan_workspace=True)
        again, _ = _run(extent, axis, periodic, layout=layout, nfields=2, seed=7, nan_workspace=True)
        touched = np.zeros(extent, dtype=bool)
        for point in bad:
            line = list(point)
            line[axis] = slice(None)
            touched[tuple(line)] = True
        for x, y, z in zip(clean, dirty, again):
            assert R.same_bits(x[~touched], y[~touched]).all() and not np.isnan(y[~touched]).any()
            assert not np.isfinite(y[touched]).all()
            assert R.same_bits(x, z).all()


def test_hand_over_from_and_to_stencils_in_stream_order():
    """A device_sync=False stencil writes rhs, LineSolve solves along I, a device_sync=False stencil reads out; nothing in between."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import linesolve
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates

    backend, (ni, nj, nk) = "hip:mi300", (96, 40, 6)
    rng = np.random.default_rng(8)
    shape = (ni + 2, nj + 2, nk)
    a, b, c = _coefficients(rng, shape, np.float64)
    u, ring = rng.uniform(-1, 1, shape), rng.uniform(-1, 1, shape)
    lap = gtscript.stencil(backend=backend, definition=hip_templates.lap_notebook, dtypes={"T": np.float64}, device_sync=False)
    d_a, d_b, d_c, d_u, d_rhs = (gt_storage.from_array(v, backend=backend, aligned_index=(1, 1, 0)) for v in (a, b, c, u, ring))
    d_x, d_out = (gt_storage.zeros(shape, backend=backend, aligned_index=(1, 1, 0)) for _ in range(2))
    # the box is the domain and its ghost ring; the stencil in front writes the domain of rhs, the ring keeps what it was given
    solve = linesolve.LineSolve(d_x, d_rhs, lower=d_a, diag=d_b, upper=d_c, axis="I", periodic=True, halo=1)
    assert solve.extent == shape and solve.origin == (1, 1, 0) and solve.path == TILES
    for _ in range(2):  # (the second round finds everything already written: the same result)
        lap(d_u, d_rhs, origin=(1, 1, 0), domain=(ni, nj, nk))
        solve()
        lap(d_x, d_out, origin=(1, 1, 0), domain=(ni, nj, nk))
    torch.cuda.synchronize()
    rhs = ring.copy()
    ORACLE.laplacian(u, rhs)
    x = R.solve_along(a, b, c, rhs, 0, True)
    want = np.zeros(shape)
    ORACLE.laplacian(x, want)
    assert np.array_equal(d_rhs.get().view(np.uint64), rhs.view(np.uint64))
    assert np.array_equal(d_x.get().view(np.uint64), x.view(np.uint64))
    assert np.array_equal(d_out.get().view(np.uint64), want.view(np.uint64))
