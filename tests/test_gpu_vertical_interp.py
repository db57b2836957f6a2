"""``gt4py_amd.vertical.interpolate_levels`` on the GPU: bit for bit against the contract's restatement
(tests/vertical_interp_ref.py), NaN compared as NaN, over EVERY byte of the destination buffer -- row padding, ghost cells outside
the box and the allocation's slack keep a NaN-payload sentinel, compared as integers --, in the four layouts of
tests/device_layouts.py, for float32 / float64 fields against float32 / float64 coordinates, at wave and workgroup boundaries along
I, for every method and every ``outside`` value, for target sets that run up, run down, jump, tie with source levels, leave the
source range or hold a NaN, for lanes of a wave at different brackets, for 1 to 9 fields per call, and handed over to a stencil in
stream order.

Wall time of this file on one MI355X: 5.3 s (51 tests; the slowest 0.21 s)."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import device_layouts as L  # noqa: E402  (the layouts; test infrastructure)
import vertical_interp_ref as V  # noqa: E402
from oracle import ref_numpy as ORACLE  # noqa: E402  (oracle = checker only)

LEVELS = [(2, 1), (2, 5), (3, 4), (4, 4), (5, 1), (17, 9), (9, 17)]
KINDS = ["inside", "increasing", "decreasing", "shuffled", "on_levels", "some_outside", "all_below", "all_above", "nan_middle"]


# ---- coordinates: float64 arrays that hold values of the coordinate dtype, so that the restatement sees what the device sees -----
def _source_coords(rng, shape_ij, ns, cdtype, scale=None):
    z = np.cumsum(rng.uniform(0.05, 1.0, shape_ij + (ns,)), axis=2)
    if scale is None:
        z = z + rng.uniform(-2, 2, shape_ij + (1,))
    else:  # every column starts at 0 and is stretched by its own factor: one shared target grid finds the lanes at different k
        z = (z - z[..., :1]) * scale[..., None]
    z = z.astype(cdtype).astype(np.float64)
    assert (np.diff(z, axis=2) > 0).all(), "source coordinates must increase strictly after rounding to the coordinate dtype"
    return z


def _targets(kind, rng, z, nd, cdtype):
    """``nd`` targets for every column of ``z`` (one column: a shared Field[K])."""
    lo, hi = z[..., :1], z[..., -1:]
    shape = z.shape[:2] + (nd,)
    inside = lo + (hi - lo) * rng.uniform(0, 1, shape)
    if kind == "inside":
        x = inside
    elif kind == "increasing":
        x = np.sort(inside, axis=2)
    elif kind == "decreasing":  # the hunt runs down
        x = np.sort(inside, axis=2)[..., ::-1]
    elif kind == "shuffled":
        x = rng.permuted(np.sort(inside, axis=2), axis=2)
    elif kind == "on_levels":  # every target ON a source level: the <= and > ties, t == 0
        x = np.take_along_axis(z, rng.integers(0, z.shape[2], shape), axis=2)
    elif kind == "some_outside":
        x = inside.copy()
        x[..., 0::3] = lo - rng.uniform(0.01, 3, x[..., 0::3].shape)
        x[..., 1::3] = hi + rng.uniform(0.01, 3, x[..., 1::3].shape)
    elif kind == "all_below":
        x = lo - rng.uniform(0.01, 3, shape)
    elif kind == "all_above":
        x = hi + rng.uniform(0.01, 3, shape)
    elif kind == "nan_middle":
        x = inside.copy()
        x[..., nd // 2] = np.nan
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x).astype(cdtype).astype(np.float64)


def _fields(rng, shape_ij, ns, nfields, fdtype):
    out = []
    for n in range(nfields):
        if n % 3 == 0:
            q = rng.uniform(-1, 1, shape_ij + (ns,))
        elif n % 3 == 1:  # monotone along K over many decades
            q = np.cumsum(rng.uniform(0.1, 1, shape_ij + (ns,)), axis=2) * 10.0 ** rng.integers(-3, 4, shape_ij + (1,))
        else:
            q = 280.0 + rng.uniform(-1, 1, shape_ij + (ns,))
        out.append(q.astype(fdtype))
    return out


def _run(ni, nj, ns, nd, method, outside=V.CLAMP, *, fill_value=V.NAN, fdtype=np.float64, cdtype=np.float64, layout="ifirst", halo=0,
         nfields=1, kind="inside", seed=0, shared_src=False, shared_dst=False, scaled=False, frozen=True):
    """One call through ``vertical.VerticalInterp`` (``frozen=False``: ``interpolate_levels``); every dst buffer is compared whole
    against the restatement, every input must come back unchanged.  Returns the boxes of the destinations as the device left them."""
    from gt4py_amd import vertical

    # (coordinates and fields from generators of their own: the same seed gives the same coordinates and the same first fields
    # whatever nfields is)
    rng, rng_q = (np.random.default_rng([seed, ni, nj, ns, nd, halo, what]) for what in (0, 1))
    # one ghost cell in front of the halo on the low sides, one ghost row / column behind the array the product sees
    ext = (ni + 2 * halo, nj + 2 * halo)
    shape_ij = (ext[0] + 2, ext[1] + 2)
    origin = (halo + 1, halo + 1, 0)
    box = (slice(1, 1 + ext[0]), slice(1, 1 + ext[1]))
    scale = 1.0 + ((np.arange(shape_ij[0])[:, None] * 7 + np.arange(shape_ij[1])[None, :] * 3) % 11) / 2.0 if scaled else None
    z = _source_coords(rng, (1, 1) if shared_src else shape_ij, ns, cdtype, scale)
    x = _targets(kind, rng, z[:1, :1] if shared_dst else np.broadcast_to(z, shape_ij + (ns,)), nd, cdtype)
    qs = _fields(rng_q, shape_ij, ns, nfields, fdtype)
    d_z = L.Line(z[0, 0], cdtype) if shared_src else L.Dev(shape_ij + (ns,), cdtype, layout, z, origin[0])
    d_x = L.Line(x[0, 0], cdtype) if shared_dst else L.Dev(shape_ij + (nd,), cdtype, layout, x, origin[0])
    srcs = [L.Dev(shape_ij + (ns,), fdtype, layout, q, origin[0]) for q in qs]
    dsts = [L.Dev(shape_ij + (nd,), fdtype, layout, None, origin[0]) for _ in qs]
    args = ([d.given for d in dsts], [s.given for s in srcs])
    kwargs = dict(src_coord=d_z.given, dst_coord=d_x.given, method=method, outside=outside, fill_value=fill_value, halo=halo, origin=origin)
    if frozen:
        vi = vertical.VerticalInterp(*args, **kwargs)
        assert (vi.ns, vi.nd, vi.extent, vi.launches, vi.method, vi.outside) == (ns, nd, ext, -(-nfields // 8), method, outside)
        vi()
    else:
        vertical.interpolate_levels(*args, **kwargs)
    what = (f"{method} outside={outside} {ni}x{nj} ns={ns} nd={nd} {np.dtype(fdtype)} fields {np.dtype(cdtype)} coordinates {layout} "
            f"halo {halo} {kind}")
    z_box = z[0, 0] if shared_src else z[box]
    x_box = x[0, 0] if shared_dst else x[box]
    got = []
    for n, (d, q) in enumerate(zip(dsts, qs)):
        want = V.interp(q[box], z_box, x_box, method, outside, fill_value)
        got.append(d.assert_box(box, want, f"{what}: dst {n} of {nfields}"))
    for n, s in enumerate(srcs):
        s.assert_unchanged(f"{what}: src {n}")
    d_z.assert_unchanged(f"{what}: src_coord")
    d_x.assert_unchanged(f"{what}: dst_coord")
    return got, qs


# ---- the grid ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nj", [1, 4, 5])
@pytest.mark.parametrize("ni", [1, 63, 64, 65, 129])
def test_extents_at_wave_and_workgroup_boundaries(ni, nj):
    for n, (ns, nd) in enumerate(LEVELS):
        for m, method in enumerate(V.METHODS):
            _run(ni, nj, ns, nd, method, V.OUTSIDE[(n + m) % 3], kind="some_outside", seed=1)


@pytest.mark.parametrize("cdtype", [np.float32, np.float64])
@pytest.mark.parametrize("fdtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", L.LAYOUTS)
def test_layouts_dtypes_and_halos(layout, fdtype, cdtype):
    for halo in (0, 2):
        for ns, nd in ((17, 9), (9, 17)):
            for m, method in enumerate(V.METHODS):
                _run(65, 5, ns, nd, method, V.OUTSIDE[(m + halo) % 3], fill_value=-999.25, fdtype=fdtype, cdtype=cdtype, layout=layout, halo=halo,
                     nfields=3, kind="some_outside", seed=2)


@pytest.mark.parametrize("outside", V.OUTSIDE)
@pytest.mark.parametrize("method", V.METHODS)
def test_every_method_and_outside_value_on_every_target_set(method, outside):
    for kind in KINDS:
        for (fdtype, cdtype), (ns, nd) in (((np.float64, np.float64), (9, 17)), ((np.float32, np.float32), (17, 9))):
            _run(129, 4, ns, nd, method, outside, fdtype=fdtype, cdtype=cdtype, nfields=2, kind=kind, seed=3)
    for ns, nd in ((2, 5), (3, 4), (4, 4)):  # the cubics fall back to linear in every interval, or in all but one
        for kind in ("on_levels", "all_below", "all_above", "nan_middle"):
            _run(65, 1, ns, nd, method, outside, fill_value=1.0e300, fdtype=np.float32, kind=kind, seed=3)  # (the fill rounds to inf)


@pytest.mark.parametrize("shared_src, shared_dst, scaled", [(False, True, True), (False, True, False), (True, False, False), (True, True, False)])
def test_coordinates_as_a_field_of_k_broadcast_without_a_copy(shared_src, shared_dst, scaled):
    """``scaled``: ONE shared target grid against source coordinates stretched per column: the lanes of a wave sit at different k."""
    for method in V.METHODS:
        for cdtype in (np.float32, np.float64):
            for layout, kind in (("ifirst", "shuffled"), ("kfirst", "some_outside")):
                _run(129, 4, 9, 17, method, V.EXTEND, fdtype=np.float32, cdtype=cdtype, layout=layout, halo=1, nfields=2, kind=kind, seed=4,
                     shared_src=shared_src, shared_dst=shared_dst, scaled=scaled)


def test_an_entry_does_not_depend_on_its_position_or_on_the_number_of_entries():
    """1, 2, 8 and 9 (two launches) fields per call: every call equals the restatement, and the first fields have the same bits in
    all of them."""
    ni, nj, ns, nd = 65, 5, 17, 9
    for method, outside in ((V.NEAREST, V.FILL), (V.LINEAR, V.EXTEND), (V.CUBIC, V.CLAMP), (V.CUBIC_MONOTONE, V.FILL)):
        nine, qs = _run(ni, nj, ns, nd, method, outside, fdtype=np.float32, nfields=9, kind="some_outside", seed=6)
        for count in (8, 2, 1):
            some, again = _run(ni, nj, ns, nd, method, outside, fdtype=np.float32, nfields=count, kind="some_outside", seed=6)
            for n in range(count):
                assert np.array_equal(again[n], qs[n])  # the same inputs
                assert V.same_bits(some[n], nine[n]).all(), (method, count, n)


def test_the_function_and_the_frozen_form_give_the_same_bytes():
    for method, outside in ((V.NEAREST, V.CLAMP), (V.LINEAR, V.FILL), (V.CUBIC_MONOTONE, V.EXTEND)):
        for fdtype in (np.float32, np.float64):
            a, _ = _run(129, 4, 9, 17, method, outside, fdtype=fdtype, nfields=3, kind="some_outside", seed=7, halo=1, frozen=True)
            b, _ = _run(129, 4, 9, 17, method, outside, fdtype=fdtype, nfields=3, kind="some_outside", seed=7, halo=1, frozen=False)
            for x, y in zip(a, b):
                assert V.same_bits(x, y).all()


def test_hand_over_to_a_stencil_in_stream_order():
    """VerticalInterp, then a device_sync=False stencil that reads dst, nothing in between: the stencil applied to the restatement."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import vertical
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates

    backend, (ni, nj, ns, nd) = "hip:mi300", (96, 40, 12, 7)
    rng = np.random.default_rng(8)
    shape_ij = (ni + 2, nj + 2)
    z = _source_coords(rng, shape_ij, ns, np.float64)
    x = _targets("shuffled", rng, z[:1, :1], nd, np.float64)[0, 0]
    q = _fields(rng, shape_ij, ns, 2, np.float64)[1]
    lap = gtscript.stencil(backend=backend, definition=hip_templates.lap_notebook, dtypes={"T": np.float64}, device_sync=False)
    d_q, d_z = (gt_storage.from_array(a, backend=backend, aligned_index=(1, 1, 0)) for a in (q, z))
    d_x = torch.from_numpy(x).cuda()
    d_p, d_out = (gt_storage.zeros(shape_ij + (nd,), backend=backend, aligned_index=(1, 1, 0)) for _ in range(2))
    to_levels = vertical.VerticalInterp([d_p], [d_q], src_coord=d_z, dst_coord=d_x, method="cubic_monotone", outside="linear", halo=1)
    assert to_levels.extent == shape_ij and to_levels.origin == (1, 1, 0)
    for _ in range(2):  # (the second round finds dst already written: the same result)
        to_levels()
        lap(d_p, d_out, origin=(1, 1, 0), domain=(ni, nj, nd))
    torch.cuda.synchronize()
    p = V.interp(q, z, x, V.CUBIC_MONOTONE, V.EXTEND)
    want = np.zeros_like(p)
    ORACLE.laplacian(p, want)
    assert np.array_equal(d_p.get().view(np.uint64), p.view(np.uint64))
    assert np.array_equal(d_out.get().view(np.uint64), want.view(np.uint64))


def test_the_c_entry_counts_what_it_enqueued():
    import torch

    from gt4py_amd import _lib, vertical

    shape_ij = (9, 4)
    rng = np.random.default_rng(9)
    z = _source_coords(rng, shape_ij, 5, np.float64)
    d_z = L.Dev(shape_ij + (5,), np.float64, "ifirst", z)
    srcs = [L.Dev(shape_ij + (5,), np.float64, "ifirst", q) for q in _fields(rng, shape_ij, 5, 9, np.float64)]
    dsts = [L.Dev(shape_ij + (5,), np.float64, "ifirst", None) for _ in srcs]
    vi = vertical.VerticalInterp([d.given for d in dsts], [s.given for s in srcs], src_coord=d_z.given, dst_coord=d_z.given, method="nearest")
    launches = ctypes.c_int(-1)
    rc = _lib.load().gt4mi_vertical_interp(vi._dst, vi._src, 9, ctypes.byref(vi._src_coord), ctypes.byref(vi._dst_coord), vi._extent2, 5, 5, 8, 8,
                                           _lib.VINTERP_NEAREST, _lib.VINTERP_OUTSIDE_CLAMP, 0.0, 0, torch.cuda.current_stream().cuda_stream,
                                           ctypes.byref(launches))
    torch.cuda.synchronize()
    assert rc == 0 and launches.value == 2
    # the source levels as targets, nearest: the identity, bit for bit
    box = (slice(0, 8), slice(0, 3))
    for d, s in zip(dsts, srcs):
        d.assert_box(box, s.host(s.image)[box], "identity")
