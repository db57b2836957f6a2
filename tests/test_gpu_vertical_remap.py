"""``gt4py_amd.vertical`` on the GPU: bit for bit against the contract's restatement (tests/vertical_remap_ref.py), NaN compared
as NaN, over EVERY byte of the destination buffer -- row padding, ghost cells outside the box and the allocation's slack keep a
NaN-payload sentinel, compared as integers --, in the four layouts of tests/device_layouts.py, for float32 / float64 fields against
float32 / float64 edges, at wave and workgroup boundaries along I, for edge sets that make the lanes of a wave diverge, tie,
leave the source range or degenerate, for 1 to 9 fields per call, and handed over to a stencil in stream order.

Wall time of this file on one MI355X: 4.9 s (46 tests; the slowest 0.19 s)."""

import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import device_layouts as L  # noqa: E402  (the layouts; test infrastructure)
import vertical_remap_ref as V  # noqa: E402
from oracle import ref_numpy as ORACLE  # noqa: E402  (oracle = checker only)

METHODS = [V.PCM, V.PLM]
LEVELS = [(1, 1), (1, 5), (5, 1), (2, 3), (17, 9), (9, 17)]


# ---- edge sets: float64 arrays that hold values of the edge dtype, so that the restatement sees what the device sees ------------
def _increments(rng, shape_ij, n):
    return rng.uniform(0.05, 1.0, shape_ij + (n,))


def _source_edges(rng, shape_ij, ns, edtype):
    z = rng.uniform(-2, 2, shape_ij + (1,)) + np.concatenate([np.zeros(shape_ij + (1,)), np.cumsum(_increments(rng, shape_ij, ns), axis=2)], axis=2)
    z = z.astype(edtype).astype(np.float64)
    assert (np.diff(z, axis=2) > 0).all()
    return z


def _between(rng, lo, hi, nd):
    """nd + 1 increasing edges per column from lo to hi (arrays (ni, nj, 1)), those two exactly."""
    t = np.cumsum(_increments(rng, lo.shape[:2], nd), axis=2)
    t = np.concatenate([np.zeros_like(lo), t / t[..., -1:]], axis=2)
    z = lo + (hi - lo) * t
    z[..., :1], z[..., -1:] = lo, hi
    return z


def _target_edges(kind, rng, zs, nd, edtype):
    ns = zs.shape[2] - 1
    lo, hi = zs[..., :1], zs[..., -1:]
    if kind == "random":  # (a) random, reaching a little outside the source range at both ends
        zd = _between(rng, lo - rng.uniform(0, 0.5, lo.shape), hi + rng.uniform(0, 0.5, hi.shape), nd)
    elif kind == "shared_grid":  # (b) one target grid for columns whose source levels are scaled per column: the lanes of a wave diverge
        zd = np.broadcast_to(_between(rng, np.full((1, 1, 1), 0.0), np.full((1, 1, 1), float(hi.min())), nd), zs.shape[:2] + (nd + 1,)).copy()
    elif kind == "coincide":  # (c) every target edge IS a source edge (the > / >= ties); past the last one where nd > ns
        if nd <= ns:
            pick = np.sort(rng.permuted(np.broadcast_to(np.arange(ns + 1), zs.shape).copy(), axis=2)[..., : nd + 1], axis=2)
            zd = np.take_along_axis(zs, pick, axis=2)
        else:
            zd = np.concatenate([zs, hi + np.cumsum(_increments(rng, zs.shape[:2], nd - ns), axis=2)], axis=2)
    elif kind == "whole_column":  # (d) one target cell spans the source column exactly
        assert nd == 1
        zd = np.concatenate([lo, hi], axis=2)
    elif kind == "inside_one_cell":  # (d) every target cell strictly inside source cell 2
        assert ns >= 3
        a, b = zs[..., 2:3], zs[..., 3:4]
        zd = a + (b - a) * np.linspace(0.1, 0.9, nd + 1)
    elif kind == "outside":  # (e) two edges below and two above the source range: whole target cells outside it
        assert nd >= 5
        zd = np.concatenate([lo - 3, lo - 2, _between(rng, lo - 0.5, hi + 0.5, nd - 4), hi + 2, hi + 3], axis=2)
    else:
        raise ValueError(kind)
    zd = zd.astype(edtype).astype(np.float64)
    assert zd.shape[2] == nd + 1 and (np.diff(zd, axis=2) > 0).all(), kind
    return zd


def _fields(rng, shape_ij, ns, nfields, fdtype):
    out = []
    for n in range(nfields):
        if n % 3 == 0:
            q = rng.uniform(-1, 1, shape_ij + (ns,))
        elif n % 3 == 1:  # monotone along K: the limited slopes are not zero
            q = np.cumsum(rng.uniform(0.1, 1, shape_ij + (ns,)), axis=2) * 10.0 ** rng.integers(-3, 4, shape_ij + (1,))
        else:
            q = 280.0 + rng.uniform(-1, 1, shape_ij + (ns,))
        out.append(q.astype(fdtype))
    return out


def _run(ni, nj, ns, nd, method, *, fdtype=np.float64, edtype=np.float64, layout="ifirst", halo=0, nfields=1, kind="random", seed=0,
         shared_src=False, shared_dst=False, edges=None):
    """One call through ``vertical.VerticalRemap``; every dst buffer is compared whole against the restatement, every input must
    come back unchanged.  Returns the boxes of the destinations as the device left them."""
    from gt4py_amd import vertical

    # (edges and fields from generators of their own: the same seed gives the same edges and the same first fields whatever nfields is)
    rng, rng_q = (np.random.default_rng([seed, ni, nj, ns, nd, halo, what]) for what in (0, 1))
    # one ghost cell in front of the halo on the low sides, one ghost row / column behind the array the product sees
    ext = (ni + 2 * halo, nj + 2 * halo)
    seen = (ext[0] + 1, ext[1] + 1)
    shape_ij = (seen[0] + 1, seen[1] + 1)
    origin = (halo + 1, halo + 1, 0)
    box = (slice(1, 1 + ext[0]), slice(1, 1 + ext[1]))
    if edges is None:
        zs = _source_edges(rng, (1, 1) if shared_src else shape_ij, ns, edtype)
        if kind == "shared_grid":
            scale = 1.0 + ((np.arange(shape_ij[0])[:, None] * 7 + np.arange(shape_ij[1])[None, :] * 3) % 11) / 2.0
            zs = ((zs - zs[..., :1]) * scale[..., None]).astype(edtype).astype(np.float64)
        zd = _target_edges(kind, rng, zs[:1, :1] if shared_dst else np.broadcast_to(zs, shape_ij + (ns + 1,)), nd, edtype)
        if shared_dst:
            zd = zd[:1, :1]
    else:
        zs, zd = edges
    qs = _fields(rng_q, shape_ij, ns, nfields, fdtype)
    d_zs = L.Line(zs[0, 0], edtype) if shared_src else L.Dev(shape_ij + (ns + 1,), edtype, layout, zs, origin[0])
    d_zd = L.Line(zd[0, 0], edtype) if shared_dst else L.Dev(shape_ij + (nd + 1,), edtype, layout, zd, origin[0])
    srcs = [L.Dev(shape_ij + (ns,), fdtype, layout, q, origin[0]) for q in qs]
    dsts = [L.Dev(shape_ij + (nd,), fdtype, layout, None, origin[0]) for _ in qs]
    vr = vertical.VerticalRemap([d.given for d in dsts], [s.given for s in srcs], src_edges=d_zs.given, dst_edges=d_zd.given,
                                method=method, halo=halo, origin=origin)
    assert (vr.ns, vr.nd, vr.extent, vr.launches) == (ns, nd, ext, -(-nfields // 8))
    vr()
    what = f"{method} {ni}x{nj} ns={ns} nd={nd} {np.dtype(fdtype)} fields {np.dtype(edtype)} edges {layout} halo {halo} {kind}"
    zs_box = zs[0, 0] if shared_src else zs[box]
    zd_box = zd[0, 0] if shared_dst else zd[box]
    got = []
    for n, (d, q) in enumerate(zip(dsts, qs)):
        want = V.remap_as(q[box], zs_box, zd_box, method)
        got.append(d.assert_box(box, want, f"{what}: dst {n} of {nfields}"))
    for n, s in enumerate(srcs):
        s.assert_unchanged(f"{what}: src {n}")
    d_zs.assert_unchanged(f"{what}: src_edges")
    d_zd.assert_unchanged(f"{what}: dst_edges")
    return got, (zs, zd), qs


# ---- the grid ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nj", [1, 3])
@pytest.mark.parametrize("ni", [1, 63, 64, 65, 130])
def test_extents_at_wave_and_workgroup_boundaries(ni, nj):
    for ns, nd in LEVELS:
        for method in METHODS:
            _run(ni, nj, ns, nd, method, seed=1)


@pytest.mark.parametrize("edtype", [np.float32, np.float64])
@pytest.mark.parametrize("fdtype", [np.float32, np.float64])
@pytest.mark.parametrize("layout", L.LAYOUTS)
def test_layouts_dtypes_and_halos(layout, fdtype, edtype):
    for halo in (0, 2):
        for ns, nd in ((17, 9), (9, 17)):
            for method in METHODS:
                _run(65, 3, ns, nd, method, fdtype=fdtype, edtype=edtype, layout=layout, halo=halo, nfields=3, seed=2)


@pytest.mark.parametrize("kind, ns, nd", [("shared_grid", 17, 9), ("shared_grid", 9, 17), ("coincide", 17, 9), ("coincide", 9, 17),
                                          ("coincide", 5, 5), ("whole_column", 17, 1), ("whole_column", 1, 1), ("inside_one_cell", 5, 4),
                                          ("outside", 9, 17), ("outside", 2, 5), ("outside", 1, 5)])
def test_edge_sets(kind, ns, nd):
    for method in METHODS:
        for fdtype, edtype in ((np.float64, np.float64), (np.float32, np.float32)):
            _run(130, 3, ns, nd, method, fdtype=fdtype, edtype=edtype, nfields=2, kind=kind, seed=3)


@pytest.mark.parametrize("shared_src, shared_dst", [(False, True), (True, False), (True, True)])
def test_edges_as_a_field_of_k_broadcast_without_a_copy(shared_src, shared_dst):
    for method in METHODS:
        for edtype in (np.float32, np.float64):
            for layout in ("ifirst", "kfirst"):
                _run(65, 3, 9, 17, method, fdtype=np.float32, edtype=edtype, layout=layout, halo=1, nfields=2, seed=4, shared_src=shared_src,
                     shared_dst=shared_dst)


@pytest.mark.parametrize("method", METHODS)
def test_degenerate_columns_equal_the_restatement_and_touch_no_other_column(method):
    """A repeated target edge in one column and a NaN in one source edge of another: their values are the restatement's (NaN as
    NaN), and every other column has the bits of a run without them."""
    ni, nj, ns, nd = 130, 3, 9, 17
    clean, (zs, zd), _ = _run(ni, nj, ns, nd, method, nfields=2, seed=5)
    zs, zd = zs.copy(), zd.copy()
    # (array indices: the box starts at 1)
    zd[1 + 70, 1 + 1, 6] = zd[1 + 70, 1 + 1, 5]
    zs[1 + 3, 1 + 2, 4] = np.nan
    zs[1 + 64, 1 + 0, 0] = np.nan
    zs[1 + 129, 1 + 2, ns] = np.nan
    dirty, _, _ = _run(ni, nj, ns, nd, method, nfields=2, seed=5, edges=(zs, zd))
    touched = np.zeros((ni, nj), dtype=bool)
    for i, j in ((70, 1), (3, 2), (64, 0), (129, 2)):
        touched[i, j] = True
    for a, b in zip(clean, dirty):
        assert V.same_bits(a[~touched], b[~touched]).all() and not np.isnan(b[~touched]).any()
        assert np.isnan(b[70, 1, 5])  # 0 / 0


def test_an_entry_does_not_depend_on_its_position_or_on_the_number_of_entries():
    """1, 3, 8 and 9 (two launches) fields per call: every call equals the restatement, and the same field has the same bits in all."""
    from gt4py_amd import vertical

    ni, nj, ns, nd = 65, 3, 17, 9
    for method in METHODS:
        nine, edges, qs = _run(ni, nj, ns, nd, method, fdtype=np.float32, nfields=9, seed=6)
        for count in (8, 3, 1):
            some, _, again = _run(ni, nj, ns, nd, method, fdtype=np.float32, nfields=count, seed=6)
            for n in range(count):
                assert np.array_equal(again[n], qs[n])  # the same inputs
                assert V.same_bits(some[n], nine[n]).all(), (method, count, n)
        # the ninth field (the second launch's first entry) alone, and as entry 2 of 3
        rng = np.random.default_rng(66)
        shape_ij = (ni + 2, nj + 2)
        zs, zd = edges
        d_zs, d_zd = L.Dev(shape_ij + (ns + 1,), np.float64, "ifirst", zs, 1), L.Dev(shape_ij + (nd + 1,), np.float64, "ifirst", zd, 1)
        fillers = _fields(rng, shape_ij, ns, 2, np.float32)
        for position, fields in ((0, [qs[8]]), (2, fillers + [qs[8]])):
            srcs = [L.Dev(shape_ij + (ns,), np.float32, "ifirst", q, 1) for q in fields]
            dsts = [L.Dev(shape_ij + (nd,), np.float32, "ifirst", None, 1) for _ in fields]
            vertical.remap_levels([d.given for d in dsts], [s.given for s in srcs], src_edges=d_zs.given, dst_edges=d_zd.given, method=method,
                                  origin=(1, 1, 0))
            got = dsts[position].assert_box((slice(1, 1 + ni), slice(1, 1 + nj)), nine[8], f"{method}: field 8 at position {position}")
            assert V.same_bits(got, nine[8]).all()


def test_identity_on_the_device_returns_the_source_bit_for_bit():
    """zd identical to zs -- the SAME edge field on both sides -- returns src: pcm every bit, -0.0 included; plm too (fields
    without -0.0)."""
    from gt4py_amd import vertical

    ni, nj, ns = 130, 3, 17
    rng = np.random.default_rng(7)
    shape_ij = (ni + 2, nj + 2)
    box = (slice(1, 1 + ni), slice(1, 1 + nj))
    for fdtype, edtype in ((np.float64, np.float32), (np.float32, np.float64)):
        zs = _source_edges(rng, shape_ij, ns, edtype)
        d_zs = L.Dev(shape_ij + (ns + 1,), edtype, "ifirst", zs, 1)
        for method in METHODS:
            qs = _fields(rng, shape_ij, ns, 3, fdtype)
            if method == V.PCM:
                qs[0][rng.uniform(size=qs[0].shape) < 0.1] = -0.0
            srcs = [L.Dev(shape_ij + (ns,), fdtype, "ifirst", q, 1) for q in qs]
            dsts = [L.Dev(shape_ij + (ns,), fdtype, "jfirst", None) for _ in qs]
            vertical.remap_levels([d.given for d in dsts], [s.given for s in srcs], src_edges=d_zs.given, dst_edges=d_zs.given, method=method,
                                  origin=(1, 1, 0))
            for n, (d, q) in enumerate(zip(dsts, qs)):
                got = d.assert_box(box, q[box], f"identity {method} {np.dtype(fdtype)} field {n}")
                ut = L.NP_UINT[np.dtype(fdtype).itemsize]
                assert np.array_equal(got.view(ut), np.ascontiguousarray(q[box]).view(ut))


def test_hand_over_to_a_stencil_in_stream_order():
    """VerticalRemap, then a device_sync=False stencil that reads dst, nothing in between: the stencil applied to the restatement."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import vertical
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates

    backend, (ni, nj, ns, nd) = "hip:mi300", (96, 40, 12, 7)
    rng = np.random.default_rng(8)
    shape_ij = (ni + 2, nj + 2)
    zs = _source_edges(rng, shape_ij, ns, np.float64)
    zd = _target_edges("random", rng, zs[:1, :1], nd, np.float64)[0, 0]
    q = _fields(rng, shape_ij, ns, 2, np.float64)[1]
    lap = gtscript.stencil(backend=backend, definition=hip_templates.lap_notebook, dtypes={"T": np.float64}, device_sync=False)
    d_q, d_zs = (gt_storage.from_array(a, backend=backend, aligned_index=(1, 1, 0)) for a in (q, zs))
    d_zd = torch.from_numpy(zd).cuda()
    d_p, d_out = (gt_storage.zeros(shape_ij + (nd,), backend=backend, aligned_index=(1, 1, 0)) for _ in range(2))
    to_levels = vertical.VerticalRemap([d_p], [d_q], src_edges=d_zs, dst_edges=d_zd, method="plm", halo=1)
    assert to_levels.extent == shape_ij and to_levels.origin == (1, 1, 0)
    for _ in range(2):  # (the second round finds dst already written: the same result)
        to_levels()
        lap(d_p, d_out, origin=(1, 1, 0), domain=(ni, nj, nd))
    torch.cuda.synchronize()
    p = V.remap_as(q, zs, zd, "plm")
    want = np.zeros_like(p)
    ORACLE.laplacian(p, want)
    assert np.array_equal(d_p.get().view(np.uint64), p.view(np.uint64))
    assert np.array_equal(d_out.get().view(np.uint64), want.view(np.uint64))


def test_the_c_entry_counts_what_it_enqueued():
    import torch

    from gt4py_amd import _lib, vertical

    shape_ij = (9, 4)
    rng = np.random.default_rng(9)
    zs = _source_edges(rng, shape_ij, 5, np.float64)
    d_zs = L.Dev(shape_ij + (6,), np.float64, "ifirst", zs)
    srcs = [L.Dev(shape_ij + (5,), np.float64, "ifirst", q) for q in _fields(rng, shape_ij, 5, 9, np.float64)]
    dsts = [L.Dev(shape_ij + (5,), np.float64, "ifirst", None) for _ in srcs]
    vr = vertical.VerticalRemap([d.given for d in dsts], [s.given for s in srcs], src_edges=d_zs.given, dst_edges=d_zs.given)
    launches = ctypes.c_int(-1)
    rc = _lib.load().gt4mi_vertical_remap(vr._dst, vr._src, 9, ctypes.byref(vr._src_edges), ctypes.byref(vr._dst_edges), vr._extent2, 5, 5, 8, 8,
                                          _lib.REMAP_PCM, 0, torch.cuda.current_stream().cuda_stream, ctypes.byref(launches))
    torch.cuda.synchronize()
    assert rc == 0 and launches.value == 2
