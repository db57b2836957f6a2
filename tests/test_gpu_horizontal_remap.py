"""``gt4py_amd.horizontal.remap_cells`` on the GPU: bit for bit against the contract's restatement (tests/horizontal_remap_ref.py),
NaN compared as NaN, over EVERY byte of the destination buffer -- row padding, ghost cells outside the box and the allocation's
slack keep a NaN-payload sentinel, compared as integers --, with the four layouts of tests/device_layouts.py on the two sides
independently, for float32 / float64 fields and both methods, at wave and workgroup boundaries along the destination I and J, at
level counts around the chunk of 8, for coarsening by 2, 3 and a non-integer ratio, refinement by 3, identical grids, one cell over
everything and destination cells outside the source grid, for 1 to 9 fields per call, with an infinity and a NaN planted, and
handed over to a stencil in stream order.

Wall time of this file on one MI355X: 3.5 s (77 tests; the slowest 0.30 s)."""

import ctypes
import functools
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import device_layouts as L  # noqa: E402  (the layouts; test infrastructure)
import horizontal_remap_ref as R  # noqa: E402
from oracle import ref_numpy as ORACLE  # noqa: E402  (oracle = checker only)

METHODS = [R.PCM, R.PLM]


# ---- grids: (source edges, destination edges) of one axis for a destination extent nd ----------------------------------------
def _random_edges(rng, n, lo, hi):
    t = np.concatenate([[0.0], np.cumsum(rng.uniform(0.2, 1.0, n))])
    x = lo + (hi - lo) * t / t[-1]
    x[0], x[-1] = lo, hi
    assert (np.diff(x) > 0).all()
    return x


def _axis(kind, nd, rng):
    if kind in ("2:1", "3:1"):  # uniform, exact weights
        r = int(kind[0])
        return np.arange(nd * r + 1, dtype=np.float64), np.arange(nd + 1, dtype=np.float64) * r
    if kind == "noninteger":  # 65 -> 27, 9 -> 4, ...: random edges on both sides, the outer ones shared
        ns = max(nd * 65 // 27, 1)
        return _random_edges(rng, ns, -1.0, 3.0), _random_edges(rng, nd, -1.0, 3.0)
    if kind == "refine":  # 1:3, uniform
        ns = -(-nd // 3)
        return np.arange(ns + 1, dtype=np.float64) * 3, np.arange(nd + 1, dtype=np.float64)
    if kind == "identical":
        x = _random_edges(rng, nd, 0.0, 5.0)
        return x, x.copy()
    if kind == "outside":  # whole destination cells below and above the source range (where there are enough of them)
        ns = max(nd // 3, 1)
        xs = _random_edges(rng, ns, 0.0, 4.0)
        return xs, _random_edges(rng, nd, -3.0, 7.5) if nd >= 3 else np.linspace(4.5, 6.0, nd + 1)
    raise ValueError(kind)


def _fields(rng, shape, count, dtype):
    ni, nj, nk = shape
    out = []
    for n in range(count):
        if n % 3 == 0:
            q = rng.uniform(-1, 1, shape)
        elif n % 3 == 1:  # monotone along I and J: the limited slopes are not zero
            q = (np.cumsum(rng.uniform(0.1, 1, ni))[:, None, None] + np.cumsum(rng.uniform(0.1, 1, nj))[None, :, None]
                 + rng.uniform(0, 0.05, shape)) * 10.0 ** rng.integers(-2, 3, (1, 1, nk))
        else:
            q = 280.0 + rng.uniform(-1, 1, shape)
        out.append(q.astype(dtype))
    return out


@functools.lru_cache(maxsize=None)
def _case(kind_i, kind_j, nd_i, nd_j, nk, fdtype, nfields, seed):
    """(edges, sources, what the restatement makes of them per method): computed once, shared, never changed."""
    rng = np.random.default_rng([seed, nd_i, nd_j, nk])
    (xs_i, xd_i), (xs_j, xd_j) = _axis(kind_i, nd_i, rng), _axis(kind_j, nd_j, rng)
    qs = _fields(np.random.default_rng([seed, 1]), (xs_i.size - 1, xs_j.size - 1, nk), nfields, fdtype)
    wants = {m: [R.remap_as(q, (xs_i, xs_j), (xd_i, xd_j), m) for q in qs] for m in METHODS}
    for a in (xs_i, xs_j, xd_i, xd_j, *qs, *[w for ws in wants.values() for w in ws]):
        a.setflags(write=False)
    return ((xs_i, xs_j), (xd_i, xd_j)), qs, wants


def _call(edges, qs, method, fdtype, dst_layout="ifirst", src_layout="ifirst", wants=None, what=""):
    """One call through ``horizontal.HorizontalRemap`` on fields with a ghost cell around the boxes; every dst buffer is compared
    whole against ``wants`` (default: the restatement), every input must come back unchanged.  Returns the dst boxes as the device
    left them."""
    from gt4py_amd import horizontal

    (xs_i, xs_j), (xd_i, xd_j) = edges
    ns, nd, nk = (xs_i.size - 1, xs_j.size - 1), (xd_i.size - 1, xd_j.size - 1), qs[0].shape[2]
    if wants is None:
        wants = [R.remap_as(q, *edges, method) for q in qs]
    s_shape, d_shape = (ns[0] + 3, ns[1] + 3, nk), (nd[0] + 3, nd[1] + 3, nk)
    s_box, d_box = (slice(1, 1 + ns[0]), slice(1, 1 + ns[1])), (slice(1, 1 + nd[0]), slice(1, 1 + nd[1]))
    srcs = []
    for q in qs:
        full = np.random.default_rng(5).uniform(50, 60, s_shape).astype(fdtype)  # ghost cells: finite, far from the fields' values
        full[s_box] = q
        srcs.append(L.Dev(s_shape, fdtype, src_layout, full, 1))
    dsts = [L.Dev(d_shape, fdtype, dst_layout, None, 1) for _ in qs]
    hr = horizontal.HorizontalRemap([d.given for d in dsts], [s.given for s in srcs], src_edges=(xs_i, xs_j), dst_edges=(xd_i, xd_j),
                                    method=method, src_origin=(1, 1, 0), dst_origin=(1, 1, 0))
    assert (hr.src_extent, hr.dst_extent, hr.nk, hr.launches) == (ns, nd, nk, -(-len(qs) // 8))
    tables = [t.cpu().numpy().copy() for t in hr._tables]
    hr()
    what = f"{what} {method} {ns}->{nd} x {nk} {np.dtype(fdtype)} dst {dst_layout} src {src_layout}"
    got = [d.assert_box(d_box, want, f"{what}: dst {n} of {len(qs)}") for n, (d, want) in enumerate(zip(dsts, wants))]
    for n, s in enumerate(srcs):
        s.assert_unchanged(f"{what}: src {n}")
    for axis, (xs, xd) in enumerate(((xs_i, xd_i), (xs_j, xd_j))):  # the tables are the host entry's, before and after
        ptr, cell, *reals = horizontal.overlap_table(xs, xd)
        assert hr.terms[axis] == cell.size
        for before, t, host in zip(tables[2 * axis:], hr._tables[2 * axis:2 * axis + 2], (np.concatenate([ptr, cell]), np.concatenate(reals))):
            assert np.array_equal(before.view(np.uint8), host.view(np.uint8)) and np.array_equal(t.cpu().numpy().view(np.uint8), host.view(np.uint8))
    return got


def _run(kind_i, kind_j, nd_i, nd_j, nk, fdtype=np.float64, nfields=1, seed=0, methods=METHODS, **layouts):
    edges, qs, wants = _case(kind_i, kind_j, nd_i, nd_j, nk, fdtype, nfields, seed)
    return {m: _call(edges, qs, m, fdtype, wants=wants[m], what=f"{kind_i} / {kind_j}", **layouts) for m in methods}


# ---- the grid ----------------------------------------------------------------------------------------------------------------------
NK_OF_NJ = {1: 17, 4: 9, 5: 8, 9: 1}


@pytest.mark.parametrize("nd_j", [1, 4, 5, 9])
@pytest.mark.parametrize("nd_i", [1, 63, 64, 65, 130])
def test_destination_extents_at_wave_and_workgroup_boundaries(nd_i, nd_j):
    kind_i, kind_j = ("2:1", "noninteger") if (nd_i + nd_j) % 2 else ("noninteger", "2:1")
    _run(kind_i, kind_j, nd_i, nd_j, NK_OF_NJ[nd_j], seed=1)


@pytest.mark.parametrize("nk", [1, 8, 9, 17])
def test_levels_around_the_chunk(nk):
    _run("3:1", "noninteger", 65, 5, nk, fdtype=np.float32, nfields=2, seed=2)


@pytest.mark.parametrize("fdtype", [np.float32, np.float64])
@pytest.mark.parametrize("src_layout", L.LAYOUTS)
@pytest.mark.parametrize("dst_layout", L.LAYOUTS)
def test_layouts_of_the_two_sides_and_dtypes(dst_layout, src_layout, fdtype):
    _run("noninteger", "noninteger", 27, 4, 3, fdtype=fdtype, nfields=2, seed=3, dst_layout=dst_layout, src_layout=src_layout)  # 65 x 9 -> 27 x 4


@pytest.mark.parametrize("kind, nd_i, nd_j", [("2:1", 65, 5), ("3:1", 64, 4), ("refine", 65, 9), ("refine", 130, 4), ("outside", 65, 9),
                                              ("outside", 63, 1)])
@pytest.mark.parametrize("fdtype", [np.float32, np.float64])
def test_ratios_refinement_and_cells_outside_the_source_grid(kind, nd_i, nd_j, fdtype):
    _run(kind, kind, nd_i, nd_j, 2, fdtype=fdtype, nfields=2, seed=4)


@pytest.mark.parametrize("fdtype", [np.float32, np.float64])
def test_one_destination_cell_over_a_130_by_9_source(fdtype):
    rng = np.random.default_rng(5)
    xs = (_random_edges(rng, 130, 0.0, 9.0), _random_edges(rng, 9, -1.0, 1.0))
    qs = _fields(rng, (130, 9, 3), 2, fdtype)
    for xd in ((np.array([0.0, 9.0]), np.array([-1.0, 1.0])), (np.array([-2.0, 11.0]), np.array([-1.5, 1.25]))):  # exactly, and beyond
        for method in METHODS:
            _call((xs, xd), qs, method, fdtype, what="one cell")


@pytest.mark.parametrize("fdtype", [np.float32, np.float64])
def test_identical_grids_return_the_source_bit_for_bit(fdtype):
    """pcm: every bit, -0.0 included; plm too on fields without -0.0 (q + s * 0.0)."""
    rng = np.random.default_rng(6)
    xs = (_random_edges(rng, 130, 0.0, 5.0), _random_edges(rng, 9, 0.0, 2.0))
    ut = L.NP_UINT[np.dtype(fdtype).itemsize]
    for method in METHODS:
        qs = _fields(rng, (130, 9, 9), 3, fdtype)
        if method == R.PCM:
            qs[0][rng.uniform(size=qs[0].shape) < 0.1] = -0.0
        got = _call((xs, xs), qs, method, fdtype, dst_layout="jfirst", wants=qs, what="identity")
        for g, q in zip(got, qs):
            assert np.array_equal(g.view(ut), q.view(ut))


def test_an_entry_does_not_depend_on_its_position_or_on_the_number_of_entries():
    """1, 4, 8 and 9 (two launches) fields per call: every call equals the restatement, and the same field has the same bits in all
    -- also as the only entry and as entry 2 of 3."""
    edges, qs, wants = _case("noninteger", "noninteger", 27, 4, 3, np.float32, 9, 7)
    for method in METHODS:
        nine = _call(edges, qs, method, np.float32, wants=wants[method])
        for count in (8, 4, 1):
            some = _call(edges, qs[:count], method, np.float32, wants=wants[method][:count])
            for n in range(count):
                assert R.same_bits(some[n], nine[n]).all(), (method, count, n)
        fillers = _fields(np.random.default_rng(77), qs[0].shape, 2, np.float32)
        for position, fields in ((0, [qs[8]]), (2, fillers + [qs[8]])):
            got = _call(edges, fields, method, np.float32)
            assert R.same_bits(got[position], nine[8]).all(), (method, position)


@pytest.mark.parametrize("method", METHODS)
def test_an_infinity_and_a_nan_change_only_the_cells_whose_overlap_holds_them(method):
    """Source 0 holds an infinity, source 1 a NaN: both calls equal the restatement (NaN as NaN), and against the clean run only the
    destination cells whose terms read the planted item may differ -- for plm that is the item's cell and its neighbours along I
    and J, whose slopes read it."""
    edges, qs, wants = _case("noninteger", "noninteger", 27, 4, 3, np.float64, 2, 8)
    clean = _call(edges, qs, method, np.float64, wants=wants[method])
    (xs_i, xs_j), (xd_i, xd_j) = edges
    where = [(31, 4, 1), (64, 0, 2)]  # (source i, source j, level); the second in a corner cell
    dirty_qs = [q.copy() for q in qs]
    dirty_qs[0][where[0]], dirty_qs[1][where[1]] = np.inf, np.nan
    dirty = _call(edges, dirty_qs, method, np.float64)
    tables = [R.axis_table([float(v) for v in s], [float(v) for v in d]) for s, d in ((xs_i, xd_i), (xs_j, xd_j))]
    reach = 1 if method == R.PLM else 0
    for n, (a, b, k) in enumerate(where):
        may = np.zeros(clean[n].shape, dtype=bool)
        hit_i = [m for m in range(27) if any(abs(c - a) <= reach for c in tables[0][1][tables[0][0][m]:tables[0][0][m + 1]])]
        hit_j = [m for m in range(4) if any(abs(c - b) <= reach for c in tables[1][1][tables[1][0][m]:tables[1][0][m + 1]])]
        cells_i = [m for m in range(27) if a in tables[0][1][tables[0][0][m]:tables[0][0][m + 1]]]
        cells_j = [m for m in range(4) if b in tables[1][1][tables[1][0][m]:tables[1][0][m + 1]]]
        may[np.ix_(hit_i, cells_j, [k])] = True  # (a slope along I is read by the terms of the item's own J cell, and vice versa)
        may[np.ix_(cells_i, hit_j, [k])] = True
        assert R.same_bits(clean[n][~may], dirty[n][~may]).all() and np.isfinite(dirty[n][~may]).all()
        assert not np.isfinite(dirty[n][np.ix_(cells_i, cells_j, [k])]).any()
        other = 1 - n
        assert R.same_bits(clean[other][:, :, [x for x in range(3) if x != where[other][2]]],
                           dirty[other][:, :, [x for x in range(3) if x != where[other][2]]]).all()


def test_hand_over_to_a_stencil_in_stream_order():
    """HorizontalRemap, then a device_sync=False stencil that reads dst, nothing in between: the stencil applied to the restatement."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import horizontal
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates

    backend, (ni, nj, nk) = "hip:mi300", (66, 30, 5)
    rng = np.random.default_rng(9)
    xd = (_random_edges(rng, ni + 2, 0.0, 10.0), _random_edges(rng, nj + 2, 0.0, 4.0))
    xs = (_random_edges(rng, 150, 0.0, 10.0), _random_edges(rng, 71, 0.0, 4.0))
    q = _fields(rng, (150, 71, nk), 2, np.float64)[1]
    lap = gtscript.stencil(backend=backend, definition=hip_templates.lap_notebook, dtypes={"T": np.float64}, device_sync=False)
    d_q = gt_storage.from_array(q, backend=backend)
    d_p, d_out = (gt_storage.zeros((ni + 2, nj + 2, nk), backend=backend, aligned_index=(1, 1, 0)) for _ in range(2))
    coarsen = horizontal.HorizontalRemap([d_p], [d_q], src_edges=xs, dst_edges=xd, method="plm")
    assert coarsen.dst_extent == (ni + 2, nj + 2) and coarsen.src_extent == (150, 71) and coarsen.nk == nk
    for _ in range(2):  # (the second round finds dst already written: the same result)
        coarsen()
        lap(d_p, d_out, origin=(1, 1, 0), domain=(ni, nj, nk))
    torch.cuda.synchronize()
    p = R.remap_as(q, xs, xd, "plm")
    want = np.zeros_like(p)
    ORACLE.laplacian(p, want)
    assert np.array_equal(d_p.get().view(np.uint64), p.view(np.uint64))
    assert np.array_equal(d_out.get().view(np.uint64), want.view(np.uint64))


def test_the_frozen_call_counts_its_launches_and_refuses_to_run_after_a_bound_array_died():
    import torch

    from gt4py_amd import _lib, horizontal

    x = np.arange(9.0)
    srcs = [torch.full((8, 8, 2), float(n), dtype=torch.float64, device="cuda") for n in range(9)]
    dsts = [torch.zeros((4, 4, 2), dtype=torch.float64, device="cuda") for _ in range(9)]
    hr = horizontal.HorizontalRemap(dsts, srcs, src_edges=(x, x), dst_edges=(x[::2], x[::2]))
    launches = ctypes.c_int(-1)
    rc = _lib.load().gt4mi_horizontal_remap(hr._dst, hr._src, 9, ctypes.byref(hr._axis_i), ctypes.byref(hr._axis_j), 2, 8, _lib.HREMAP_PCM, 0,
                                            torch.cuda.current_stream().cuda_stream, ctypes.byref(launches))
    torch.cuda.synchronize()
    assert rc == 0 and launches.value == 2 and hr.launches == 2 and hr.terms == (8, 8)
    assert all(bool((d == float(n)).all()) for n, d in enumerate(dsts))
    horizontal.remap_cells(dsts[0], srcs[5], src_edges=(x, x), dst_edges=(x[::2], x[::2]), method="plm")  # the one-off form
    torch.cuda.synchronize()
    assert bool((dsts[0] == 5.0).all())
    del srcs[3]
    gc.collect()
    with pytest.raises(RuntimeError, match="no longer exists"):
        hr()
    torch.cuda.synchronize()
