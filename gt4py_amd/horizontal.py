"""``gt4py_amd.horizontal`` -- the value of fields at run-time horizontal positions (:func:`interpolate`) and their cell means on
another rectilinear grid (:func:`remap_cells`), one kernel launch per 8 fields.

GTScript takes compile-time horizontal offsets only (only K may be indexed at run time), so "the value of a field at a point whose
I / J position is data" -- the departure-point interpolation of a semi-Lagrangian step, sampling on a rotated, shifted or nested
grid, tracing back along a velocity field -- cannot be written as a stencil; gt4py leaves it to fancy indexing on its numpy / cupy
storages.  ``gt4mi_horizontal_interp`` (csrc/horizontal_interp.hip.h) computes the indices and weights of a point once and applies
them to up to eight fields in the same launch, on the current stream, without synchronisation or allocation.

    from gt4py_amd import boundary, horizontal
    fill = boundary.HaloFill([q, t], halo=3, mode="periodic")
    advect = horizontal.HorizontalInterp([q_new, t_new], [q, t], pos_i=di, pos_j=dj, relative=True,
                                         method="cubic_monotone", halo=3)              # frozen
    for step in range(steps):
        displacements(u, v, di, dj, dt_dx=dt / dx, dt_dy=dt / dy)   # a stencil: di = -u * dt / dx, dj = -v * dt / dy
        fill()
        advect()                                                    # q_new(i, j, k) = q at (i + di, j + dj), level k
        physics(q_new, t_new, ...)                                  # the next stencil, in stream order

``pos_i`` / ``pos_j`` hold, for every point of the compute domain, a position in index units of the domain (0.0 is domain point 0)
or, with ``relative=True``, a displacement from the point's own index -- what a stencil can produce, which has no I or J as a
value.  They are IJK fields or ``Field[IJ]`` (one flow for every level), float32 or float64 whatever the fields are.  ``halo`` is
how far the gather may reach into ``src``'s ghost cells; positions beyond it are clamped to it (edge replication), so on a
decomposed run the halo width is the Courant limit.  ``method`` is ``"nearest"``, ``"linear"``, ``"cubic"`` (Lagrange) or
``"cubic_monotone"`` (the cubic limited to the range of the four surrounding items: the quasi-monotone limiter of semi-Lagrangian
schemes).  The arithmetic -- float64 throughout, its order fixed -- is part of the contract (include/gt4py_amd.h): the same point
gives the same bits whatever the layout, the position in the call or the device.

Point sampling neither conserves nor averages.  ``gt4mi_horizontal_remap`` (csrc/horizontal_remap.hip.h) takes cell MEANS on one
rectilinear grid to cell means on another -- coarser, finer or shifted: output at reduced resolution, a nest and its parent, the
restriction and prolongation of a multigrid cycle --, which no stencil can write (a destination point reads sources at compile-time
constant offsets only, never ``2*i`` or a source of another shape).  The grids are four 1-d HOST arrays of edges, fixed for the
life of the frozen call; the geometry is two small per-axis overlap tables computed once on the host.

    coarsen = horizontal.HorizontalRemap([u_c, v_c, t_c], [u, v, t], src_edges=(x, y), dst_edges=(x_out, y_out), method="plm")
    out = transfer.Download([u_c, v_c, t_c], dtype=np.float32)
    for step in range(steps):
        ...
        if step % n == 0:
            coarsen()            # enqueues; the download behind it on the same stream reads the coarse fields
            pending = out()

``method`` is ``"pcm"`` (piecewise constant) or ``"plm"`` (piecewise linear, slopes limited per axis).  Both conserve the integral
when the outer edges of the two grids coincide; a destination cell that reaches outside the source grid sees the end cell's mean
there.
"""

from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._bound import FLAGS, FLOATS, STREAM, Bound, Out, _common_domain, _float_pairs, _origin3, _pair_lists, _triple, field_table, raise_refusal
from .storage.device_array import DeviceArray

METHODS = {"nearest": _lib.INTERP_NEAREST, "linear": _lib.INTERP_LINEAR, "cubic": _lib.INTERP_CUBIC,
           "cubic_monotone": _lib.INTERP_CUBIC_MONOTONE}


def _position_field(a: DeviceArray, origin) -> "_lib.Field":
    if a.ndim == 2:  # Field[IJ]: every level reads the same items
        return _lib.Field.make(a.ptr, (a.shape[0], a.shape[1], 1), (a.strides[0], a.strides[1], 0), (origin[0], origin[1], 0))
    return _lib.Field.make(a.ptr, a.shape, a.strides, origin)


class HorizontalInterp(Bound):
    """The frozen form of :func:`interpolate` (what ``FrozenStencil`` is for stencils): arguments are checked (through the
    library's dry run) and the native descriptors built once, ``__call__()`` makes only the ctypes call, on the stream that is
    current THEN.

    ``domain`` is the box that is written (every point of it in every dst), ``method`` the method's name, ``launches`` the kernels
    a call enqueues.  The object holds raw pointers and weak references to the CALLER's objects, not the arrays: it refuses to
    run once one of them has died.  (An exporter that cannot be weakly referenced is held instead.)"""

    _entry, _dry_run_bit = "gt4mi_horizontal_interp", _lib.INTERP_DRY_RUN

    def _arguments(self) -> tuple:
        return (self._dst, self._src, self._n, ctypes.byref(self._pos_i), ctypes.byref(self._pos_j), self._extent, self._reach, self._size,
                self._pos_size, self._method, FLAGS, STREAM, Out(ctypes.c_int))

    def __init__(self, dst, src, *, pos_i, pos_j, method: str = "linear", relative: bool = False, halo=0,
                 origin: Optional[Sequence[int]] = None):
        dsts, srcs, d_arrays, s_arrays, p_arrays, self._halo = _float_pairs(
            "interpolate", dst, src, halo, method, METHODS, shared=(pos_i, pos_j), names=("pos_i", "pos_j"), ndims=(2, 3), kind="Field[IJ]",
            plural="position fields")
        self.method, self.relative = method, bool(relative)
        self.origin = origin = _origin3(origin, self._halo)
        self.domain = domain = _common_domain(d_arrays + s_arrays + p_arrays, self._halo, origin, d_arrays + s_arrays)
        self._n = len(d_arrays)
        self._dst, self._src = field_table(d_arrays, origin), field_table(s_arrays, origin)
        self._pos_i, self._pos_j = (_position_field(a, origin) for a in p_arrays)
        self._extent = _lib.domain3(domain)
        self._reach = (ctypes.c_int64 * 4)(*self._halo)
        self._size, self._pos_size, self._method = d_arrays[0].itemsize, p_arrays[0].itemsize, METHODS[method]
        self._flags = _lib.INTERP_RELATIVE if self.relative else 0
        # every check of the library, nothing enqueued; also: how many kernels
        self.launches, = self._dry_run()
        self._bind("interpolate", d_arrays + s_arrays + p_arrays, dsts + srcs + [pos_i, pos_j])


def interpolate(dst, src, *, pos_i, pos_j, method: str = "linear", relative: bool = False, halo=0,
                origin: Optional[Sequence[int]] = None) -> None:
    """Write to every point (i, j, k) of the compute domain of ``dst`` the value of ``src`` at level k and the horizontal position
    that ``pos_i`` / ``pos_j`` hold for that point, in one kernel launch (per 8 pairs) on the current stream.

    ``dst``, ``src``  one field each or two sequences of equal length: IJK :class:`DeviceArray`\\ s of one dtype (float32 or
                float64) or anything ``as_device_array`` accepts; every field may differ in address, strides and padding.  A dst
                must not share memory with a src, a position field or another dst.
    ``pos_i``, ``pos_j``  IJK fields or ``Field[IJ]`` (shared by every level), of one dtype (float32 or float64, not necessarily
                the fields'): positions in index units of the compute domain, 0.0 = domain point 0.
    ``method``  ``"nearest"``, ``"linear"``, ``"cubic"`` or ``"cubic_monotone"``.
    ``relative``  the position fields hold displacements from each point's own index.
    ``halo``    an int, ``(hi, hj)`` or ``((lo_i, hi_i), (lo_j, hi_j))``, as for ``boundary.fill_halo``: how far the gather may
                reach into ``src``'s ghost cells.  Positions (and stencil points) beyond it are clamped to it.
    ``origin``  first compute-domain point of every array, default ``(lo_i, lo_j, 0)``.

    Raises ``ValueError`` / ``TypeError`` (with the library's message) before any GPU work.  For a time loop build a
    :class:`HorizontalInterp` once instead."""
    HorizontalInterp(dst, src, pos_i=pos_i, pos_j=pos_j, method=method, relative=relative, halo=halo, origin=origin)()


# ---- conservative remapping between rectilinear grids ---------------------------------------------------------------------------
REMAP_METHODS = {"pcm": _lib.HREMAP_PCM, "plm": _lib.HREMAP_PLM}


def overlap_table(src_edges, dst_edges):
    """The overlap table of one axis (``gt4mi_overlap_table``, host code): ``(ptr, cell, w, h, c, den)`` as numpy arrays, int32 /
    int32 / float64 x 4; the terms of destination cell ``m`` are ``ptr[m] .. ptr[m + 1]``."""
    xs, xd = (np.ascontiguousarray(e, dtype=np.float64) for e in (src_edges, dst_edges))
    ns, nd = xs.size - 1, xd.size - 1
    capacity = max(ns + nd - 1, 1)
    ptr, cell = np.zeros(max(nd, 0) + 1, dtype=np.int32), np.zeros(capacity, dtype=np.int32)
    w, h, c, den = (np.zeros(capacity, dtype=np.float64) for _ in range(4))
    nnz = ctypes.c_int(0)
    rc = _lib.load().gt4mi_overlap_table(xs.ctypes.data, ns, xd.ctypes.data, nd, ptr.ctypes.data, cell.ctypes.data, w.ctypes.data,
                                         h.ctypes.data, c.ctypes.data, den.ctypes.data, capacity, ctypes.byref(nnz))
    if rc != _lib.OK:
        raise_refusal("gt4mi_overlap_table", rc)
    return (ptr,) + tuple(a[: nnz.value] for a in (cell, w, h, c, den))


def _edge_pair(edges, name: str):
    if not isinstance(edges, (tuple, list)) or len(edges) != 2:
        raise ValueError(f"{name} must be a pair (edges along I, edges along J)")
    out = []
    for axis, e in zip("IJ", edges):
        try:
            e = np.array(e, dtype=np.float64)  # (a copy: the edges are fixed for the life of the call)
        except (TypeError, ValueError):
            raise TypeError(f"{name} along {axis} must be a 1-d host array-like of numbers") from None
        if e.ndim != 1 or e.size < 2:
            raise ValueError(f"{name} along {axis} must be a 1-d array of at least 2 edges, not an array of shape {e.shape}")
        out.append(e)
    return out


class HorizontalRemap(Bound):
    """The frozen form of :func:`remap_cells`: arguments are checked, the two overlap tables computed on the host
    (``gt4mi_overlap_table``) and copied to device arrays that the object OWNS, the library's dry run made and the native
    descriptors built once; ``__call__()`` makes only the ctypes call, on the stream that is current THEN.

    ``src_extent`` / ``dst_extent`` are the (I, J) cells of the two grids, ``nk`` the levels, ``terms`` the table entries per axis,
    ``launches`` the kernels a call enqueues.  The object holds raw pointers and weak references to the CALLER's fields, not the
    arrays: it refuses to run once one of them has died.  (An exporter that cannot be weakly referenced is held instead.)"""

    _entry, _dry_run_bit = "gt4mi_horizontal_remap", _lib.HREMAP_DRY_RUN

    def _arguments(self) -> tuple:
        return (self._dst, self._src, self._n, ctypes.byref(self._axis_i), ctypes.byref(self._axis_j), self.nk, self._size, self._method,
                FLAGS, STREAM, Out(ctypes.c_int))

    def __init__(self, dst, src, *, src_edges, dst_edges, method: str = "pcm", src_origin: Optional[Sequence[int]] = None,
                 dst_origin: Optional[Sequence[int]] = None):
        dsts, srcs, d_arrays, s_arrays, _, _ = _pair_lists("remap_cells", dst, src, 0, method, REMAP_METHODS)
        for a in d_arrays + s_arrays:
            if a.ndim != 3:
                raise ValueError(f"remap_cells takes IJK fields, not a field of {a.ndim} dimension(s)")
        dtype = d_arrays[0].dtype
        for a in d_arrays + s_arrays:
            if a.dtype != dtype:
                raise TypeError(f"the fields of one call share a dtype: {dtype} and {a.dtype} differ")
        if dtype not in FLOATS:
            raise TypeError(f"remap_cells takes float32 or float64 fields, not {dtype}")
        self.method = method
        xs, xd = _edge_pair(src_edges, "src_edges"), _edge_pair(dst_edges, "dst_edges")
        self.src_extent, self.dst_extent = tuple(e.size - 1 for e in xs), tuple(e.size - 1 for e in xd)
        self.src_origin = s_origin = (0, 0, 0) if src_origin is None else _triple(src_origin, "src_origin", 0)
        self.dst_origin = d_origin = (0, 0, 0) if dst_origin is None else _triple(dst_origin, "dst_origin", 0)
        # levels: what every field has behind its origin along K; cells: what the edges say must fit behind the origin in I and J
        levels = {a.shape[2] - org[2] for arrays, org in ((d_arrays, d_origin), (s_arrays, s_origin)) for a in arrays}
        if len(levels) != 1:
            raise ValueError(f"the fields of one call share their number of levels behind the origin: {sorted(levels)} differ")
        self.nk = levels.pop()
        if self.nk < 1:
            raise ValueError(f"origins {d_origin} (dst) / {s_origin} (src) leave no level in fields of shapes {[a.shape for a in d_arrays + s_arrays]}")
        for side, arrays, org, extent in (("dst", d_arrays, d_origin, self.dst_extent), ("src", s_arrays, s_origin, self.src_extent)):
            for n, a in enumerate(arrays):
                for ax in range(2):
                    if org[ax] < 0 or org[ax] + extent[ax] > a.shape[ax]:
                        raise ValueError(f"{side}_edges along {'IJ'[ax]} has {extent[ax] + 1} edges: {extent[ax]} cells from origin {org[ax]} do "
                                         f"not match {side} {n} of shape {a.shape}")
        tables = [overlap_table(s, d) for s, d in zip(xs, xd)]  # (refuses edges that are not finite and strictly increasing)
        self.terms = tuple(int(t[1].size) for t in tables)
        import torch

        device = d_arrays[0].tensor.device
        self._tables, axes = [], []
        for (ptr, cell, *reals), ns, nd in zip(tables, self.src_extent, self.dst_extent):
            ints = torch.from_numpy(np.concatenate([ptr, cell])).to(device)
            real = torch.from_numpy(np.concatenate(reals)).to(device)
            self._tables += [ints, real]
            nnz = cell.size
            axes.append(_lib.OverlapAxis(ns, nd, nnz, ints.data_ptr(), ints.data_ptr() + 4 * (nd + 1),
                                         *[real.data_ptr() + 8 * nnz * m for m in range(4)]))
        self._axis_i, self._axis_j = axes
        self._n = len(d_arrays)
        self._dst, self._src = field_table(d_arrays, d_origin), field_table(s_arrays, s_origin)
        self._size, self._method = d_arrays[0].itemsize, REMAP_METHODS[method]
        # every check of the library, nothing enqueued; also: how many kernels
        self.launches, = self._dry_run()
        self._bind("remap_cells", d_arrays + s_arrays, dsts + srcs)


def remap_cells(dst, src, *, src_edges, dst_edges, method: str = "pcm", src_origin: Optional[Sequence[int]] = None,
                dst_origin: Optional[Sequence[int]] = None) -> None:
    """Remap the cell means ``src`` on the rectilinear grid ``src_edges`` to cell means ``dst`` on the grid ``dst_edges``, level by
    level, in one kernel launch (per 8 pairs) on the current stream.

    ``dst``, ``src``  one field each or two sequences of equal length: IJK :class:`DeviceArray`\\ s of one dtype (float32 or
                float64) or anything ``as_device_array`` accepts; every field may differ in address, strides and padding, the
                sources have one horizontal shape and the destinations another.  A dst must not share memory with a src or
                another dst.
    ``src_edges``, ``dst_edges``  pairs ``(edges along I, edges along J)`` of 1-d HOST array-likes, converted to float64: finite,
                strictly increasing, ``cells + 1`` each.  The boxes they describe start at the origins.
    ``method``  ``"pcm"`` or ``"plm"``.
    ``src_origin``, ``dst_origin``  first cell of the grid in every src / dst, default ``(0, 0, 0)``; all fields have the same
                number of levels ``nk`` behind their origin.

    Raises ``ValueError`` / ``TypeError`` (with the library's message) before any GPU work.  For a time loop build a
    :class:`HorizontalRemap` once instead."""
    HorizontalRemap(dst, src, src_edges=src_edges, dst_edges=dst_edges, method=method, src_origin=src_origin, dst_origin=dst_origin)()
