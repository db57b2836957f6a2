"""``gt4py_amd.vertical`` -- columns from one set of levels to another, one kernel launch per 8 fields: conservative remapping
of cell means (:func:`remap_levels`) and interpolation of point values to run-time levels (:func:`interpolate_levels`).

A model on a Lagrangian or terrain-following vertical coordinate remaps its fields to fixed levels before output.  GTScript can
write that (a FORWARD sweep that carries a run-time source index, a ``while`` over the overlapping source cells, a read at a
run-time K index), but one field at a time; gt4py has no counterpart.  ``gt4mi_vertical_remap`` (csrc/vertical_remap.hip.h)
computes the overlaps and weights of a column once and applies them to up to eight fields in the same launch, on the current
stream, without synchronisation or allocation.

    from gt4py_amd import transfer, vertical
    vertical.remap_levels([u_p, v_p, t_p], [u, v, t], src_edges=z_model, dst_edges=z_fixed, method="plm")
    to_levels = vertical.VerticalRemap([u_p, v_p, t_p], [u, v, t], src_edges=z_model, dst_edges=z_fixed)  # frozen
    out = transfer.Download([u_p, v_p, t_p], dtype=np.float32)
    for step in range(steps):
        ...
        if step % n == 0:
            to_levels()          # enqueues; the download behind it on the same stream reads the remapped fields
            pending = out()

``src`` holds cell MEANS between the ``ns + 1`` edges of ``src_edges``, ``dst`` receives cell means between the ``nd + 1`` edges of
``dst_edges``; edges increase with k (negate a coordinate that decreases).  An edge field is an IJK field, or a ``Field[K]`` that
every column shares.  ``method`` is ``"pcm"`` (piecewise constant) or ``"plm"`` (piecewise linear with limited slopes: monotone).
Both conserve the column integral when the outer edges of the two sets coincide; a target cell that reaches outside the source
range sees the end cell's mean there.  The arithmetic -- float64 throughout, its order fixed -- is part of the contract
(include/gt4py_amd.h): the same column gives the same bits whatever the layout, the position in the call or the device.

Output on pressure, height or isentropic levels is not a remap: it is the POINT value of a field at a coordinate that differs from
column to column, linear in ``ln p``, missing below the ground; so is the vertical half of a semi-Lagrangian step, the value at a
run-time departure height.  ``gt4mi_vertical_interp`` (csrc/vertical_interp.hip.h) finds the bracket and the weights of a target
once and applies them to up to eight fields in the same launch.

    on_pressure = vertical.VerticalInterp([u_p, v_p, t_p], [u, v, t], src_coord=ln_p, dst_coord=ln_p_out, outside="fill")  # frozen
    depart = vertical.VerticalInterp([q_new], [q_star], src_coord=z, dst_coord=z_departure, method="cubic_monotone")

``src`` holds point values at the ``ns`` levels whose coordinate ``src_coord`` holds, strictly increasing with k (negate a coordinate
that decreases; pass ``ln p`` for interpolation that is linear in ``ln p``: the kernel computes no logarithm); ``dst`` receives the
values at the ``nd`` coordinates of ``dst_coord``, which may come in ANY order.  A coordinate field is an IJK field or a ``Field[K]``
that every column shares.  ``method`` is ``"nearest"``, ``"linear"``, ``"cubic"`` (Lagrange on the four surrounding levels, linear
in the two end intervals) or ``"cubic_monotone"`` (the cubic limited to the two bracketing values); ``outside`` says what a target
below the first or above the last source level gets: ``"clamp"`` (the end level's value), ``"linear"`` (the end interval's line,
extended) or ``"fill"`` (``fill_value``).  Again the arithmetic and its order are the contract, and a target's bits depend on
neither the other targets of its column nor their order.
"""

from __future__ import annotations

import ctypes
from typing import Optional, Sequence

from . import _lib
from ._bound import Bound, _float_pairs, _origin3, raise_refusal
from .storage.device_array import DeviceArray

METHODS = {"pcm": _lib.REMAP_PCM, "plm": _lib.REMAP_PLM}
INTERP_METHODS = {"nearest": _lib.VINTERP_NEAREST, "linear": _lib.VINTERP_LINEAR, "cubic": _lib.VINTERP_CUBIC,
                  "cubic_monotone": _lib.VINTERP_CUBIC_MONOTONE}
OUTSIDE = {"clamp": _lib.VINTERP_OUTSIDE_CLAMP, "linear": _lib.VINTERP_OUTSIDE_LINEAR, "fill": _lib.VINTERP_OUTSIDE_FILL}


def _native(dst, src, n: int, src_edges, dst_edges, extent_ij, ns: int, nd: int, size: int, edge_size: int, method: int, flags: int,
            stream: Optional[int]) -> int:
    """The ctypes call; a refusal of the library becomes ``ValueError`` (``TypeError`` for what no kernel handles) with the
    library's message.  Returns the kernels enqueued."""
    launches = ctypes.c_int(0)
    rc = _lib.load().gt4mi_vertical_remap(dst, src, n, ctypes.byref(src_edges), ctypes.byref(dst_edges), extent_ij, ns, nd, size,
                                          edge_size, method, flags, stream, ctypes.byref(launches))
    if rc != _lib.OK:
        raise_refusal("gt4mi_vertical_remap", rc)
    return launches.value


def _edge_field(a: DeviceArray, start) -> "_lib.Field":
    if a.ndim == 1:  # Field[K]: every column reads the same items
        return _lib.Field.make(a.ptr, (1, 1, a.shape[0]), (0, 0, a.strides[0]), (0, 0, start[2]))
    return _lib.Field.make(a.ptr, a.shape, a.strides, start)


class VerticalRemap(Bound):
    """The frozen form of :func:`remap_levels` (what ``FrozenStencil`` is for stencils): arguments are checked (through the
    library's dry run) and the native descriptors built once, ``__call__()`` makes only the ctypes call, on the stream that is
    current THEN.

    ``ns`` / ``nd`` are the source / target levels, ``extent`` the IJ box (the compute domain grown by the halo), ``launches`` the
    kernels a call enqueues.  The object holds raw pointers and weak references to the CALLER's objects, not the arrays: it
    refuses to run once one of them has died.  (An exporter that cannot be weakly referenced is held instead.)"""

    def __init__(self, dst, src, *, src_edges, dst_edges, method: str = "pcm", halo=0, origin: Optional[Sequence[int]] = None):
        dsts, srcs, d_arrays, s_arrays, e_arrays, self._halo = _float_pairs(
            "remap_levels", dst, src, halo, method, METHODS, shared=(src_edges, dst_edges), names=("src_edges", "dst_edges"), ndims=(1, 3),
            kind="Field[K]", plural="edge fields")
        self.method = method
        lo_i, hi_i, lo_j, hi_j = self._halo
        self.origin = origin = _origin3(origin, self._halo)
        # levels: what every src / dst has behind the origin; an edge field has one more
        levels = []
        for side, arrays, edges, name in (("sources", s_arrays, e_arrays[0], "src_edges"), ("destinations", d_arrays, e_arrays[1], "dst_edges")):
            n = arrays[0].shape[2] - origin[2]
            if n < 1:
                raise ValueError(f"origin {origin} leaves no level in the {side} (shape {arrays[0].shape})")
            for a in arrays:
                if a.shape[2] - origin[2] != n:
                    raise ValueError(f"the {side} of one call share their number of levels: {n} and {a.shape[2] - origin[2]} differ")
            have = edges.shape[-1] - origin[2]
            if have != n + 1:
                raise ValueError(f"{name} has {have} edges along K, {n} levels need {n + 1}")
            levels.append(n)
        self.ns, self.nd = levels
        # the common IJ compute domain: what every IJK array has left behind its origin and in front of its high ghost cells
        rest = [tuple(s - o - h for s, o, h in zip(a.shape[:2], origin[:2], (hi_i, hi_j))) for a in d_arrays + s_arrays + e_arrays if a.ndim == 3]
        domain = tuple(min(r[ax] for r in rest) for ax in range(2))
        if min(domain) < 0:
            raise ValueError(f"halo {self._halo} and origin {origin} leave no domain in fields of shapes {[a.shape for a in d_arrays + s_arrays]}")
        self.domain = domain
        #: the IJ box that is remapped: the domain grown by the halo
        self.extent = (domain[0] + lo_i + hi_i, domain[1] + lo_j + hi_j)
        start = (origin[0] - lo_i, origin[1] - lo_j, origin[2])
        self._n = len(d_arrays)
        self._dst, self._src = (_lib.Field * self._n)(), (_lib.Field * self._n)()
        for table, arrays in ((self._dst, d_arrays), (self._src, s_arrays)):
            for n, a in enumerate(arrays):
                table[n] = _lib.Field.make(a.ptr, a.shape, a.strides, start)
        self._src_edges, self._dst_edges = (_edge_field(a, start) for a in e_arrays)
        self._extent2 = (ctypes.c_int64 * 2)(*self.extent)
        self._size, self._edge_size, self._method = d_arrays[0].itemsize, e_arrays[0].itemsize, METHODS[method]
        # every check of the library, nothing enqueued; also: how many kernels
        self.launches = _native(self._dst, self._src, self._n, self._src_edges, self._dst_edges, self._extent2, self.ns, self.nd,
                                self._size, self._edge_size, self._method, _lib.REMAP_DRY_RUN, None)
        self._bind("remap_levels", d_arrays + s_arrays + e_arrays, dsts + srcs + [src_edges, dst_edges])

    def __call__(self) -> None:
        self._check_alive()
        rc = self._lib.gt4mi_vertical_remap(self._dst, self._src, self._n, ctypes.byref(self._src_edges), ctypes.byref(self._dst_edges),
                                            self._extent2, self.ns, self.nd, self._size, self._edge_size, self._method, 0,
                                            self._current_stream().cuda_stream, None)
        if rc != _lib.OK:
            _lib.check("gt4mi_vertical_remap", rc)


def remap_levels(dst, src, *, src_edges, dst_edges, method: str = "pcm", halo=0, origin: Optional[Sequence[int]] = None) -> None:
    """Remap the cell means ``src`` between the edges ``src_edges`` to cell means ``dst`` between the edges ``dst_edges``, column
    by column over the compute domain (plus ``halo`` ghost cells in I and J), in one kernel launch (per 8 pairs) on the current
    stream.

    ``dst``, ``src``  one field each or two sequences of equal length: IJK :class:`DeviceArray`\\ s of one dtype (float32 or
                float64) or anything ``as_device_array`` accepts; every field may differ in address, strides and padding.  The
                sources share their number of levels ``ns``, the destinations theirs ``nd``.
    ``src_edges``, ``dst_edges``  ``ns + 1`` / ``nd + 1`` edges along K, increasing: IJK fields or ``Field[K]`` (shared by every
                column), of one dtype (float32 or float64, not necessarily the fields').
    ``method``  ``"pcm"`` or ``"plm"``.
    ``halo``    an int, ``(hi, hj)`` or ``((lo_i, hi_i), (lo_j, hi_j))``, as for ``boundary.fill_halo``.
    ``origin``  first compute-domain point of every IJK array, default ``(lo_i, lo_j, 0)``.

    Raises ``ValueError`` / ``TypeError`` (with the library's message) before any GPU work.  For a time loop build a
    :class:`VerticalRemap` once instead."""
    VerticalRemap(dst, src, src_edges=src_edges, dst_edges=dst_edges, method=method, halo=halo, origin=origin)()


def _native_interp(dst, src, n: int, src_coord, dst_coord, extent_ij, ns: int, nd: int, size: int, coord_size: int, method: int,
                   outside: int, fill_value: float, flags: int, stream: Optional[int]) -> int:
    """The ctypes call of ``gt4mi_vertical_interp``, refusals as in :func:`_native`.  Returns the kernels enqueued."""
    launches = ctypes.c_int(0)
    rc = _lib.load().gt4mi_vertical_interp(dst, src, n, ctypes.byref(src_coord), ctypes.byref(dst_coord), extent_ij, ns, nd, size,
                                           coord_size, method, outside, fill_value, flags, stream, ctypes.byref(launches))
    if rc != _lib.OK:
        raise_refusal("gt4mi_vertical_interp", rc)
    return launches.value


class VerticalInterp(Bound):
    """The frozen form of :func:`interpolate_levels`: arguments are checked (through the library's dry run) and the native
    descriptors built once, ``__call__()`` makes only the ctypes call, on the stream that is current THEN.

    ``ns`` / ``nd`` are the source / target levels, ``extent`` the IJ box (the compute domain grown by the halo), ``launches`` the
    kernels a call enqueues, ``method`` and ``outside`` the names that were passed.  The object holds raw pointers and weak
    references to the CALLER's objects, not the arrays: it refuses to run once one of them has died.  (An exporter that cannot be
    weakly referenced is held instead.)"""

    def __init__(self, dst, src, *, src_coord, dst_coord, method: str = "linear", outside: str = "clamp", fill_value: float = float("nan"),
                 halo=0, origin: Optional[Sequence[int]] = None):
        dsts, srcs, d_arrays, s_arrays, c_arrays, self._halo = _float_pairs(
            "interpolate_levels", dst, src, halo, method, INTERP_METHODS, shared=(src_coord, dst_coord), names=("src_coord", "dst_coord"),
            ndims=(1, 3), kind="Field[K]", plural="coordinate fields")
        if outside not in OUTSIDE:
            raise ValueError(f"outside must be one of {sorted(OUTSIDE)}, not {outside!r}")
        if isinstance(fill_value, bool) or not isinstance(fill_value, (int, float)):
            raise TypeError(f"fill_value must be a Python float, not {type(fill_value).__name__}")
        self.method, self.outside, self.fill_value = method, outside, float(fill_value)
        lo_i, hi_i, lo_j, hi_j = self._halo
        self.origin = origin = _origin3(origin, self._halo)
        # levels: what every src / dst has behind the origin; a coordinate field has as many
        levels = []
        for side, arrays, coord, name in (("sources", s_arrays, c_arrays[0], "src_coord"), ("destinations", d_arrays, c_arrays[1], "dst_coord")):
            n = arrays[0].shape[2] - origin[2]
            if n < 1:
                raise ValueError(f"origin {origin} leaves no level in the {side} (shape {arrays[0].shape})")
            for a in arrays:
                if a.shape[2] - origin[2] != n:
                    raise ValueError(f"the {side} of one call share their number of levels: {n} and {a.shape[2] - origin[2]} differ")
            have = coord.shape[-1] - origin[2]
            if have != n:
                raise ValueError(f"{name} has {have} levels along K, the {side} have {n}")
            levels.append(n)
        self.ns, self.nd = levels
        # the common IJ compute domain: what every IJK array has left behind its origin and in front of its high ghost cells
        rest = [tuple(s - o - h for s, o, h in zip(a.shape[:2], origin[:2], (hi_i, hi_j))) for a in d_arrays + s_arrays + c_arrays if a.ndim == 3]
        domain = tuple(min(r[ax] for r in rest) for ax in range(2))
        if min(domain) < 0:
            raise ValueError(f"halo {self._halo} and origin {origin} leave no domain in fields of shapes {[a.shape for a in d_arrays + s_arrays]}")
        self.domain = domain
        #: the IJ box that is interpolated: the domain grown by the halo
        self.extent = (domain[0] + lo_i + hi_i, domain[1] + lo_j + hi_j)
        start = (origin[0] - lo_i, origin[1] - lo_j, origin[2])
        self._n = len(d_arrays)
        self._dst, self._src = (_lib.Field * self._n)(), (_lib.Field * self._n)()
        for table, arrays in ((self._dst, d_arrays), (self._src, s_arrays)):
            for n, a in enumerate(arrays):
                table[n] = _lib.Field.make(a.ptr, a.shape, a.strides, start)
        self._src_coord, self._dst_coord = (_edge_field(a, start) for a in c_arrays)
        self._extent2 = (ctypes.c_int64 * 2)(*self.extent)
        self._size, self._coord_size = d_arrays[0].itemsize, c_arrays[0].itemsize
        self._method, self._outside = INTERP_METHODS[method], OUTSIDE[outside]
        # every check of the library, nothing enqueued; also: how many kernels
        self.launches = _native_interp(self._dst, self._src, self._n, self._src_coord, self._dst_coord, self._extent2, self.ns, self.nd,
                                       self._size, self._coord_size, self._method, self._outside, self.fill_value, _lib.VINTERP_DRY_RUN, None)
        self._bind("interpolate_levels", d_arrays + s_arrays + c_arrays, dsts + srcs + [src_coord, dst_coord])

    def __call__(self) -> None:
        self._check_alive()
        rc = self._lib.gt4mi_vertical_interp(self._dst, self._src, self._n, ctypes.byref(self._src_coord), ctypes.byref(self._dst_coord),
                                             self._extent2, self.ns, self.nd, self._size, self._coord_size, self._method, self._outside,
                                             self.fill_value, 0, self._current_stream().cuda_stream, None)
        if rc != _lib.OK:
            _lib.check("gt4mi_vertical_interp", rc)


def interpolate_levels(dst, src, *, src_coord, dst_coord, method: str = "linear", outside: str = "clamp", fill_value: float = float("nan"),
                       halo=0, origin: Optional[Sequence[int]] = None) -> None:
    """Write to level m of every column of ``dst`` the value of ``src`` at the coordinate ``dst_coord[m]`` of that column, ``src``
    given at the coordinates ``src_coord``, over the compute domain (plus ``halo`` ghost cells in I and J), in one kernel launch
    (per 8 pairs) on the current stream.

    ``dst``, ``src``  one field each or two sequences of equal length: IJK :class:`DeviceArray`\\ s of one dtype (float32 or
                float64) or anything ``as_device_array`` accepts; every field may differ in address, strides and padding.  The
                sources share their number of levels ``ns`` (at least 2), the destinations theirs ``nd``.
    ``src_coord``  the coordinate of the ``ns`` source levels, strictly increasing with k (negate one that decreases).
    ``dst_coord``  the coordinate of the ``nd`` target levels, in any order.  Both are IJK fields or ``Field[K]`` (shared by every
                column), of one dtype (float32 or float64, not necessarily the fields').
    ``method``  ``"nearest"``, ``"linear"``, ``"cubic"`` or ``"cubic_monotone"``.
    ``outside``  what a target below ``src_coord[0]`` or above ``src_coord[ns-1]`` gets: ``"clamp"`` the end level's value,
                ``"linear"`` the end interval's line, extended, ``"fill"`` ``fill_value``.
    ``fill_value``  a Python float, rounded once to the fields' dtype; NaN (the default) is stored as the canonical quiet NaN.
    ``halo``    an int, ``(hi, hj)`` or ``((lo_i, hi_i), (lo_j, hi_j))``, as for ``boundary.fill_halo``.
    ``origin``  first compute-domain point of every IJK array, default ``(lo_i, lo_j, 0)``.

    Raises ``ValueError`` / ``TypeError`` (with the library's message) before any GPU work.  For a time loop build a
    :class:`VerticalInterp` once instead."""
    VerticalInterp(dst, src, src_coord=src_coord, dst_coord=dst_coord, method=method, outside=outside, fill_value=fill_value, halo=halo,
                   origin=origin)()
