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
from ._bound import FLAGS, STREAM, Bound, Out, _common_domain, _float_pairs, _origin3, field_table
from .storage.device_array import DeviceArray

METHODS = {"pcm": _lib.REMAP_PCM, "plm": _lib.REMAP_PLM}
INTERP_METHODS = {"nearest": _lib.VINTERP_NEAREST, "linear": _lib.VINTERP_LINEAR, "cubic": _lib.VINTERP_CUBIC,
                  "cubic_monotone": _lib.VINTERP_CUBIC_MONOTONE}
OUTSIDE = {"clamp": _lib.VINTERP_OUTSIDE_CLAMP, "linear": _lib.VINTERP_OUTSIDE_LINEAR, "fill": _lib.VINTERP_OUTSIDE_FILL}


def _shared_field(a: DeviceArray, start) -> "_lib.Field":
    if a.ndim == 1:  # Field[K]: every column reads the same items
        return _lib.Field.make(a.ptr, (1, 1, a.shape[0]), (0, 0, a.strides[0]), (0, 0, start[2]))
    return _lib.Field.make(a.ptr, a.shape, a.strides, start)


class _Columns(Bound):
    """What :class:`VerticalRemap` and :class:`VerticalInterp` share: (dst, src) pairs of IJK fields and two shared fields along K,
    one for the source levels and one for the target levels.  A subclass states its entry, its methods, what it calls itself and
    its shared fields, how many more items than levels a shared field has, and its scalars behind ``method``."""

    _who = ""
    _methods: dict = {}
    _names = ("", "")  # the shared fields: the keyword of the sources' one and of the targets' one
    _plural = ""       # what the dtype message calls them
    _surplus = 0       # items a shared field has along K beyond the levels: 1 for edges, 0 for coordinates

    def _wrong_count(self, name: str, have: int, n: int, side: str) -> str:
        """The message for a shared field ``name`` of ``have`` items along K where the ``side`` have ``n`` levels."""
        raise NotImplementedError

    def _scalars(self, **own) -> tuple:
        """Checks the subclass's own keywords and returns the native arguments between ``method`` and the flags."""
        return ()

    def _arguments(self) -> tuple:
        return (self._dst, self._src, self._n, *self._shared_refs, self._extent2, self.ns, self.nd, self._size, self._shared_size,
                self._method, *self._own, FLAGS, STREAM, Out(ctypes.c_int))

    def _columns(self, dst, src, shared, method: str, halo, origin, **own) -> None:
        dsts, srcs, d_arrays, s_arrays, x_arrays, self._halo = _float_pairs(
            self._who, dst, src, halo, method, self._methods, shared=shared, names=self._names, ndims=(1, 3), kind="Field[K]",
            plural=self._plural)
        self.method = method
        self._own = self._scalars(**own)
        lo_i, hi_i, lo_j, hi_j = self._halo
        self.origin = origin = _origin3(origin, self._halo)
        # levels: what every src / dst has behind the origin; a shared field has `_surplus` more
        levels = []
        for side, arrays, x, name in (("sources", s_arrays, x_arrays[0], self._names[0]), ("destinations", d_arrays, x_arrays[1], self._names[1])):
            n = arrays[0].shape[2] - origin[2]
            if n < 1:
                raise ValueError(f"origin {origin} leaves no level in the {side} (shape {arrays[0].shape})")
            for a in arrays:
                if a.shape[2] - origin[2] != n:
                    raise ValueError(f"the {side} of one call share their number of levels: {n} and {a.shape[2] - origin[2]} differ")
            have = x.shape[-1] - origin[2]
            if have != n + self._surplus:
                raise ValueError(self._wrong_count(name, have, n, side))
            levels.append(n)
        self.ns, self.nd = levels
        # the common IJ compute domain of the IJK arrays (a Field[K] has none)
        self.domain = domain = _common_domain([a for a in d_arrays + s_arrays + x_arrays if a.ndim == 3], self._halo, origin,
                                              d_arrays + s_arrays, axes=2)
        #: the IJ box that is written: the domain grown by the halo
        self.extent = (domain[0] + lo_i + hi_i, domain[1] + lo_j + hi_j)
        start = (origin[0] - lo_i, origin[1] - lo_j, origin[2])
        self._n = len(d_arrays)
        self._dst, self._src = field_table(d_arrays, start), field_table(s_arrays, start)
        fields = [_shared_field(a, start) for a in x_arrays]
        for name, f in zip(self._names, fields):  # (the descriptors under the shared fields' names: `_src_edges`, `_dst_coord`, ...)
            setattr(self, "_" + name, f)
        self._shared_refs = tuple(ctypes.byref(f) for f in fields)
        self._extent2 = (ctypes.c_int64 * 2)(*self.extent)
        self._size, self._shared_size, self._method = d_arrays[0].itemsize, x_arrays[0].itemsize, self._methods[method]
        # every check of the library, nothing enqueued; also: how many kernels
        self.launches, = self._dry_run()
        self._bind(self._who, d_arrays + s_arrays + x_arrays, dsts + srcs + list(shared))


class VerticalRemap(_Columns):
    """The frozen form of :func:`remap_levels` (what ``FrozenStencil`` is for stencils): arguments are checked (through the
    library's dry run) and the native descriptors built once, ``__call__()`` makes only the ctypes call, on the stream that is
    current THEN.

    ``ns`` / ``nd`` are the source / target levels, ``extent`` the IJ box (the compute domain grown by the halo), ``launches`` the
    kernels a call enqueues.  The object holds raw pointers and weak references to the CALLER's objects, not the arrays: it
    refuses to run once one of them has died.  (An exporter that cannot be weakly referenced is held instead.)"""

    _who, _entry, _dry_run_bit, _methods = "remap_levels", "gt4mi_vertical_remap", _lib.REMAP_DRY_RUN, METHODS
    _names, _plural, _surplus = ("src_edges", "dst_edges"), "edge fields", 1

    def _wrong_count(self, name: str, have: int, n: int, side: str) -> str:
        return f"{name} has {have} edges along K, {n} levels need {n + 1}"

    def __init__(self, dst, src, *, src_edges, dst_edges, method: str = "pcm", halo=0, origin: Optional[Sequence[int]] = None):
        self._columns(dst, src, (src_edges, dst_edges), method, halo, origin)


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


class VerticalInterp(_Columns):
    """The frozen form of :func:`interpolate_levels`: arguments are checked (through the library's dry run) and the native
    descriptors built once, ``__call__()`` makes only the ctypes call, on the stream that is current THEN.

    ``ns`` / ``nd`` are the source / target levels, ``extent`` the IJ box (the compute domain grown by the halo), ``launches`` the
    kernels a call enqueues, ``method`` and ``outside`` the names that were passed.  The object holds raw pointers and weak
    references to the CALLER's objects, not the arrays: it refuses to run once one of them has died.  (An exporter that cannot be
    weakly referenced is held instead.)"""

    _who, _entry, _dry_run_bit, _methods = "interpolate_levels", "gt4mi_vertical_interp", _lib.VINTERP_DRY_RUN, INTERP_METHODS
    _names, _plural, _surplus = ("src_coord", "dst_coord"), "coordinate fields", 0

    def _wrong_count(self, name: str, have: int, n: int, side: str) -> str:
        return f"{name} has {have} levels along K, the {side} have {n}"

    def _scalars(self, outside, fill_value) -> tuple:
        if outside not in OUTSIDE:
            raise ValueError(f"outside must be one of {sorted(OUTSIDE)}, not {outside!r}")
        if isinstance(fill_value, bool) or not isinstance(fill_value, (int, float)):
            raise TypeError(f"fill_value must be a Python float, not {type(fill_value).__name__}")
        self.outside, self.fill_value = outside, float(fill_value)
        return OUTSIDE[outside], self.fill_value

    def __init__(self, dst, src, *, src_coord, dst_coord, method: str = "linear", outside: str = "clamp", fill_value: float = float("nan"),
                 halo=0, origin: Optional[Sequence[int]] = None):
        self._columns(dst, src, (src_coord, dst_coord), method, halo, origin, outside=outside, fill_value=fill_value)


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
