"""``gt4py_amd.departure`` -- the value of fields at run-time positions that moved in all three directions
(:func:`interpolate_3d`), one kernel launch per 8 fields.

The departure point of a semi-Lagrangian step lies off the arrival point's level AND off its column.  ``horizontal.HorizontalInterp``
gathers on a point's own level and ``vertical.VerticalInterp`` in a point's own column; chaining them does not give the 3-D value,
because the column the vertical step reads is the one at (i, j), not the one at the horizontal departure position.
``gt4mi_departure_interp`` (csrc/departure_interp.hip.h) computes the three sets of indices and weights of a point once and
applies them to up to eight fields in the same launch, on the current stream, without synchronisation or allocation.

    from gt4py_amd import boundary, departure
    fill = boundary.HaloFill([q, t], halo=3, mode="periodic")
    advect = departure.DepartureInterp([q_new, t_new], [q, t], pos_i=di, pos_j=dj, pos_k=dk, relative=True,
                                       method="cubic_monotone", halo=3)                # frozen
    for step in range(steps):
        displacements(u, v, w, di, dj, dk, dt_dx=dt / dx, dt_dy=dt / dy, dt_dz=dt / dz)   # a stencil: di = -u * dt / dx, ...
        fill()
        advect()                                           # q_new(i, j, k) = q at (i + di, j + dj, k + dk)
        physics(q_new, t_new, ...)                         # the next stencil, in stream order

``pos_i`` / ``pos_j`` / ``pos_k`` hold, for every point of the compute domain, a position in index units of the domain (0.0 is
domain point 0, or level 0) or, with ``relative=True``, a displacement from the point's own index on each of the three axes.
``pos_i`` and ``pos_j`` are IJK fields or ``Field[IJ]`` (one horizontal flow for every level), ``pos_k`` is an IJK field; all three
share a dtype, float32 or float64 whatever the fields are.  ``halo`` is how far the gather may reach into ``src``'s ghost cells
along I and J; positions beyond it are clamped to it (edge replication).  K has no ghost levels: ``pos_k`` is clamped to
``[0, nk - 1]``.  ``method`` is ``"nearest"``, ``"linear"`` (trilinear), ``"cubic"`` (Lagrange; along K the rule of
``vertical.VerticalInterp``: the four-level formula where four levels surround the point, linear over the two cubic plane values in
the end intervals) or ``"cubic_monotone"`` (the cubic limited to the range of the eight surrounding items).  The arithmetic --
float64 throughout, its order fixed -- is part of the contract (include/gt4py_amd.h): the same point gives the same bits whatever
the layout, the position in the call or the device.

A physical vertical coordinate (height, pressure) is not an index: convert it to a fractional level in a stencil, or interpolate to
levels with ``vertical.VerticalInterp`` first.
"""

from __future__ import annotations

import ctypes
from typing import Optional, Sequence

from . import _lib
from ._bound import FLAGS, STREAM, Bound, Out, _common_domain, _float_pairs, _origin3, field_table
from .horizontal import METHODS, _position_field


class DepartureInterp(Bound):
    """The frozen form of :func:`interpolate_3d` (what ``FrozenStencil`` is for stencils): arguments are checked (through the
    library's dry run) and the native descriptors built once, ``__call__()`` makes only the ctypes call, on the stream that is
    current THEN.

    ``domain`` is the box that is written (every point of it in every dst), ``origin`` its first point in every array, ``method``
    the method's name, ``relative`` whether the positions are displacements, ``launches`` the kernels a call enqueues.  The object
    holds raw pointers and weak references to the CALLER's objects, not the arrays: it refuses to run once one of them has died.
    (An exporter that cannot be weakly referenced is held instead.)"""

    _entry, _dry_run_bit = "gt4mi_departure_interp", _lib.INTERP_DRY_RUN

    def _arguments(self) -> tuple:
        return (self._dst, self._src, self._n, ctypes.byref(self._pos_i), ctypes.byref(self._pos_j), ctypes.byref(self._pos_k), self._extent,
                self._reach, self._size, self._pos_size, self._method, FLAGS, STREAM, Out(ctypes.c_int))

    def __init__(self, dst, src, *, pos_i, pos_j, pos_k, method: str = "linear", relative: bool = False, halo=0,
                 origin: Optional[Sequence[int]] = None):
        dsts, srcs, d_arrays, s_arrays, p_arrays, self._halo = _float_pairs(
            "interpolate_3d", dst, src, halo, method, METHODS, shared=(pos_i, pos_j, pos_k), names=("pos_i", "pos_j", "pos_k"),
            ndims=((2, 3), (2, 3), (3,)), kind="Field[IJ]", plural="position fields")
        self.method, self.relative = method, bool(relative)
        self.origin = origin = _origin3(origin, self._halo)
        self.domain = domain = _common_domain(d_arrays + s_arrays + p_arrays, self._halo, origin, d_arrays + s_arrays)
        self._n = len(d_arrays)
        self._dst, self._src = field_table(d_arrays, origin), field_table(s_arrays, origin)
        self._pos_i, self._pos_j, self._pos_k = (_position_field(a, origin) for a in p_arrays)
        self._extent = _lib.domain3(domain)
        self._reach = (ctypes.c_int64 * 4)(*self._halo)
        self._size, self._pos_size, self._method = d_arrays[0].itemsize, p_arrays[0].itemsize, METHODS[method]
        self._flags = _lib.INTERP_RELATIVE if self.relative else 0
        # every check of the library, nothing enqueued; also: how many kernels
        self.launches, = self._dry_run()
        self._bind("interpolate_3d", d_arrays + s_arrays + p_arrays, dsts + srcs + [pos_i, pos_j, pos_k])


def interpolate_3d(dst, src, *, pos_i, pos_j, pos_k, method: str = "linear", relative: bool = False, halo=0,
                   origin: Optional[Sequence[int]] = None) -> None:
    """Write to every point (i, j, k) of the compute domain of ``dst`` the value of ``src`` at the position that ``pos_i`` /
    ``pos_j`` / ``pos_k`` hold for that point, in one kernel launch (per 8 pairs) on the current stream.

    ``dst``, ``src``  one field each or two sequences of equal length: IJK :class:`DeviceArray`\\ s of one dtype (float32 or
                float64) or anything ``as_device_array`` accepts; every field may differ in address, strides and padding.  A dst
                must not share memory with a src, a position field or another dst.
    ``pos_i``, ``pos_j``  IJK fields or ``Field[IJ]`` (shared by every level): positions in index units of the compute domain,
                0.0 = domain point 0.
    ``pos_k``   an IJK field: the position along K in levels, 0.0 = level 0, clamped to ``[0, nk - 1]``.  The three position
                fields share a dtype (float32 or float64, not necessarily the fields').
    ``method``  ``"nearest"``, ``"linear"``, ``"cubic"`` or ``"cubic_monotone"``.
    ``relative``  the position fields hold displacements from each point's own index, on all three axes.
    ``halo``    an int, ``(hi, hj)`` or ``((lo_i, hi_i), (lo_j, hi_j))``, as for ``boundary.fill_halo``: how far the gather may
                reach into ``src``'s ghost cells.  Positions (and stencil points) beyond it are clamped to it.
    ``origin``  first compute-domain point of every array, default ``(lo_i, lo_j, 0)``.

    Raises ``ValueError`` / ``TypeError`` (with the library's message) before any GPU work.  For a time loop build a
    :class:`DepartureInterp` once instead."""
    DepartureInterp(dst, src, pos_i=pos_i, pos_j=pos_j, pos_k=pos_k, method=method, relative=relative, halo=halo, origin=origin)()
