"""``gt4py_amd.horizontal`` -- the value of fields at run-time horizontal positions, one kernel launch per 8 fields.

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
"""

from __future__ import annotations

import ctypes
from typing import Optional, Sequence

from . import _lib
from ._bound import Bound, _float_pairs, _origin3, raise_refusal
from .storage.device_array import DeviceArray

METHODS = {"nearest": _lib.INTERP_NEAREST, "linear": _lib.INTERP_LINEAR, "cubic": _lib.INTERP_CUBIC,
           "cubic_monotone": _lib.INTERP_CUBIC_MONOTONE}


def _native(dst, src, n: int, pos_i, pos_j, extent, reach, size: int, pos_size: int, method: int, flags: int, stream: Optional[int]) -> int:
    """The ctypes call; a refusal of the library becomes ``ValueError`` (``TypeError`` for what no kernel handles) with the
    library's message.  Returns the kernels enqueued."""
    launches = ctypes.c_int(0)
    rc = _lib.load().gt4mi_horizontal_interp(dst, src, n, ctypes.byref(pos_i), ctypes.byref(pos_j), extent, reach, size, pos_size, method,
                                             flags, stream, ctypes.byref(launches))
    if rc != _lib.OK:
        raise_refusal("gt4mi_horizontal_interp", rc)
    return launches.value


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

    def __init__(self, dst, src, *, pos_i, pos_j, method: str = "linear", relative: bool = False, halo=0,
                 origin: Optional[Sequence[int]] = None):
        dsts, srcs, d_arrays, s_arrays, p_arrays, self._halo = _float_pairs(
            "interpolate", dst, src, halo, method, METHODS, shared=(pos_i, pos_j), names=("pos_i", "pos_j"), ndims=(2, 3), kind="Field[IJ]",
            plural="position fields")
        self.method, self.relative = method, bool(relative)
        lo_i, hi_i, lo_j, hi_j = self._halo
        self.origin = origin = _origin3(origin, self._halo)
        # the common compute domain: what every array has left behind its origin and (in I and J) in front of its high ghost cells
        rest = [tuple(s - o - h for s, o, h in zip(a.shape, origin, (hi_i, hi_j, 0))) for a in d_arrays + s_arrays + p_arrays]
        domain = tuple(min(r[ax] for r in rest if len(r) > ax) for ax in range(3))
        if min(domain) < 0:
            raise ValueError(f"halo {self._halo} and origin {origin} leave no domain in fields of shapes {[a.shape for a in d_arrays + s_arrays]}")
        self.domain = domain
        self._n = len(d_arrays)
        self._dst, self._src = (_lib.Field * self._n)(), (_lib.Field * self._n)()
        for table, arrays in ((self._dst, d_arrays), (self._src, s_arrays)):
            for n, a in enumerate(arrays):
                table[n] = _lib.Field.make(a.ptr, a.shape, a.strides, origin)
        self._pos_i, self._pos_j = (_position_field(a, origin) for a in p_arrays)
        self._extent = _lib.domain3(domain)
        self._reach = (ctypes.c_int64 * 4)(*self._halo)
        self._size, self._pos_size, self._method = d_arrays[0].itemsize, p_arrays[0].itemsize, METHODS[method]
        self._flags = _lib.INTERP_RELATIVE if self.relative else 0
        # every check of the library, nothing enqueued; also: how many kernels
        self.launches = _native(self._dst, self._src, self._n, self._pos_i, self._pos_j, self._extent, self._reach, self._size,
                                self._pos_size, self._method, self._flags | _lib.INTERP_DRY_RUN, None)
        self._bind("interpolate", d_arrays + s_arrays + p_arrays, dsts + srcs + [pos_i, pos_j])

    def __call__(self) -> None:
        self._check_alive()
        rc = self._lib.gt4mi_horizontal_interp(self._dst, self._src, self._n, ctypes.byref(self._pos_i), ctypes.byref(self._pos_j),
                                               self._extent, self._reach, self._size, self._pos_size, self._method, self._flags,
                                               self._current_stream().cuda_stream, None)
        if rc != _lib.OK:
            _lib.check("gt4mi_horizontal_interp", rc)


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
