"""``gt4py_amd.boundary`` -- boundary conditions on the I/J ghost cells of ``hip:mi300`` fields, one kernel launch.

The reference leaves boundary conditions to the user, who writes them with numpy / cupy slicing on storages that ARE numpy /
cupy arrays.  The storages of this backend are :class:`~gt4py_amd.storage.DeviceArray`\\ s, where eight slice assignments are
eight launches of a generic strided copy in front of every time step; ``gt4mi_halo_fill`` (csrc/halo_fill.hip.h) fills all
selected faces and corners of up to eight fields in ONE launch on the current stream, without synchronisation or allocation.

    from gt4py_amd import boundary
    boundary.fill_halo(u, v, halo=2, mode=("periodic", "zero_gradient"))       # one call
    bc = boundary.HaloFill([u, v], halo=2, mode=("periodic", "zero_gradient"))  # frozen: descriptors built once
    for step in range(n):
        bc()
        ...

Semantics = ``numpy.pad`` of the compute domain, axis by axis (I first, then J over the whole padded I range):
``"periodic"`` = wrap, ``"zero_gradient"`` = edge, ``"symmetric"``, ``"reflect"``, ``"constant"``; ``None`` leaves an axis alone.
Bit patterns are moved, never computed: bool and integer fields work, NaN payloads and the sign of zero survive.
"""

from __future__ import annotations

import ctypes
from typing import Any, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._bound import FLAGS, STREAM, Bound, Out, _box_of, _halo4, field_table
from .storage.device_array import DeviceArray, as_device_array

I_LO, I_HI, J_LO, J_HI = _lib.HALO_I_LO, _lib.HALO_I_HI, _lib.HALO_J_LO, _lib.HALO_J_HI
ALL = _lib.HALO_ALL_SIDES

MODES = {
    None: _lib.HALO_NONE,
    "periodic": _lib.HALO_PERIODIC,
    "zero_gradient": _lib.HALO_ZERO_GRADIENT,
    "symmetric": _lib.HALO_SYMMETRIC,
    "reflect": _lib.HALO_REFLECT,
    "constant": _lib.HALO_CONSTANT,
}


def physical_sides(decomp) -> int:
    """The ``sides`` mask of a :class:`~gt4py_amd.distributed.halo.Decomposition`: the sides of this rank's block that have
    no neighbour (``neighbours[...] is None``), i.e. the ones a boundary condition fills; the others belong to the exchange."""
    nb = decomp.neighbours
    return sum(bit for name, bit in (("W", I_LO), ("E", I_HI), ("S", J_LO), ("N", J_HI)) if nb[name] is None)


def _mode_pair(mode) -> Tuple[int, int]:
    pair = tuple(mode) if isinstance(mode, (tuple, list)) else (mode, mode)
    if len(pair) != 2:
        raise ValueError(f"mode must be one name or (mode_i, mode_j), not {mode!r}")
    for m in pair:
        if m is not None and not isinstance(m, str):
            raise TypeError(f"mode must be a name or None, not {type(m).__name__}")
        if m not in MODES:
            raise ValueError(f"unknown boundary mode {m!r}: expected one of {[k for k in MODES if k]} or None")
    return MODES[pair[0]], MODES[pair[1]]


class HaloFill(Bound):
    """The frozen form of :func:`fill_halo` (what ``FrozenStencil`` is for stencils): arguments are checked and the native
    descriptors built once, ``__call__()`` makes only the ctypes call, on the stream that is current THEN.

    The object holds raw pointers and weak references to the CALLER's objects, not the arrays: it refuses to run once one of
    them has died.  (An exporter that cannot be weakly referenced is held instead, so its memory stays valid.)"""

    _entry, _dry_run_bit = "gt4mi_halo_fill", _lib.HALO_DRY_RUN

    def _arguments(self) -> tuple:  # (the sides are the entry's flags)
        return (self._fields, self._n, self._domain3, self._halo4, self._modes[0], self._modes[1], FLAGS, self._value, self._itemsize,
                STREAM, Out(ctypes.c_int))

    def __init__(self, fields: Sequence[Any], *, halo, mode, origin: Optional[Sequence[int]] = None,
                 domain: Optional[Sequence[int]] = None, value=0, sides: int = ALL):
        fields = list(fields)
        arrays = [as_device_array(f) for f in fields]
        if not arrays:
            raise ValueError("fill_halo needs at least one field")
        self._halo = _halo4(halo)
        self._modes = _mode_pair(mode)
        if isinstance(sides, bool) or not isinstance(sides, (int, np.integer)):
            raise TypeError(f"sides must be a bit mask of I_LO, I_HI, J_LO, J_HI, not {type(sides).__name__}")
        if int(sides) & ~ALL:
            raise ValueError(f"sides must be a bit mask of I_LO, I_HI, J_LO, J_HI (0..{ALL}), not {int(sides)}")
        self._sides = self._flags = int(sides)
        first = arrays[0]
        for a in arrays:
            if a.ndim not in (2, 3):
                raise ValueError(f"fill_halo takes IJ or IJK fields; a field of {a.ndim} dimension(s) has no I or no J axis")
            if a.itemsize != first.itemsize or (a.dtype != first.dtype and _lib.HALO_CONSTANT in self._modes):
                raise TypeError(f"the fields of one call share an item size (and, for 'constant', a dtype): {first.dtype} and "
                                f"{a.dtype} differ")
        origin, domain = _box_of(first, self._halo, origin, domain, 0)
        self.origin, self.domain = origin, domain
        self._itemsize = first.itemsize
        # the scalar of "constant": one item of the fields' dtype, passed as its bytes (a value the dtype cannot hold is refused)
        try:
            item = np.array(value, dtype=first.dtype)
        except (TypeError, ValueError, OverflowError) as exc:
            raise TypeError(f"value {value!r} cannot be held by a {first.dtype} field") from exc
        if item.ndim != 0:
            raise TypeError("value must be a scalar")
        self._value = ctypes.create_string_buffer(item.tobytes(), 8)
        self._n = len(arrays)
        self._fields = field_table(arrays, origin)
        self._domain3 = _lib.domain3(domain)
        self._halo4 = (ctypes.c_int64 * 4)(*self._halo)
        # every check of the library, nothing enqueued; also: how many kernels a call makes
        self.launches, = self._dry_run()
        self._bind("fill_halo", arrays, fields)


def fill_halo(*fields, halo, mode, origin: Optional[Sequence[int]] = None, domain: Optional[Sequence[int]] = None, value=0,
              sides: int = ALL) -> None:
    """Fill the I/J ghost cells of ``fields`` from their own compute domain, in one kernel launch (per 8 fields) on the current
    stream.

    ``fields``  :class:`DeviceArray`\\ s (IJK, or IJ), or anything ``as_device_array`` accepts; they may differ in address,
                strides and padding and share item size, ``origin`` and ``domain``.
    ``halo``    an int, ``(hi, hj)`` or ``((lo_i, hi_i), (lo_j, hi_j))``.
    ``mode``    one name or ``(mode_i, mode_j)`` of ``"periodic" | "zero_gradient" | "symmetric" | "reflect" | "constant" | None``.
    ``origin``  first compute-domain point, default ``(lo_i, lo_j, 0)``; ``domain`` defaults to what remains of the first
                field's shape.
    ``value``   the scalar of ``"constant"``.
    ``sides``   bit mask of ``I_LO | I_HI | J_LO | J_HI`` (default ``ALL``); see :func:`physical_sides`.

    Raises ``ValueError`` / ``TypeError`` (with the library's message) before any GPU work.  For a time loop build a
    :class:`HaloFill` once instead."""
    HaloFill(fields, halo=halo, mode=mode, origin=origin, domain=domain, value=value, sides=sides)()
