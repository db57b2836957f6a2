"""``gt4py_amd.sampling`` -- the value of fields at a list of run-time positions (:func:`sample`): station soundings, cross-sections
along a path, the values along a track, one kernel launch per 8 fields.

A stencil writes fields of the shape it reads, at compile-time horizontal offsets; ``horizontal.HorizontalInterp`` and
``departure.DepartureInterp`` gather at run-time positions but write one value per point of the compute domain.  What an output
step asks for has another shape: 200 columns of a 1024 x 1024 x 80 field, not its 335 MB.  ``gt4mi_point_sample``
(csrc/point_sample.hip.h) computes the indices and weights of a point once and applies them to up to eight fields in the same
launch, on the current stream, without synchronisation or allocation, and leaves a small C-ordered result on the device.

    from gt4py_amd import sampling, transfer
    stations = sampling.Sample([t, q, u, v], pos_i=si, pos_j=sj, method="linear", halo=3)   # frozen; si, sj: 1-d device arrays
    out = transfer.Download([stations.result])
    for step in range(steps):
        ...
        if step % n == 0:
            stations()           # enqueues; result[f, p, k] = field f at (si[p], sj[p]), level k
            pending = out()      # the download behind it on the same stream reads the soundings

COLUMN MODE (no ``pos_k``): ``result`` has shape ``(nf, npoints, nk)`` -- a sounding per point; with the points along a flight leg or
a great circle, a curtain -- by the arithmetic of ``HorizontalInterp``.  POINT MODE (``pos_k`` given, in fractional levels):
``result`` has shape ``(nf, npoints)`` by the arithmetic of ``DepartureInterp``; ``vertical.VerticalInterp`` converts heights to
levels.  Positions are in index units of the compute domain (0.0 is domain point 0); ``halo`` is how far a gather may reach into
the ghost cells.  ``outside="clamp"`` clamps positions to that box as the interpolators do (NaN gives NaN); ``outside="fill"`` gives
every point outside it, or with a NaN position, ``fill_value`` instead -- on a decomposed run each rank samples its own stations and
the rest is marked.  The position arrays are read when the kernel runs: rewrite them between two calls and the samples move with
them.  The arithmetic -- float64 throughout, its order fixed -- is part of the contract (include/gt4py_amd.h): a sample has the same
bits whatever the layout, the other fields and points of the call, or the device, and they are the bits the two interpolators write.
"""

from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._bound import FLAGS, FLOATS, STREAM, BoundResult, Out, _as_list, _common_domain, _halo4, _origin3, field_table
from .horizontal import METHODS
from .storage.device_array import DeviceArray, as_device_array

OUTSIDE = {"clamp": 0, "fill": _lib.SAMPLE_FILL}


def _list_field(a: DeviceArray) -> "_lib.Field":
    """A 1-d array as a ``gt4mi_field``: axis 0 is the point."""
    return _lib.Field.make(a.ptr, (a.shape[0], 1, 1), (a.strides[0], 0, 0), (0, 0, 0))


class Sample(BoundResult):
    """The frozen form of :func:`sample` (what ``FrozenStencil`` is for stencils): arguments are checked (through the library's dry
    run), the native descriptors and the result built ONCE; ``__call__()`` makes only the ctypes call, on the stream that is
    current THEN, and does not synchronise; :meth:`get` synchronises that stream and returns a numpy array.

    ``result`` is a C-ordered :class:`DeviceArray` of the fields' dtype, ``(nf, npoints, nk)`` in column mode and ``(nf, npoints)``
    in point mode (``out=``: the caller's array of that shape and dtype, any strides); every call overwrites it, and later device
    code -- ``transfer.Download``, a stencil on :meth:`column` -- reads it in stream order.  ``npoints`` is the length of the
    position arrays, ``domain`` the compute domain of the fields, ``origin`` its first point in every field, ``launches`` the
    kernels a call enqueues.  The object holds raw pointers and weak references to the CALLER's objects, not the arrays: it refuses
    to run once one of them has died.  (An exporter that cannot be weakly referenced is held instead.)"""

    _entry, _dry_run_bit = "gt4mi_point_sample", _lib.SAMPLE_DRY_RUN

    def _arguments(self) -> tuple:
        return (self._dst, self._src, self._n, ctypes.byref(self._pos_i), ctypes.byref(self._pos_j),
                None if self._pos_k is None else ctypes.byref(self._pos_k), self.npoints, self._extent, self._reach, self._size, self._pos_size,
                self._method, FLAGS, self.fill_value, STREAM, Out(ctypes.c_int))

    def __init__(self, fields, *, pos_i, pos_j, pos_k=None, method: str = "linear", outside: str = "clamp", fill_value: float = math.nan,
                 halo=0, origin: Optional[Sequence[int]] = None, out=None):
        fields = _as_list(fields)
        if not fields:
            raise ValueError("sample needs at least one field")
        if method not in METHODS:
            raise ValueError(f"method must be one of {sorted(METHODS)}, not {method!r}")
        if outside not in OUTSIDE:
            raise ValueError(f"outside must be one of {sorted(OUTSIDE)}, not {outside!r}")
        if isinstance(fill_value, bool) or not isinstance(fill_value, (int, float, np.integer, np.floating)):
            raise TypeError(f"fill_value must be a number, not {type(fill_value).__name__}")
        arrays = [as_device_array(f) for f in fields]
        names = ("pos_i", "pos_j") + (() if pos_k is None else ("pos_k",))
        positions = [pos_i, pos_j] + ([] if pos_k is None else [pos_k])
        p_arrays = [as_device_array(p) for p in positions]
        self._halo = _halo4(halo)
        if min(self._halo) < 0:
            raise ValueError(f"halo widths must not be negative: {self._halo}")
        for a in arrays:
            if a.ndim != 3:
                raise ValueError(f"sample takes IJK fields, not a field of {a.ndim} dimension(s)")
        for name, a in zip(names, p_arrays):
            if a.ndim != 1:
                raise ValueError(f"{name} must be a 1-d array of positions, not an array of {a.ndim} dimension(s)")
        dtype = arrays[0].dtype
        for a in arrays:
            if a.dtype != dtype:
                raise TypeError(f"the fields of one call share a dtype: {dtype} and {a.dtype} differ")
        if dtype not in FLOATS:
            raise TypeError(f"sample takes float32 or float64 fields, not {dtype}")
        for name, a in zip(names[1:], p_arrays[1:]):
            if a.dtype != p_arrays[0].dtype:
                raise TypeError(f"pos_i and {name} share a dtype: {p_arrays[0].dtype} and {a.dtype} differ")
            if a.shape != p_arrays[0].shape:
                raise ValueError(f"pos_i and {name} share a length: {p_arrays[0].shape[0]} and {a.shape[0]} differ")
        if p_arrays[0].dtype not in FLOATS:
            raise TypeError(f"position arrays are float32 or float64, not {p_arrays[0].dtype}")
        if p_arrays[0].shape[0] < 1:
            raise ValueError("sample needs at least one point")
        self.method, self.outside, self.fill_value = method, outside, float(fill_value)
        self.origin = origin = _origin3(origin, self._halo)
        self.domain = domain = _common_domain(arrays, self._halo, origin, arrays)
        self.npoints = npoints = p_arrays[0].shape[0]
        self._n = len(arrays)
        shape = (self._n, npoints) + ((domain[2],) if pos_k is None else ())
        if out is None:
            import torch

            # (on the fields' device; for host arrays -- which _bind refuses last -- in host memory: no check before needs a device)
            self.result = DeviceArray(torch.empty(shape, dtype=arrays[0].tensor.dtype, device=arrays[0].tensor.device))
        else:
            self.result = as_device_array(out)
            if self.result.shape != shape or self.result.dtype != dtype:
                raise ValueError(f"out must have shape {shape} and dtype {dtype}, not {self.result.shape} and {self.result.dtype}")
        self._src = field_table(arrays, origin)
        self._dst = (_lib.Field * self._n)()
        for n in range(self._n):
            r = self.result[n]  # (npoints, nk) or (npoints,): axis 0 the point, axis 1 the level
            self._dst[n] = _lib.Field.make(r.ptr, tuple(r.shape) + (1,) * (3 - r.ndim), tuple(r.strides) + (0,) * (3 - r.ndim), (0, 0, 0))
        self._pos_i, self._pos_j = _list_field(p_arrays[0]), _list_field(p_arrays[1])
        self._pos_k = None if pos_k is None else _list_field(p_arrays[2])
        self._extent = _lib.domain3(domain)
        self._reach = (ctypes.c_int64 * 4)(*self._halo)
        self._size, self._pos_size, self._method = arrays[0].itemsize, p_arrays[0].itemsize, METHODS[method]
        self._flags = OUTSIDE[outside]
        # every check of the library, nothing enqueued; also: how many kernels
        self.launches, = self._dry_run()
        self._bind("sample", arrays + p_arrays + [self.result], fields + positions + ([] if out is None else [out]))

    def get(self) -> np.ndarray:
        """Synchronise the stream of the last call and return ``result`` as a numpy array (``RuntimeError`` before the first
        call)."""
        self._wait()
        return self.result.tensor.cpu().numpy()

    def column(self, n: int = 0) -> DeviceArray:
        """The device view of field ``n`` of ``result``: ``(npoints, nk)`` in column mode -- K contiguous --, ``(npoints,)`` in
        point mode.  It holds what the LAST call left there, in stream order."""
        return self.result[self._index(n, "field")]


def sample(fields, *, pos_i, pos_j, pos_k=None, method: str = "linear", outside: str = "clamp", fill_value: float = math.nan, halo=0,
           origin: Optional[Sequence[int]] = None, out=None) -> np.ndarray:
    """The value of ``fields`` at the positions ``pos_i`` / ``pos_j`` (/ ``pos_k``), as a numpy array: one kernel launch (per 8 fields)
    on the current stream, then a synchronisation of that stream.

    ``fields``  one field or a sequence of any length: IJK :class:`DeviceArray`\\ s of one dtype (float32 or float64) or anything
                ``as_device_array`` accepts; every field may differ in address, strides and padding.
    ``pos_i``, ``pos_j``  1-d device arrays (torch tensors or :class:`DeviceArray`\\ s) of one length and one dtype (float32 or float64,
                not necessarily the fields'): positions in index units of the compute domain, 0.0 = domain point 0.
    ``pos_k``   ``None`` -- column mode, the result is ``(nf, npoints, nk)``: every level at the point's horizontal position -- or a
                third such array of fractional levels, 0.0 = level 0 -- point mode, the result is ``(nf, npoints)``.
    ``method``  ``"nearest"``, ``"linear"``, ``"cubic"`` or ``"cubic_monotone"``, as for ``horizontal.interpolate`` (column mode) and
                ``departure.interpolate_3d`` (point mode).
    ``outside`` ``"clamp"``: positions beyond the halo (along K: beyond the levels) are clamped to it and a NaN position gives NaN;
                ``"fill"``: such points get ``fill_value`` (rounded once to the fields' dtype) in every field and level.
    ``halo``    an int, ``(hi, hj)`` or ``((lo_i, hi_i), (lo_j, hi_j))``, as for ``boundary.fill_halo``: how far a gather may reach
                into the fields' ghost cells.
    ``origin``  first compute-domain point of every field, default ``(lo_i, lo_j, 0)``.
    ``out``     a device array of the result's shape and dtype to write to (any strides) instead of a new one.

    Raises ``ValueError`` / ``TypeError`` (with the library's message) before any GPU work.  For a time loop build a
    :class:`Sample` once instead."""
    frozen = Sample(fields, pos_i=pos_i, pos_j=pos_j, pos_k=pos_k, method=method, outside=outside, fill_value=fill_value, halo=halo,
                    origin=origin, out=out)
    frozen()
    return frozen.get()
