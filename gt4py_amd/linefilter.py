"""``gt4py_amd.linefilter`` -- Fourier filtering along periodic lines of I, J or K, and the lines' spectra, one kernel launch per 8
fields.

A stencil reads its neighbours at compile-time offsets; a Fourier coefficient reads the whole line.  The polar filter of a
latitude-longitude grid (the high zonal wavenumbers damped with a response that depends on the latitude), a spectral low-pass or
de-aliasing filter on a doubly periodic box, a sponge on selected wavenumbers, the zonal power spectrum: ``gt4mi_line_filter``
(csrc/line_filter.hip.h) transforms every line of the box along ``axis``, multiplies wavenumber ``m`` by a real ``response[m]`` and
transforms back, for up to eight (dst, src) pairs per launch, on the current stream, without synchronisation, allocation or
workspace.  The line stays on chip between the forward transform, the multiply and the inverse: every item is read once and written
once.

    from gt4py_amd import linefilter
    polar = linefilter.LineFilter([u, v, t], [u, v, t], axis="I", response=damping)    # frozen; damping: (nj, 1, ni // 2 + 1)
    for step in range(steps):
        dynamics(u, v, t, ...)            # a stencil
        polar()                           # one call on the current stream, in place
        physics(u, v, t, ...)
    zonal = linefilter.LineSpectrum([u], axis="I")                                     # frozen; zonal() ... zonal.power()

The arithmetic -- radix-2, IEEE float64 on the items converted exactly, one rounding per operation, no FMA, the twiddles a table
that this module computes with numpy -- is part of the contract (include/gt4py_amd.h): the same line, response and length give the
same bits whatever the layout, the axis, the kernel path, the other fields of the call or the device.  The line length is a power
of two from 2 to 4096; mixed radix is out of scope.  A rank that holds only part of a line cannot transform it: there is no merge.
"""

from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._bound import FLAGS, STREAM, Bound, BoundResult, Out, _as_list, _line_pairs, field_table, one_shot
from .storage.device_array import DeviceArray, as_device_array

PATHS = {_lib.LINE_PATH_LANES: "lanes", _lib.LINE_PATH_TILES: "tiles", _lib.LINE_PATH_ITEMS: "items"}


def twiddles(n: int) -> np.ndarray:
    """The table the kernels take, ``n`` float64: ``cos(2 pi j / n)`` at ``[j]`` and ``-sin(2 pi j / n)`` at ``[n // 2 + j]`` for
    ``j < n // 2``, from numpy; ``w[0] = (1, 0)`` and ``w[n // 4] = (0, -1)`` are set exactly."""
    j = np.arange(n // 2, dtype=np.float64)
    wr, wi = np.cos(2.0 * np.pi * j / n), -np.sin(2.0 * np.pi * j / n)
    wr[0], wi[0] = 1.0, 0.0
    if n >= 4:
        wr[n // 4], wi[n // 4] = 0.0, -1.0
    return np.concatenate([wr, wi])


class _Lines(Bound):
    """What :class:`LineFilter` and :class:`LineSpectrum` share: one native entry, one argument list, the twiddle table."""

    _entry, _dry_run_bit = "gt4mi_line_filter", _lib.FILTER_DRY_RUN
    _mode = _lib.FILTER_APPLY
    _dst = _response = _response_extent = _twiddle_ptr = _result_ptr = None

    def _arguments(self) -> tuple:
        return (self._dst, self._src, self._n, self._response, self._response_extent, self._twiddle_ptr, self._result_ptr, self._extent3,
                self._axis, self._size, self._mode, FLAGS, STREAM, Out(ctypes.c_int), Out(ctypes.c_int))

    def _own_twiddles(self, torch, device, outs) -> None:
        """The twiddle table on the device: built once, owned by the object (what :meth:`_own_buffers` calls)."""
        self._twiddles = torch.from_numpy(twiddles(self.n)).to(device)
        self._twiddle_ptr = self._twiddles.data_ptr()


class LineFilter(_Lines):
    """The frozen form of :func:`filter_lines` (what ``FrozenStencil`` is for stencils): arguments are checked (through the
    library's dry run), the native descriptors and the twiddle table built once; ``__call__()`` makes only the ctypes call, on the
    stream that is current THEN.

    ``n`` is the line length, ``lines`` the number of lines, ``extent`` the IJK box (the compute domain grown by the halo in I and
    J), ``launches`` the kernels a call enqueues (one per 8 pairs), ``path`` the way the strides select for the loads and stores
    (``"tiles"``: ``axis`` is the unit-stride axis, lanes run along the line; ``"lanes"``: another axis is, a workgroup takes
    neighbouring lines along it; ``"items"``: anything else, slow).  The response is read when the kernel runs: rewriting it
    changes the filter of the next call, nothing is checked again.  The object holds raw pointers and weak references to the
    CALLER's objects, not the arrays: it refuses to run once one of them has died."""

    def __init__(self, dst, src, *, axis: str = "I", response, halo=0, origin: Optional[Sequence[int]] = None):
        #: ``extent``: the IJK box that is filtered (the domain grown by the halo in I and J); ``n``, ``lines``: its lines' length and number
        (dsts, srcs, d_arrays, s_arrays, _, self._halo, self.origin, self.domain, self.extent, self.n, self.lines, ax,
         start) = _line_pairs("filter_lines", dst, src, axis, halo, origin, shared=(), names=(), sharing="the fields")
        self.axis = axis
        r = as_device_array(response)
        nh = self.n // 2 + 1
        if r.dtype != np.dtype("float64"):
            raise TypeError(f"response must be float64, not {r.dtype}")
        if r.ndim not in (1, 3):
            raise ValueError(f"response must have shape (nh,) or (ea, eb, nh), not {r.shape}")
        if r.shape[-1] != nh:
            raise ValueError(f"response holds {r.shape[-1]} wavenumbers, a line of {self.n} points along {axis} needs n // 2 + 1 = {nh}")
        dense = tuple(8 * int(np.prod(r.shape[d + 1:])) for d in range(r.ndim))
        if any(s != d for s, d, e in zip(r.strides, dense, r.shape) if e > 1):
            raise ValueError(f"response must be C-ordered and dense, not of byte strides {r.strides}")
        self._n = len(d_arrays)
        self._dst, self._src = field_table(d_arrays, start), field_table(s_arrays, start)
        self._response = r.ptr
        self._response_extent = (ctypes.c_int64 * 2)(*((1, 1) if r.ndim == 1 else r.shape[:2]))
        self._extent3 = _lib.domain3(self.extent)
        self._axis, self._size = ax, d_arrays[0].itemsize
        path, self.launches = self._own_buffers("filter_lines", d_arrays + s_arrays + [r], self._own_twiddles)
        self.path = PATHS.get(path)
        self._bind("filter_lines", d_arrays + s_arrays + [r], dsts + srcs + [response])


def filter_lines(dst, src, *, axis: str = "I", response, halo=0, origin: Optional[Sequence[int]] = None) -> None:
    """``dst`` = ``src`` with every line of the compute domain (plus ``halo`` ghost cells in I and J) along ``axis`` taken as
    periodic, transformed, wavenumber ``m`` multiplied by ``response[m]`` and transformed back, in one kernel launch (per 8 pairs)
    on the current stream.

    ``dst``, ``src``  one field each or two sequences of equal length: IJK :class:`DeviceArray`\\ s of one dtype (float32 or
                float64) or anything ``as_device_array`` accepts; every field may differ in address, strides and padding.
                ``dst[n]`` may be ``src[n]`` itself (in place); every other overlap is refused.
    ``axis``    ``"I"``, ``"J"`` or ``"K"``.  The line length ``n`` must be a power of two, 2 <= n <= 4096.
    ``response``  float64 on the device, C-ordered, never written, its values not checked: ``(nh,)`` with ``nh = n // 2 + 1`` that
                every line shares, or ``(ea, eb, nh)``, ``ea`` and ``eb`` the extents of the two other axes in IJK order, either of
                which may be 1 and broadcasts: the polar filter along I is ``(nj, 1, nh)``.
    ``halo``    an int, ``(hi, hj)`` or ``((lo_i, hi_i), (lo_j, hi_j))``, as for ``boundary.fill_halo``.
    ``origin``  first compute-domain point of every IJK array, default ``(lo_i, lo_j, 0)``.

    The arithmetic is float64 whatever the fields' dtype, with one rounding on the store.  A response of all ones returns ``src``
    to within a few float64 roundings of the line's largest item, NOT bit for bit.  Raises ``ValueError`` / ``TypeError`` (with the
    library's message) before any GPU work."""
    LineFilter(dst, src, axis=axis, response=response, halo=halo, origin=origin)()


class LineSpectrum(_Lines, BoundResult):
    """The forward transform alone, for up to 8 fields per launch: frozen like :class:`LineFilter`, with a result the object owns.

    ``result`` is a float64 :class:`DeviceArray` of shape ``(nf, 2, ea, eb, nh)``: row 0 the real, row 1 the imaginary part,
    ``ea`` and ``eb`` the extents of the two axes other than ``axis`` in IJK order, wavenumber ``m = 0 .. n // 2`` fastest; the
    shape does not depend on the path.  Every call overwrites it.  ``n``, ``lines``, ``extent``, ``launches`` and ``path`` as on
    :class:`LineFilter`.  There is no merge: a rank that holds part of a line cannot transform it."""

    _mode = _lib.FILTER_SPECTRUM

    def __init__(self, fields, *, axis: str = "I", halo=0, origin: Optional[Sequence[int]] = None):
        fields = _as_list(fields)
        if not fields:
            raise ValueError("spectrum_lines needs at least one field")
        (_, _, arrays, _, _, self._halo, self.origin, self.domain, self.extent, self.n, self.lines, ax,
         start) = _line_pairs("spectrum_lines", fields, fields, axis, halo, origin, shared=(), names=(), sharing="the fields")
        self.axis = axis
        self._n = len(arrays)
        self._src = field_table(arrays, start)
        self._extent3 = _lib.domain3(self.extent)
        self._axis, self._size = ax, arrays[0].itemsize

        def allocate(torch, device, outs):
            self._own_twiddles(torch, device, outs)
            ea, eb = (self.extent[d] for d in range(3) if d != ax)
            self.result = DeviceArray(torch.zeros((self._n, 2, ea, eb, self.n // 2 + 1), dtype=torch.float64, device=device))
            self._result_ptr = self.result.ptr

        path, self.launches = self._own_buffers("spectrum_lines", arrays, allocate)
        self.path = PATHS.get(path)
        self._bind("spectrum_lines", arrays, fields)

    def coefficients(self) -> DeviceArray:
        """The device view ``(nf, 2, ea, eb, nh)`` of the result: what the LAST call left there, in stream order."""
        return self.result

    def get(self) -> np.ndarray:
        """Synchronise the stream of the last call and return the coefficients as a complex128 numpy array ``(nf, ea, eb, nh)``
        (``RuntimeError`` before the first call)."""
        self._wait()
        rows = self.result.tensor.cpu().numpy()
        out = np.empty(rows.shape[:1] + rows.shape[2:], dtype=np.complex128)
        out.real, out.imag = rows[:, 0], rows[:, 1]  # (the parts as they are: 1j * inf would put a NaN beside it)
        return out

    def power(self) -> np.ndarray:
        """On the host: ``|X[m]|**2 / n**2`` of :meth:`get`, with the factor 2 for ``0 < m < n // 2`` (the two-sided spectrum
        folded: the rows sum to the line's mean square)."""
        c = self.get()
        p = (c.real * c.real + c.imag * c.imag) / (float(self.n) * float(self.n))
        p[..., 1: self.n // 2] *= 2.0
        return p


def spectrum_lines(*fields, axis: str = "I", halo=0, origin: Optional[Sequence[int]] = None) -> np.ndarray:
    """The Fourier coefficients of every line of the compute domain (plus ``halo`` ghost cells in I and J) along ``axis``, for
    wavenumbers ``0 .. n // 2``: a complex128 numpy array ``(nf, ea, eb, nh)``, in one kernel launch (per 8 fields) on the current
    stream, then a synchronisation of that stream.  Arguments as for :func:`filter_lines`.  In a time loop build a
    :class:`LineSpectrum` once instead."""
    return one_shot(LineSpectrum, fields, axis=axis, halo=halo, origin=origin)
