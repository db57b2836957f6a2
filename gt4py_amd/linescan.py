"""``gt4py_amd.linescan`` -- running sums, maxima and minima along the lines of I, J or K, one kernel launch per 8 fields.

A stencil can write a scan along K only, as a FORWARD or BACKWARD sweep, one field per call; it cannot write one along I or J at
all.  The integral of ``v dx`` from the western wall, an accumulated optical path, "is there cloud anywhere west of this point",
the mass above a level for several fields at once, a cumulative distribution for remapping: ``gt4mi_line_scan``
(csrc/line_scan.hip.h) gives, at every point of every line of the box along ``axis``, the reduction of the line so far, for up to
eight (dst, src) pairs per launch, on the current stream, without synchronisation, allocation or workspace.

    from gt4py_amd import linescan
    linescan.scan_lines(psi, v, axis="I", weight=dx)                                   # psi = the integral of v dx from the west
    scan = linescan.LineScan([tu, tv], [u, v], axis="I", op="sum", weight=dx)          # frozen
    for step in range(steps):
        winds(u, v, ...)                  # a stencil
        scan()                            # one call on the current stream
        transport(tu, tv, ...)

The arithmetic -- strictly sequential along the line, one rounding per operation, no FMA -- is part of the contract
(include/gt4py_amd.h): the same line gives the same bits whatever the layout, the axis, the kernel path, the position in the call
or the device, and the float sum is ``numpy.cumsum`` along that axis bit for bit.  Parallelism comes across lines: a box of few,
long lines (a 2-d field with 1024 lines) is served correctly and not fast; a segmented parallel scan, whose order of additions
would depend on the length, is out of scope.
"""

from __future__ import annotations

import ctypes
from typing import Optional, Sequence

from . import _lib
from ._bound import FLAGS, STREAM, Bound, Out, _coefficient, _line_pairs, field_table

OPS = {"sum": _lib.SCAN_SUM, "max": _lib.SCAN_MAX, "min": _lib.SCAN_MIN}
PATHS = {_lib.SCAN_PATH_LANES: "lanes", _lib.SCAN_PATH_TILES: "tiles", _lib.SCAN_PATH_ITEMS: "items"}


class LineScan(Bound):
    """The frozen form of :func:`scan_lines` (what ``FrozenStencil`` is for stencils): arguments are checked (through the
    library's dry run) and the native descriptors built once, ``__call__()`` makes only the ctypes call, on the stream that is
    current THEN.

    ``n`` is the line length, ``lines`` the number of lines, ``extent`` the IJK box (the compute domain grown by the halo in I
    and J), ``launches`` the kernels a call enqueues, ``path`` the kernel the strides select (``"lanes"``: lanes along a
    unit-stride axis other than ``axis``; ``"tiles"``: ``axis`` is the unit-stride axis, tiles go through LDS; ``"items"``:
    anything else, slow).  The object holds raw pointers and weak references to the CALLER's objects, not the arrays: it refuses
    to run once one of them has died."""

    _entry, _dry_run_bit = "gt4mi_line_scan", _lib.SCAN_DRY_RUN

    def _arguments(self) -> tuple:
        weight = None if self._weight is None else ctypes.byref(self._weight)
        return (self._dst, self._src, self._n, weight, self._extent3, self._axis, self._size, self._op, FLAGS, STREAM, Out(ctypes.c_int),
                Out(ctypes.c_int))

    def __init__(self, dst, src, *, axis: str = "I", op: str = "sum", exclusive: bool = False, reverse: bool = False, weight=None,
                 wide: bool = False, halo=0, origin: Optional[Sequence[int]] = None):
        shared = () if weight is None else (weight,)

        def names() -> None:
            if op not in OPS:
                raise ValueError(f"op must be one of {sorted(OPS)}, not {op!r}")
            if weight is not None and op != "sum":
                raise ValueError(f"a weight goes with op='sum' only, not with op={op!r}")

        #: ``extent``: the IJK box that is scanned (the domain grown by the halo in I and J); ``n``, ``lines``: its lines' length and number
        (dsts, srcs, d_arrays, s_arrays, w_arrays, self._halo, self.origin, self.domain, self.extent, self.n, self.lines, ax,
         start) = _line_pairs("scan_lines", dst, src, axis, halo, origin, shared=shared, names=("weight",),
                              sharing="the fields and the weight", own_checks=names)
        self.axis, self.op, self.exclusive, self.reverse, self.wide = axis, op, bool(exclusive), bool(reverse), bool(wide)
        self._n = len(d_arrays)
        self._dst, self._src = field_table(d_arrays, start), field_table(s_arrays, start)
        self._weight = _coefficient(w_arrays[0], ax, start) if w_arrays else None
        self._extent3 = _lib.domain3(self.extent)
        self._axis, self._size, self._op = ax, d_arrays[0].itemsize, OPS[op]
        self._flags = ((_lib.SCAN_EXCLUSIVE if self.exclusive else 0) | (_lib.SCAN_REVERSE if self.reverse else 0) |
                       (_lib.SCAN_WIDE if self.wide else 0))
        path, self.launches = self._dry_run()  # every check of the library, nothing enqueued
        self.path = PATHS.get(path)
        self._bind("scan_lines", d_arrays + s_arrays + w_arrays, dsts + srcs + list(shared))


def scan_lines(dst, src, *, axis: str = "I", op: str = "sum", exclusive: bool = False, reverse: bool = False, weight=None,
               wide: bool = False, halo=0, origin: Optional[Sequence[int]] = None) -> None:
    """``dst`` = the running ``op`` of ``src`` along every line of the compute domain (plus ``halo`` ghost cells in I and J) along
    ``axis``, in one kernel launch (per 8 pairs) on the current stream.

    ``dst``, ``src``  one field each or two sequences of equal length: IJK :class:`DeviceArray`\\ s of one dtype (float32 or
                float64) or anything ``as_device_array`` accepts; every field may differ in address, strides and padding.
                ``dst[n]`` may be ``src[n]`` itself (in place); every other overlap is refused.
    ``axis``    ``"I"``, ``"J"`` or ``"K"``.
    ``op``      ``"sum"``, ``"max"`` or ``"min"``.  A NaN, once met, stays in the rest of its line (max and min do not drop it).
    ``exclusive``  ``dst[m]`` holds the scan of the items BEFORE ``m``; the first item gets the identity: ``+0.0`` for sum,
                ``-inf`` for max, ``+inf`` for min.
    ``reverse``  the scan starts at the far end of the line (the BACKWARD sweep); ``dst`` is written at the item's own index.
    ``weight``  (sum only) the terms' factors, the grid spacing of an integral: terms are ``src[m] * weight[m]``.  Of the fields'
                dtype, never written: an IJK field, or a 1-d array of n items along ``axis`` that every line shares (broadcast,
                not copied).
    ``wide``    sum on float32 fields: accumulate in float64, with one rounding to float32 on the store.  It has NO effect for
                float64 fields or for max and min.
    ``halo``    an int, ``(hi, hj)`` or ``((lo_i, hi_i), (lo_j, hi_j))``, as for ``boundary.fill_halo``.
    ``origin``  first compute-domain point of every IJK array, default ``(lo_i, lo_j, 0)``.

    The sum is strictly sequential along the line, one rounding per addition: ``numpy.cumsum`` along that axis bit for bit (with
    ``wide``: ``numpy.cumsum(x, dtype=float64).astype(float32)``).  Raises ``ValueError`` / ``TypeError`` (with the library's
    message) before any GPU work."""
    LineScan(dst, src, axis=axis, op=op, exclusive=exclusive, reverse=reverse, weight=weight, wide=wide, halo=halo, origin=origin)()
