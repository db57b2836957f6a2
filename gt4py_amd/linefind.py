"""``gt4py_amd.linefind`` -- WHERE on the lines of I, J or K something happens: the first crossing of a level, or the place of the
maximum / minimum, one kernel launch per 8 fields.

A stencil can write such a search along K only, as a FORWARD sweep with a carried flag, one field per call; it cannot write one
along I or J at all, and its result has another shape than the fields.  The freezing level, the height of a theta or PV surface,
cloud base and top, the mixed-layer depth (crossings, from the ground up or from the top down; the column need not be monotone),
the latitude of the jet axis, the level of maximum wind (extrema): ``gt4mi_line_find`` (csrc/line_find.hip.h) gives, for every line
of the box along ``axis``, the fractional position, the coordinate there and the value (or the number of crossings), for up to
eight fields per launch, on the current stream, without synchronisation, allocation or workspace.

    from gt4py_amd import linefind
    fz = linefind.LineFind([t], axis="K", what="crossing", level=273.15, coord=z)     # frozen
    for step in range(steps):
        physics(t, ...)                       # a stencil
        fz()                                  # one call on the current stream
        melt(fz.section("coord"), ...)        # the freezing-level height as Field[IJ, np.float64], same stream
    jet, = linefind.find_lines(ubar, axis="J", what="argmax")                         # one-shot, synchronous
    jet.position, jet.value

The comparisons and the arithmetic -- IEEE float64 on the items converted exactly, one rounding per operation, no FMA -- are part of
the contract (include/gt4py_amd.h): a line gives the same three numbers whatever the layout, the axis, the kernel path, the other
fields of the call or the device.
"""

from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._bound import FLAGS, STREAM, BoundResult, Out, _as_list, _axis_index, _coefficient, _line_pairs, field_table, one_shot
from .storage.device_array import DeviceArray

WHATS = {"crossing": _lib.FIND_CROSSING, "argmax": _lib.FIND_ARGMAX, "argmin": _lib.FIND_ARGMIN}
DIRECTIONS = {"any": _lib.FIND_ANY, "rising": _lib.FIND_RISING, "falling": _lib.FIND_FALLING}
PATHS = {_lib.LINE_PATH_LANES: "lanes", _lib.LINE_PATH_TILES: "tiles", _lib.LINE_PATH_ITEMS: "items"}
#: the rows of a result block, in order; the third is ``value`` for the extrema and ``crossings`` for a crossing
ROWS = ("position", "coord", "extra")


class Found:
    """What one field's lines gave: ``(nA, nB)`` numpy arrays -- A < B the two axes other than the line axis -- of ``position``
    (in forward index units of the box, fractional for a crossing), ``coord`` (the coordinate there; ``position`` where no
    ``coord=`` was given) and ``value`` (float64, the extrema; ``None`` for a crossing) or ``crossings`` (int64, how often the line
    crosses the level; ``None`` for the extrema).  A line without a crossing holds ``missing`` in ``position`` and ``coord``."""

    __slots__ = ("position", "coord", "value", "crossings")

    def __init__(self, position, coord, value=None, crossings=None):
        self.position, self.coord, self.value, self.crossings = position, coord, value, crossings

    @classmethod
    def from_rows(cls, rows, what: str) -> "Found":
        """From one ``(3, nB, nA)`` block of a :class:`LineFind` result."""
        rows = np.asarray(rows, dtype=np.float64)
        if rows.ndim != 3 or rows.shape[0] != _lib.FIND_ROWS:
            raise ValueError(f"a result block has shape (3, nB, nA), not {rows.shape}")
        position, coord, extra = (np.ascontiguousarray(r) for r in rows.transpose(0, 2, 1))
        if what == "crossing":
            return cls(position, coord, crossings=extra.astype(np.int64))
        return cls(position, coord, value=extra)

    def __repr__(self) -> str:
        return f"Found(shape={self.position.shape}, {'crossings' if self.value is None else 'value'})"


class LineFind(BoundResult):
    """The frozen form of :func:`find_lines`: arguments are checked (through the library's dry run), the descriptors and the result
    buffer built ONCE; ``__call__()`` makes only the ctypes call, on the stream that is current THEN, and does not synchronise;
    :meth:`get` synchronises that stream and returns one :class:`Found` per field.

    ``n`` is the line length, ``lines`` the number of lines, ``extent`` the IJK box (the compute domain grown by the halo in I and
    J), ``launches`` the kernels a call enqueues (one per 8 fields), ``path`` the kernel the strides select (``"lanes"``: lanes
    along a unit-stride axis other than ``axis``; ``"tiles"``: ``axis`` is the unit-stride axis, tiles go through LDS;
    ``"items"``: anything else, slow).

    ``result`` is a float64 :class:`DeviceArray` of shape ``(nf, 3, nB, nA)`` (rows in the order of :data:`ROWS`; A < B the two
    other axes: the layout of ``LineStats.result``); :meth:`section` hands out one row of it as an ``(nA, nB)`` view, which a
    stencil takes as ``Field[IJ, np.float64]`` (axis K), ``Field[IK, ...]`` (axis J) or ``Field[JK, ...]`` (axis I) in the same
    stream with no synchronisation in between.  Every call overwrites it.  The levels are passed BY VALUE at each call: a captured
    graph keeps the levels of its capture, :meth:`set_level` changes the next direct call only.  :meth:`get` also waits for the stream
    that is current then, so after a replay call it with the replay's stream current.  The object holds raw pointers and weak references to
    the CALLER's objects, not the arrays: it refuses to run once one of them has died."""

    _entry, _dry_run_bit = "gt4mi_line_find", _lib.FIND_DRY_RUN
    _result_ptr = None

    def _arguments(self) -> tuple:
        coord = None if self._coord is None else ctypes.byref(self._coord)
        return (self._fields, self._n, coord, self._extent3, self._axis, self._size, self._what, self._direction, self._level,
                ctypes.c_double(self.missing), self._result_ptr, FLAGS, STREAM, Out(ctypes.c_int), Out(ctypes.c_int))

    def __init__(self, fields, *, axis="K", what: str = "crossing", level=None, direction: str = "any", reverse: bool = False, coord=None,
                 missing: float = float("nan"), halo=0, origin: Optional[Sequence[int]] = None):
        fields = _as_list(fields)
        if not fields:
            raise ValueError("find_lines needs at least one field")
        ax = _axis_index(axis)
        shared = () if coord is None else (coord,)

        def names() -> None:
            if what not in WHATS:
                raise ValueError(f"what must be one of {sorted(WHATS)}, not {what!r}")
            if direction not in DIRECTIONS:
                raise ValueError(f"direction must be one of {sorted(DIRECTIONS)}, not {direction!r}")
            if what != "crossing" and (level is not None or direction != "any"):
                raise ValueError(f"a level and a direction go with what='crossing' only, not with what={what!r}")
            if what == "crossing" and level is None:
                raise ValueError("what='crossing' needs a level")

        #: ``extent``: the IJK box that is searched (the domain grown by the halo in I and J); ``n``, ``lines``: its lines' length and number
        (_, _, arrays, _, z_arrays, self._halo, self.origin, self.domain, self.extent, self.n, self.lines, _,
         start) = _line_pairs("find_lines", fields, fields, "IJK"[ax], halo, origin, shared=shared, names=("coord",),
                              sharing="the fields and the coord", own_checks=names)
        self.axis, self.what, self.direction, self.reverse, self.missing = ax, what, direction, bool(reverse), float(missing)
        self._n = len(arrays)
        self._level = None
        if what == "crossing":
            self._level = (ctypes.c_double * self._n)()
            self.set_level(level)
        self._fields = field_table(arrays, start)
        self._coord = _coefficient(z_arrays[0], ax, start) if z_arrays else None
        self._extent3 = _lib.domain3(self.extent)
        self._axis, self._size, self._what, self._direction = ax, arrays[0].itemsize, WHATS[what], DIRECTIONS[direction]
        self._flags = _lib.FIND_REVERSE if self.reverse else 0

        def allocate(torch, device, outs):
            a, b = (d for d in range(3) if d != ax)
            self.result = DeviceArray(torch.zeros((self._n, _lib.FIND_ROWS, self.extent[b], self.extent[a]), dtype=torch.float64, device=device))
            self._result_ptr = self.result.ptr

        path, self.launches = self._own_buffers("find_lines", arrays + z_arrays, allocate)
        self.path = PATHS.get(path)
        self._bind("find_lines", arrays + z_arrays, fields + list(shared))

    @property
    def level(self) -> Optional[tuple]:
        """The levels of the next call, one per field (``None`` for the extrema)."""
        return None if self._level is None else tuple(self._level)

    def set_level(self, values) -> None:
        """Replace the levels -- one float for every field, or one per field -- for the calls from now on.  They are passed by
        value at each call: nothing is checked again and nothing is rebuilt."""
        if self._level is None:
            raise ValueError(f"a level goes with what='crossing' only, not with what={self.what!r}")
        values = [float(v) for v in values] if isinstance(values, (tuple, list, np.ndarray)) else [float(values)] * self._n
        if len(values) != self._n:
            raise ValueError(f"one level for every field or one per field: {len(values)} levels for {self._n} field(s)")
        self._level[:] = values

    def get(self) -> List[Found]:
        """Synchronise the stream of the last call and return its results, one :class:`Found` per field (``RuntimeError`` before
        the first call)."""
        self._wait()
        return [Found.from_rows(block, self.what) for block in self.result.tensor.cpu().numpy()]

    def section(self, name: str, entry: int = 0) -> DeviceArray:
        """The ``(nA, nB)`` device view (byte strides ``(8, 8 * nA)``, no copy) of one row of ``result``: ``"position"``,
        ``"coord"``, and ``"value"`` (the extrema) or ``"crossings"`` (a crossing; as float64).  It holds what the LAST call left
        there, in stream order: pass it to a stencil as ``Field[IJ, np.float64]`` (axis K) on the stream of that call and no
        synchronisation is needed."""
        rows = ROWS[:2] + (("crossings",) if self.what == "crossing" else ("value",))
        if name not in rows:
            raise ValueError(f"no section {name!r}: the rows of what={self.what!r} are {', '.join(rows)}")
        return self.result[self._index(entry), rows.index(name)].transpose()


def find_lines(*fields, axis="K", what: str = "crossing", level=None, direction: str = "any", reverse: bool = False, coord=None,
               missing: float = float("nan"), halo=0, origin: Optional[Sequence[int]] = None) -> List[Found]:
    """Where every line of the compute domain (plus ``halo`` ghost cells in I and J) along ``axis`` first crosses ``level``, or has
    its maximum / minimum: one :class:`Found` per field, in one kernel launch (per 8 fields) on the current stream, then a
    synchronisation of that stream.

    ``fields``  IJK :class:`DeviceArray`\\ s of one dtype (float32 or float64) or anything ``as_device_array`` accepts; every
                field may differ in address, strides and padding.  None is written.
    ``axis``    ``"I"``, ``"J"``, ``"K"`` or 0, 1, 2.
    ``what``    ``"crossing"``, ``"argmax"`` or ``"argmin"``.  The extrema are ``numpy.argmax`` / ``numpy.argmin`` of the line in
                scan order: the first NaN wins, else the first of equal items.
    ``level``   (crossing only) one float, or one per field; kept as float64.  The pair ``q, q+1`` of the scan rises through it if
                ``y[q] < level <= y[q+1]`` and falls if ``y[q] > level >= y[q+1]``; the first item equal to it counts as found.
                The position is linear between the pair's items.  A NaN makes no crossing.
    ``direction``  (crossing only) ``"any"``, ``"rising"`` or ``"falling"``, in scan order.
    ``reverse``  scan from the far end of the line ("from the top down"; the extrema resolve a tie from that end).  Positions stay
                in the forward index units of the box.
    ``coord``   the coordinate along the line, of the fields' dtype, never written: an IJK field, or a 1-d array of n items along
                ``axis`` that every line shares (broadcast, not copied).  ``Found.coord`` is it at the position, linear between
                the pair's items.
    ``missing``  what ``position`` and ``coord`` hold on a line with no crossing (default NaN).
    ``halo``    an int, ``(hi, hj)`` or ``((lo_i, hi_i), (lo_j, hi_j))``, as for ``boundary.fill_halo``.
    ``origin``  first compute-domain point of every IJK array, default ``(lo_i, lo_j, 0)``.

    Raises ``ValueError`` / ``TypeError`` (with the library's message) before any GPU work.  In a time loop build a
    :class:`LineFind` once instead."""
    return one_shot(LineFind, fields, axis=axis, what=what, level=level, direction=direction, reverse=reverse, coord=coord, missing=missing,
                    halo=halo, origin=origin)
