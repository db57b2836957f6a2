"""``gt4py_amd.diagnostics`` -- one-pass, bit-reproducible statistics of ``hip:mi300`` fields.

What a time loop asks of a field after every few steps -- is anything NaN or Inf yet, what is max |u| (CFL), what is the total
(conservation), what is ||a - b|| between two time levels, <r, p> in an iterative solver -- the reference leaves to numpy / cupy
on storages that ARE numpy / cupy arrays.  ``gt4mi_field_stats`` (csrc/field_stats.hip.h) reads up to eight fields ONCE in one
launch, a second small launch combines the tiles' partial results; nothing is allocated and nothing synchronises.

    from gt4py_amd import diagnostics
    s, = diagnostics.field_stats(u, halo=2)                 # one shot, synchronous: s.max_abs, s.sum, s.all_finite ...
    watch = diagnostics.FieldStats([u], halo=2)             # frozen: buffers and descriptors built once
    for step in range(n):
        ...
        watch()                                             # enqueued on the current stream, no synchronisation
    s, = watch.get()                                        # synchronises that stream

All arithmetic is float64 (float32 fields are widened first).  THE ORDER OF THE ADDITIONS IS PART OF THE CONTRACT: it depends on
the domain ``(ni, nj, nk)`` alone -- not on addresses, strides, padding, how many fields share the call, or the device -- so the
same domain data gives the same bits, always.  Results of a decomposed run are joined with :func:`merge`.

PER LEVEL (``gt4mi_level_stats``, csrc/level_stats.hip.h): the same eight values and the mean for every level ``k`` of the
domain, one pass again, left on the device as contiguous ``Field[K, float64]`` profiles that a stencil can read in the same
stream -- what GTScript, which has no reduction over I and J, cannot express:

    watch = diagnostics.LevelStats([u], halo=2)
    watch()                                                 # enqueued, no synchronisation
    anomaly(u, watch.profile("mean"), out)                  # m: Field[K, np.float64]; out = u - m
    p, = watch.get()                                        # a Profile: p.max_abs[k], p.first_nonfinite, p[k] (a Stats)

The order of the additions of a level depends on ``(ni, nj)`` alone: the same plane gives the same bits whatever ``nk`` is and
whichever level it is.  Profiles of a decomposed run are joined with :func:`merge_profiles`.
"""

from __future__ import annotations

import ctypes
import math
from typing import Any, List, NamedTuple, Optional, Sequence, Union

import numpy as np

from . import _lib
from ._bound import FLAGS, FLOATS, STREAM, BoundResult, Out, _axis_index, _box_of, _halo4, _shape3, one_shot
from .storage.device_array import DeviceArray, as_device_array


class Stats(NamedTuple):
    """The eight values of one entry (``x`` = the field, or ``a - b`` with a second field) and what follows from them."""

    count: int        # points of the domain
    nonfinite: int    # points where x is NaN or +-Inf
    sum: float
    sum_abs: float
    sum_sq: float
    min: float        # NaN if any x is NaN; min(-0, +0) = -0
    max: float        # NaN if any x is NaN; max(-0, +0) = +0
    dot: float        # sum of a * b with a second field, else 0

    @property
    def mean(self) -> float:
        return self.sum / self.count if self.count else math.nan

    @property
    def norm2(self) -> float:
        return math.sqrt(self.sum_sq)

    @property
    def max_abs(self) -> float:
        if math.isnan(self.min) or math.isnan(self.max):
            return math.nan
        return max(abs(self.min), abs(self.max))

    @property
    def all_finite(self) -> bool:
        return self.nonfinite == 0

    @classmethod
    def from_row(cls, row) -> "Stats":
        r = [float(v) for v in row]
        return cls(int(r[_lib.STATS_COUNT]), int(r[_lib.STATS_NONFINITE]), r[_lib.STATS_SUM], r[_lib.STATS_SUM_ABS],
                   r[_lib.STATS_SUM_SQ], r[_lib.STATS_MIN], r[_lib.STATS_MAX], r[_lib.STATS_DOT])


def _minimum(a: float, b: float) -> float:
    if math.isnan(a) or math.isnan(b):
        return math.nan
    if a == b:  # equal: -0 wins over +0
        return a if math.copysign(1.0, a) < 0 else b
    return a if a < b else b


def _maximum(a: float, b: float) -> float:
    if math.isnan(a) or math.isnan(b):
        return math.nan
    if a == b:  # equal: +0 wins over -0
        return a if math.copysign(1.0, a) > 0 else b
    return a if a > b else b


def merge(stats: Sequence[Stats]) -> Stats:
    """Join the per-rank results of a decomposed run on the host, IN THE ORDER GIVEN.

    ``count`` and ``nonfinite`` add exactly; ``min`` / ``max`` are joined exactly (NaN if any is NaN, -0 below +0).  The sums
    are added left to right in float64: reproducible for a fixed process grid and rank order, but NOT bit for bit what one
    undecomposed call over the whole domain gives (its additions are ordered by the whole domain).  No collective is made
    here; gather first, in rank order:

        local, = diagnostics.field_stats(u, halo=2)
        parts = [None] * torch.distributed.get_world_size()
        torch.distributed.all_gather_object(parts, local)
        total = diagnostics.merge(parts)          # the same bits on every rank
    """
    stats = list(stats)
    if not stats:
        raise ValueError("merge needs at least one Stats")
    for s in stats:
        if not isinstance(s, Stats):
            raise TypeError(f"merge joins Stats records, not {type(s).__name__}")
    out = stats[0]
    for s in stats[1:]:
        out = Stats(out.count + s.count, out.nonfinite + s.nonfinite, out.sum + s.sum, out.sum_abs + s.sum_abs,
                    out.sum_sq + s.sum_sq, _minimum(out.min, s.min), _maximum(out.max, s.max), out.dot + s.dot)
    return out


class _StatsCall(BoundResult):
    """What :class:`FieldStats` and :class:`LevelStats` share: everything but the entry, the public function's name in the
    messages and the shape of a result block."""

    _who = ""
    _dry_run_bit = _lib.STATS_DRY_RUN

    def _result_block(self) -> tuple:
        raise NotImplementedError

    _workspace_ptr, _workspace_bytes, _result_ptr = None, 0, None  # (until the first dry run has said how large they are)

    def _arguments(self) -> tuple:
        return (self._fields, self._others, self._n, self._domain3, self._itemsize, self._workspace_ptr, self._workspace_bytes,
                self._result_ptr, FLAGS, STREAM, Out(ctypes.c_int64), Out(ctypes.c_int))

    def __init__(self, fields: Sequence[Any], *, others: Optional[Sequence[Any]] = None, origin: Optional[Sequence[int]] = None,
                 domain: Optional[Sequence[int]] = None, halo=0):
        who = self._who
        fields = list(fields)
        arrays = [as_device_array(f) for f in fields]
        if not arrays:
            raise ValueError(f"{who} needs at least one field")
        if others is None:
            others = [None] * len(fields)
        others = list(others)
        if len(others) != len(fields):
            raise ValueError(f"others must have one entry (or None) per field: {len(others)} for {len(fields)} fields")
        other_arrays = [None if o is None else as_device_array(o) for o in others]
        first = arrays[0]
        every = arrays + [o for o in other_arrays if o is not None]
        for a in every:
            if a.dtype not in FLOATS:
                raise TypeError(f"{who} takes float32 or float64 fields, not {a.dtype}")
            if a.dtype != first.dtype:
                raise TypeError(f"the fields of one call share a dtype: {first.dtype} and {a.dtype} differ")
            if a.ndim not in (2, 3):
                raise ValueError(f"{who} takes IJ or IJK fields, not a field of {a.ndim} dimension(s)")
        self.origin, self.domain = origin, domain = _box_of(first, _halo4(halo), origin, domain, 1)
        self._itemsize = first.itemsize
        self._n = len(arrays)

        def describe(a, weight):
            strides = tuple(a.strides) + (0,) * (3 - a.ndim)
            # a broadcast axis of a weight (stride 0) has no origin of its own
            org = tuple(0 if weight and s == 0 else o for o, s in zip(origin, strides))
            return _lib.Field.make(a.ptr, _shape3(a), strides, org)

        self._fields = (_lib.Field * self._n)()
        self._others = (_lib.Field * self._n)()  # (data == NULL: no second field)
        for n, (a, o) in enumerate(zip(arrays, other_arrays)):
            self._fields[n] = describe(a, False)
            if o is not None:
                self._others[n] = describe(o, True)
        self._domain3 = _lib.domain3(domain)

        def allocate(torch, device, outs):
            needed = outs[0]
            self._workspace = torch.empty(needed // 8, dtype=torch.float64, device=device)
            self.result = DeviceArray(torch.zeros((self._n,) + self._result_block(), dtype=torch.float64, device=device))
            self._workspace_ptr, self._workspace_bytes, self._result_ptr = self._workspace.data_ptr(), needed, self.result.ptr

        # the dry run says: the workspace the call needs, how many kernels it makes and, for LineStats, the kernel the strides selected
        _, self.launches, *path = self._own_buffers(who, every, allocate)
        if path:
            self.path, = path
        self._bind(who, every, fields + [o for o in others if o is not None])

    _record = None  # what get() makes of one entry's block of the result

    def get(self) -> list:
        """Synchronise the stream of the last call and the stream that is current now (where a replay of a captured graph ran:
        call ``get()`` with that stream current) and return the results, one record per entry (``RuntimeError`` before the first
        call)."""
        self._wait()
        return [self._record(block) for block in self.result.tensor.cpu().numpy()]

    def _row(self, what: str, name: str, entry: int) -> DeviceArray:
        """Row ``name`` of entry ``entry`` of ``result``, as the device holds it; ``what``: what the caller calls it."""
        if name not in PROFILE_ROWS:
            raise ValueError(f"no {what} {name!r}: the rows are {', '.join(PROFILE_ROWS)}")
        return self.result[self._index(entry), PROFILE_ROWS.index(name)]


def _one_shot(frozen_class, fields, other, **kwargs):
    """The synchronous form of a statistics call: ``other`` for every field or one per field, then :func:`one_shot` on the fields
    as ONE tuple (they come positionally only: a list among them is no field)."""
    others = list(other) if isinstance(other, (list, tuple)) else None if other is None else [other] * len(fields)
    return one_shot(frozen_class, (fields,), others=others, **kwargs)


class FieldStats(_StatsCall):
    """The frozen form of :func:`field_stats`: arguments are checked (through the library's dry run), the descriptors, the
    workspace and the result buffer built ONCE; ``__call__()`` makes only the ctypes call, on the stream that is current THEN,
    and does not synchronise; :meth:`get` synchronises that stream and returns one :class:`Stats` per entry.

    ``result`` is a float64 :class:`DeviceArray` of shape ``(n, 8)`` (slots in the order of :class:`Stats`): a later kernel, or
    a captured graph, can read it on the device.  Every call overwrites it.

    The object holds raw pointers and weak references to the CALLER's objects, not the arrays: it refuses to run once one of
    them has died.  (An exporter that cannot be weakly referenced is held instead, so its memory stays valid.)"""

    _who, _entry, _record = "field_stats", "gt4mi_field_stats", Stats.from_row

    def _result_block(self) -> tuple:
        return (_lib.STATS_SLOTS,)


def field_stats(*fields, other=None, origin: Optional[Sequence[int]] = None, domain: Optional[Sequence[int]] = None,
                halo=0) -> List[Stats]:
    """Statistics of ``fields`` over their compute domain, one :class:`Stats` each: one pass (per 8 fields) and one finishing
    launch on the current stream, then a synchronisation of that stream.

    ``fields``  :class:`DeviceArray`\\ s (IJK, or IJ) of float32 or float64, or anything ``as_device_array`` accepts; they may
                differ in address, strides and padding and share dtype, ``origin`` and ``domain``.
    ``other``   a second field for EVERY field (or a list, one per field, entries may be ``None``): the statistics are then
                those of ``a - b`` and ``dot`` is the sum of ``a * b``.  It may be broadcast (stride 0) along an axis, and an IJ
                field against IJK fields is: a weight such as a cell area.  With a weight ``sum`` ... ``max`` still describe
                ``a - w``; for the sum of ``a * w`` next to the statistics of ``a`` itself pass ``a`` twice, once alone and once
                with the weight: ``FieldStats([a, a], others=[None, w])`` -- two entries, one launch.
    ``halo``    an int, ``(hi, hj)`` or ``((lo_i, hi_i), (lo_j, hi_j))``: what surrounds the compute domain.  ``origin``
                defaults to ``(lo_i, lo_j, 0)``, ``domain`` to what remains of the first field's shape.

    Raises ``ValueError`` / ``TypeError`` (with the library's message) before any GPU work.  In a time loop build a
    :class:`FieldStats` once instead and read it a step late."""
    return _one_shot(FieldStats, fields, other, origin=origin, domain=domain, halo=halo)


# ---- per level: K profiles ---------------------------------------------------------------------------------------------------
#: the rows of a LevelStats result block, in order: the fields of Stats, then the mean
PROFILE_ROWS = Stats._fields + ("mean",)


class _Rows:
    """What :class:`Profile` and :class:`Lines` share: the nine rows as numpy arrays of ``_ndim`` dimensions and one shape
    (``_shape_error``: the refusal of anything else), the :class:`Stats` of one index, what follows from the rows, and equality."""

    __slots__ = PROFILE_ROWS
    _ndim, _shape_error = 0, ""

    def __init__(self, count, nonfinite, sum, sum_abs, sum_sq, min, max, dot, mean=None):  # noqa: A002 - the names of Stats
        nd = self._ndim
        self.count, self.nonfinite = (np.array(v, dtype=np.int64, ndmin=nd) for v in (count, nonfinite))
        self.sum, self.sum_abs, self.sum_sq, self.min, self.max, self.dot = (
            np.array(v, dtype=np.float64, ndmin=nd) for v in (sum, sum_abs, sum_sq, min, max, dot))
        if mean is None:
            with np.errstate(all="ignore"):
                mean = self.sum / self.count  # one IEEE division per level or line, as the kernel's
        self.mean = np.array(mean, dtype=np.float64, ndmin=nd)
        if any(getattr(self, name).shape != self.count.shape or self.count.ndim != nd for name in PROFILE_ROWS):
            raise ValueError(self._shape_error)

    def __getitem__(self, index) -> Stats:
        if self._ndim == 2:
            a, b = index
            index = int(a), int(b)
        else:
            index = int(index)
        return Stats(int(self.count[index]), int(self.nonfinite[index]), float(self.sum[index]), float(self.sum_abs[index]),
                     float(self.sum_sq[index]), float(self.min[index]), float(self.max[index]), float(self.dot[index]))

    @property
    def norm2(self) -> np.ndarray:
        with np.errstate(all="ignore"):
            return np.sqrt(self.sum_sq)

    @property
    def max_abs(self) -> np.ndarray:
        """max |x| per level or line (the CFL limit differs from one to the next); NaN where it holds a NaN."""
        return np.maximum(np.abs(self.min), np.abs(self.max))  # (numpy's maximum hands a NaN on)

    @property
    def all_finite(self) -> np.ndarray:
        return self.nonfinite == 0

    def __eq__(self, other) -> bool:
        """Bit for bit, NaN equal to NaN."""
        if not isinstance(other, type(self)):
            return NotImplemented
        return all(np.array_equal(getattr(self, n), getattr(other, n), equal_nan=True)
                   and np.array_equal(np.signbit(getattr(self, n)), np.signbit(getattr(other, n))) for n in PROFILE_ROWS)

    __hash__ = None  # type: ignore[assignment]


class Profile(_Rows):
    """The per-level values of one entry: numpy arrays of length ``nk`` for ``count``, ``nonfinite`` (int64), ``sum``,
    ``sum_abs``, ``sum_sq``, ``min``, ``max``, ``dot`` and ``mean`` (float64), with the NaN and signed-zero rules of
    :class:`Stats` level by level.  ``profile[k]`` is the :class:`Stats` of level ``k``; index 0 is the first level of the
    domain (``origin[2]``)."""

    __slots__ = ()
    _ndim, _shape_error = 1, "the rows of a Profile are one-dimensional and of one length"

    @classmethod
    def from_rows(cls, rows) -> "Profile":
        """From one ``(9, nk)`` block of a :class:`LevelStats` result."""
        rows = np.asarray(rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[0] != _lib.LEVEL_STATS_ROWS:
            raise ValueError(f"a result block has shape (9, nk), not {rows.shape}")
        return cls(*rows[:_lib.STATS_SLOTS], mean=rows[_lib.LEVEL_STATS_MEAN])

    @property
    def nk(self) -> int:
        return len(self.count)

    def __len__(self) -> int:
        return self.nk

    @property
    def first_nonfinite(self) -> Optional[int]:
        """The lowest level index with a NaN or +-Inf item, or ``None``."""
        bad = np.flatnonzero(self.nonfinite)
        return int(bad[0]) if bad.size else None

    def total(self) -> Stats:
        """The levels joined left to right as :func:`merge` does: exact counts and extremes, sums added in level order.  NOT
        the bits of :func:`field_stats` over the whole domain, whose additions are ordered by the whole domain."""
        return merge([self[k] for k in range(self.nk)])

    def __repr__(self) -> str:
        return f"Profile(nk={self.nk}, first_nonfinite={self.first_nonfinite})"


def merge_profiles(parts: Sequence[Profile]) -> Profile:
    """Join the per-rank profiles of a decomposed run on the host, level by level, IN THE ORDER GIVEN.  K is never split, so all
    parts have the same ``nk`` (``ValueError`` otherwise).  As with :func:`merge`: counts add exactly, ``min`` / ``max`` are
    joined exactly (NaN if any is NaN, -0 below +0), the sums are added left to right in float64 -- reproducible for a fixed
    process grid and rank order, NOT bit for bit what one undecomposed call gives.  ``mean`` is recomputed from the joined
    ``sum`` and ``count``.  No collective is made here; gather first, in rank order."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_profiles needs at least one Profile")
    for p in parts:
        if not isinstance(p, Profile):
            raise TypeError(f"merge_profiles joins Profile records, not {type(p).__name__}")
        if p.nk != parts[0].nk:
            raise ValueError(f"the parts of a decomposed run share their levels: nk = {parts[0].nk} and {p.nk} differ")
    levels = [merge([p[k] for p in parts]) for k in range(parts[0].nk)]
    return Profile(*(np.array([getattr(s, name) for s in levels]) for name in Stats._fields))


class LevelStats(_StatsCall):
    """The frozen form of :func:`level_stats`, with the arguments and defaults of :class:`FieldStats`; ``origin[2]`` /
    ``domain[2]`` select the levels, profile index 0 is level ``origin[2]``, and IJ fields give ``nk = 1``.  Arguments are
    checked (through the library's dry run), the descriptors, the workspace and the result buffer built ONCE; ``__call__()``
    makes only the ctypes call, on the stream that is current THEN, and does not synchronise; :meth:`get` synchronises that
    stream and returns one :class:`Profile` per entry.

    ``result`` is a float64 :class:`DeviceArray` of shape ``(n, 9, nk)`` (rows in the order of :data:`PROFILE_ROWS`);
    :meth:`profile` hands out one contiguous row of it, which a stencil takes as ``Field[K, np.float64]`` in the same stream
    with no synchronisation in between.  Every call overwrites it.

    The object holds raw pointers and weak references to the CALLER's objects, as :class:`FieldStats` does: it refuses to run
    once one of them has died."""

    _who, _entry, _record = "level_stats", "gt4mi_level_stats", Profile.from_rows

    def _result_block(self) -> tuple:
        return (_lib.LEVEL_STATS_ROWS, self.domain[2])

    @property
    def nk(self) -> int:
        return self.domain[2]

    def profile(self, name: str, entry: int = 0) -> DeviceArray:
        """The contiguous ``(nk,)`` device view of one row of ``result``: ``name`` is a field of :class:`Stats` or ``"mean"``.
        It holds what the LAST call left there, in stream order: pass it to a stencil as ``Field[K, np.float64]`` on the
        stream of that call and no synchronisation is needed."""
        return self._row("profile", name, entry)


def level_stats(*fields, other: Union[None, Any, Sequence[Any]] = None, origin: Optional[Sequence[int]] = None,
                domain: Optional[Sequence[int]] = None, halo=0) -> List[Profile]:
    """Per-level statistics of ``fields`` over their compute domain, one :class:`Profile` each: the synchronous one-shot form,
    with the arguments of :func:`field_stats`.  One pass (per 8 fields) and one finishing launch on the current stream, then a
    synchronisation of that stream.  With an IJ area weight as ``other``, ``dot`` is the area-weighted level sum.  In a time
    loop build a :class:`LevelStats` once instead and read it a step late."""
    return _one_shot(LevelStats, fields, other, origin=origin, domain=domain, halo=halo)


# ---- along a line: zonal means and their kin ------------------------------------------------------------------------------------
#: the rows of a LineStats result block, in order: those of a LevelStats block
LINE_ROWS = PROFILE_ROWS


def _np_minimum(a, b):
    """IEEE-754-2019 minimum, element-wise: NaN if either is NaN, -0 below +0."""
    return np.where(np.isnan(a) | np.isnan(b), np.nan, np.where(a < b, a, np.where(b < a, b, np.where(np.signbit(a), a, b))))


def _np_maximum(a, b):
    return np.where(np.isnan(a) | np.isnan(b), np.nan, np.where(a > b, a, np.where(b > a, b, np.where(np.signbit(a), b, a))))


class Lines(_Rows):
    """The per-line values of one entry: numpy arrays of shape ``(nA, nB)`` -- A < B the two axes other than the line axis, so
    ``[j, k]`` for lines along I -- for ``count``, ``nonfinite`` (int64), ``sum``, ``sum_abs``, ``sum_sq``, ``min``, ``max``,
    ``dot`` and ``mean`` (float64), with the NaN and signed-zero rules of :class:`Stats` line by line.  ``lines[a, b]`` is the
    :class:`Stats` of one line; index 0 is the first line of the domain."""

    __slots__ = ()
    _ndim, _shape_error = 2, "the rows of a Lines record are two-dimensional and of one shape"

    @classmethod
    def from_rows(cls, rows) -> "Lines":
        """From one ``(9, nB, nA)`` block of a :class:`LineStats` result."""
        rows = np.asarray(rows, dtype=np.float64)
        if rows.ndim != 3 or rows.shape[0] != _lib.LINE_STATS_ROWS:
            raise ValueError(f"a result block has shape (9, nB, nA), not {rows.shape}")
        rows = rows.transpose(0, 2, 1)
        return cls(*rows[:_lib.STATS_SLOTS], mean=rows[_lib.LINE_STATS_MEAN])

    @property
    def shape(self) -> tuple:
        return self.count.shape

    @property
    def first_nonfinite(self) -> Optional[tuple]:
        """``(a, b)`` of the first line with a NaN or +-Inf item -- lowest ``b``, then lowest ``a`` -- or ``None``."""
        bad = np.flatnonzero(self.nonfinite.T)
        return None if not bad.size else (int(bad[0] % self.shape[0]), int(bad[0] // self.shape[0]))

    def __repr__(self) -> str:
        return f"Lines(shape={self.shape}, first_nonfinite={self.first_nonfinite})"


def merge_lines(parts: Sequence[Lines]) -> Lines:
    """Join the per-rank results of ranks that split the LINE axis (ranks along I for zonal statistics) on the host, line by line,
    IN THE ORDER GIVEN; all parts have the same shape (``ValueError`` otherwise).  As with :func:`merge_profiles`: counts add
    exactly, ``min`` / ``max`` are joined exactly (NaN if any is NaN, -0 below +0), the sums are added left to right in float64 --
    reproducible for a fixed process grid and rank order, NOT bit for bit what one undecomposed call gives.  ``mean`` is recomputed
    from the joined ``sum`` and ``count``.  Ranks that split another axis hold different lines: concatenate their arrays instead.
    No collective is made here; gather first, in rank order."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_lines needs at least one Lines")
    for p in parts:
        if not isinstance(p, Lines):
            raise TypeError(f"merge_lines joins Lines records, not {type(p).__name__}")
        if p.shape != parts[0].shape:
            raise ValueError(f"the parts of a decomposed run share their lines: shapes {parts[0].shape} and {p.shape} differ")
    out = {name: getattr(parts[0], name) for name in Stats._fields}
    with np.errstate(all="ignore"):
        for p in parts[1:]:
            for name in Stats._fields:
                join = _np_minimum if name == "min" else _np_maximum if name == "max" else np.add
                out[name] = join(out[name], getattr(p, name))
    return Lines(**out)


class LineStats(_StatsCall):
    """The frozen form of :func:`line_stats`, with the arguments and defaults of :class:`FieldStats` and ``axis``: ``"I"`` (the
    zonal statistics), ``"J"``, ``"K"`` or 0, 1, 2 -- the axis ALONG which every line of the domain is reduced.  Arguments are
    checked (through the library's dry run), the descriptors, the workspace and the result buffer built ONCE; ``__call__()`` makes
    only the ctypes call, on the stream that is current THEN, and does not synchronise; :meth:`get` synchronises that stream and
    returns one :class:`Lines` per entry.

    ``result`` is a float64 :class:`DeviceArray` of shape ``(n, 9, nB, nA)`` (rows in the order of :data:`LINE_ROWS`; A < B the two
    other axes); :meth:`section` hands out one row of it as an ``(nA, nB)`` view, which a stencil takes as ``Field[JK]`` (axis
    I), ``Field[IK]`` (axis J) or ``Field[IJ]`` (axis K) of float64 in the same stream with no synchronisation in between.  Every
    call overwrites it.  ``path`` is the kernel the strides selected (``_lib.LINE_STATS_PATH_*``); it never changes the result.

    The order of the additions of a line depends on its length alone (csrc/line_stats.hip.h): the same line gives the same bits
    whatever the axis, the layout or the other lines are.  The object holds raw pointers and weak references to the CALLER's
    objects, as :class:`FieldStats` does: it refuses to run once one of them has died."""

    _who, _entry, _record = "line_stats", "gt4mi_line_stats", Lines.from_rows

    def __init__(self, fields: Sequence[Any], *, axis, others: Optional[Sequence[Any]] = None, origin: Optional[Sequence[int]] = None,
                 domain: Optional[Sequence[int]] = None, halo=0):
        self.axis = _axis_index(axis)
        super().__init__(fields, others=others, origin=origin, domain=domain, halo=halo)

    def _arguments(self) -> tuple:
        return (self._fields, self._others, self._n, self._domain3, self.axis, self._itemsize, self._workspace_ptr, self._workspace_bytes,
                self._result_ptr, FLAGS, STREAM, Out(ctypes.c_int64), Out(ctypes.c_int), Out(ctypes.c_int))

    def _result_block(self) -> tuple:
        a, b = (d for d in range(3) if d != self.axis)
        return (_lib.LINE_STATS_ROWS, self.domain[b], self.domain[a])

    def section(self, name: str, entry: int = 0) -> DeviceArray:
        """The ``(nA, nB)`` device view (byte strides ``(8, 8 * nA)``, no copy) of one row of ``result``: ``name`` is a field of
        :class:`Stats` or ``"mean"``.  It holds what the LAST call left there, in stream order: pass it to a stencil as
        ``Field[JK, np.float64]`` (axis I), ``Field[IK, ...]`` (axis J) or ``Field[IJ, ...]`` (axis K) on the stream of that call
        and no synchronisation is needed."""
        return self._row("section", name, entry).transpose()


def line_stats(*fields, axis, other: Union[None, Any, Sequence[Any]] = None, origin: Optional[Sequence[int]] = None,
               domain: Optional[Sequence[int]] = None, halo=0) -> List[Lines]:
    """Statistics of ``fields`` along every line of their compute domain along ``axis``, one :class:`Lines` each: the synchronous
    one-shot form, with the arguments of :func:`field_stats`.  One pass (per 8 fields) and, for lines of more than one segment,
    one finishing launch on the current stream, then a synchronisation of that stream.  With an IJ area weight as ``other``,
    ``dot`` is the area-weighted sum along the line.  In a time loop build a :class:`LineStats` once instead and read it a step
    late."""
    return _one_shot(LineStats, fields, other, axis=axis, origin=origin, domain=domain, halo=halo)
