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
"""

from __future__ import annotations

import ctypes
import math
import weakref
from typing import Any, List, NamedTuple, Optional, Sequence

import numpy as np

from . import _lib
from .boundary import _halo4
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


def _native(fields, others, n: int, domain, itemsize: int, workspace, workspace_bytes: int, result, flags: int, stream):
    """The ctypes call; a refusal of the library becomes ``ValueError`` (``TypeError`` for what no kernel handles) with the
    library's message.  Returns (workspace bytes needed, kernels enqueued)."""
    needed, launches = ctypes.c_int64(0), ctypes.c_int(0)
    rc = _lib.load().gt4mi_field_stats(fields, others, n, domain, itemsize, workspace, workspace_bytes, result, flags, stream,
                                       ctypes.byref(needed), ctypes.byref(launches))
    if rc != _lib.OK:
        message = _lib.load().gt4mi_last_error().decode("utf-8", "replace")
        if rc == _lib.ERR_HIP:
            raise _lib.NativeError("gt4mi_field_stats", rc, message)
        raise (TypeError if rc == _lib.ERR_UNSUPPORTED else ValueError)(message)
    return needed.value, launches.value


class FieldStats:
    """The frozen form of :func:`field_stats`: arguments are checked (through the library's dry run), the descriptors, the
    workspace and the result buffer built ONCE; ``__call__()`` makes only the ctypes call, on the stream that is current THEN,
    and does not synchronise; :meth:`get` synchronises that stream and returns one :class:`Stats` per entry.

    ``result`` is a float64 :class:`DeviceArray` of shape ``(n, 8)`` (slots in the order of :class:`Stats`): a later kernel, or
    a captured graph, can read it on the device.  Every call overwrites it.

    The object holds raw pointers and weak references to the CALLER's objects, not the arrays: it refuses to run once one of
    them has died.  (An exporter that cannot be weakly referenced is held instead, so its memory stays valid.)"""

    def __init__(self, fields: Sequence[Any], *, others: Optional[Sequence[Any]] = None, origin: Optional[Sequence[int]] = None,
                 domain: Optional[Sequence[int]] = None, halo=0):
        fields = list(fields)
        arrays = [as_device_array(f) for f in fields]
        if not arrays:
            raise ValueError("field_stats needs at least one field")
        if others is None:
            others = [None] * len(fields)
        others = list(others)
        if len(others) != len(fields):
            raise ValueError(f"others must have one entry (or None) per field: {len(others)} for {len(fields)} fields")
        other_arrays = [None if o is None else as_device_array(o) for o in others]
        first = arrays[0]
        for a in arrays + [o for o in other_arrays if o is not None]:
            if a.dtype not in (np.dtype("float32"), np.dtype("float64")):
                raise TypeError(f"field_stats takes float32 or float64 fields, not {a.dtype}")
            if a.dtype != first.dtype:
                raise TypeError(f"the fields of one call share a dtype: {first.dtype} and {a.dtype} differ")
            if a.ndim not in (2, 3):
                raise ValueError(f"field_stats takes IJ or IJK fields, not a field of {a.ndim} dimension(s)")
        h = _halo4(halo)
        if origin is None:
            origin = (h[0], h[2], 0)
        origin = tuple(int(o) for o in origin)
        origin = origin + (0,) * (3 - len(origin))
        if len(origin) != 3:
            raise ValueError(f"origin must have at most three entries, not {origin}")
        shape3 = tuple(first.shape) + (1,) * (3 - first.ndim)
        if domain is None:
            domain = (shape3[0] - origin[0] - h[1], shape3[1] - origin[1] - h[3], shape3[2] - origin[2])
            if min(domain) < 1:
                raise ValueError(f"halo {h} and origin {origin} leave no domain in a field of shape {first.shape}")
        domain = tuple(int(d) for d in domain)
        domain = domain + (1,) * (3 - len(domain))
        if len(domain) != 3:
            raise ValueError(f"domain must have at most three entries, not {domain}")
        self.origin, self.domain = origin, domain
        self._itemsize = first.itemsize
        self._n = len(arrays)

        def describe(a, weight):
            shape = tuple(a.shape) + (1,) * (3 - a.ndim)
            strides = tuple(a.strides) + (0,) * (3 - a.ndim)
            # a broadcast axis of a weight (stride 0) has no origin of its own
            org = tuple(0 if weight and s == 0 else o for o, s in zip(origin, strides))
            return _lib.Field.make(a.ptr, shape, strides, org)

        self._fields = (_lib.Field * self._n)()
        self._others = (_lib.Field * self._n)()  # (data == NULL: no second field)
        for n, (a, o) in enumerate(zip(arrays, other_arrays)):
            self._fields[n] = describe(a, False)
            if o is not None:
                self._others[n] = describe(o, True)
        self._domain3 = _lib.domain3(domain)
        # every check of the library, nothing enqueued; also: the workspace the call needs and how many kernels it makes
        needed, self.launches = _native(self._fields, self._others, self._n, self._domain3, self._itemsize, None, 0, None,
                                        _lib.STATS_DRY_RUN, None)
        # (last: none of the checks above needs a device)
        for a in arrays + [o for o in other_arrays if o is not None]:
            if not a.tensor.is_cuda:
                raise TypeError("field_stats works on device fields; a host array was passed")
        import torch

        self._workspace = torch.empty(needed // 8, dtype=torch.float64, device=first.tensor.device)
        self.result = DeviceArray(torch.zeros((self._n, _lib.STATS_SLOTS), dtype=torch.float64, device=first.tensor.device))
        self._workspace_bytes = needed
        # the buffers against the fields (overlap, alignment): the dry run once more, now with them
        _native(self._fields, self._others, self._n, self._domain3, self._itemsize, self._workspace.data_ptr(), needed,
                self.result.ptr, _lib.STATS_DRY_RUN, None)
        # what must stay alive is what the CALLER holds (see HaloFill)
        self._refs, self._held = [], []
        for f in fields + [o for o in others if o is not None]:
            try:
                self._refs.append(weakref.ref(f))
            except TypeError:
                self._held.append(f)
        self._current_stream = torch.cuda.current_stream
        self._stream = None
        self._lib = _lib.load()

    def __call__(self) -> None:
        if any(r() is None for r in self._refs):
            raise RuntimeError("FieldStats: an array this call was bound to no longer exists; build a new FieldStats")
        self._stream = self._current_stream()
        rc = self._lib.gt4mi_field_stats(self._fields, self._others, self._n, self._domain3, self._itemsize,
                                         self._workspace.data_ptr(), self._workspace_bytes, self.result.ptr, 0,
                                         self._stream.cuda_stream, None, None)
        if rc != _lib.OK:
            _lib.check("gt4mi_field_stats", rc)

    def get(self) -> List[Stats]:
        """Synchronise the stream of the last call and return its results (``RuntimeError`` before the first call)."""
        if self._stream is None:
            raise RuntimeError("FieldStats.get: the object has not been called yet")
        self._stream.synchronize()
        return [Stats.from_row(row) for row in self.result.tensor.cpu().numpy()]


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
    if isinstance(other, (list, tuple)):
        others = list(other)
    else:
        others = None if other is None else [other] * len(fields)
    frozen = FieldStats(fields, others=others, origin=origin, domain=domain, halo=halo)
    frozen()
    return frozen.get()
