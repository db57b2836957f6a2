"""``gt4py_amd.histogram`` -- how the values of ``hip:mi300`` fields are distributed: one-launch histograms over the whole box or
per level, exact and bit-reproducible.

The diagnostics family gives moments, extrema and places; none of it says how the values are distributed: the PDF of
precipitation, the median of a field, the fraction of points above a threshold per level, the contoured-frequency-by-altitude
diagram (CFAD), the same PDF accumulated over a whole run.  A stencil cannot write it (no reduction, and the result has another
shape than the fields).  ``gt4mi_field_histogram`` (csrc/field_histogram.hip.h) reads up to eight fields ONCE in one launch on the
current stream, without synchronisation, allocation or workspace, and leaves int64 counters on the device.

    from gt4py_amd import histogram
    pdf = histogram.Histogram.uniform([precip], 0.0, 50.0, 100, accumulate=True, halo=3)   # the PDF of the whole run
    cfad = histogram.Histogram([w], edges=w_edges, by="K", halo=3)                         # per level, every step anew
    for step in range(steps):
        physics(precip, w, ...)               # stencils
        pdf(); cfad()                         # one call each on the current stream
    p, = pdf.get()                            # a Hist: p.counts, p.below, p.above, p.nan, p.quantile(0.5)
    c, = cfad.get()                           # c.counts is (nk, nb); c.fraction_above(1.0) is a profile

THE CONTRACT (include/gt4py_amd.h): ``nb + 1`` float64 edges ``e[0] < ... < e[nb]``, all finite.  Every item of the box, converted
exactly to float64, lands in exactly one counter: ``nan``, ``below`` (``x < e[0]``), ``above`` (``x > e[nb]``), else the bin ``b``
with ``e[b] <= x < e[b+1]``, the last bin closed -- ``numpy.histogram``'s bins.  The counters are integers, so a result is the
same bits whatever the layout, the kernel path or the device, and the histograms of the parts of a decomposed field add up to the
histogram of the whole (:func:`merge_histograms`), bit for bit.
"""

from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np

from . import _lib
from ._bound import FLAGS, FLOATS, STREAM, Bound, Out, _as_list, _box_of, _halo4, field_table, one_shot
from .storage.device_array import DeviceArray, as_device_array

BYS = {None: _lib.HISTOGRAM_WHOLE, "K": _lib.HISTOGRAM_BY_K}
PATHS = {_lib.HISTOGRAM_PATH_ROWS: "rows", _lib.HISTOGRAM_PATH_ITEMS: "items"}


class Hist:
    """The histogram of one field: ``edges`` (``nb + 1`` float64), ``counts`` (int64, ``(nb,)``, or ``(nk, nb)`` per level) and
    the three counters beside the bins -- ``below`` (``x < edges[0]``, -inf included), ``above`` (``x > edges[-1]``, +inf included)
    and ``nan`` -- as ints, or as ``(nk,)`` int64 arrays per level.  ``inside`` is the sum of the bins, ``total`` the sum of
    everything: the items of the box (of a level)."""

    __slots__ = ("edges", "counts", "below", "above", "nan")

    def __init__(self, edges, counts, below=0, above=0, nan=0):
        self.edges = np.array(edges, dtype=np.float64)
        self.counts = np.array(counts, dtype=np.int64)
        if self.edges.ndim != 1 or self.counts.ndim not in (1, 2) or self.counts.shape[-1] != self.edges.size - 1 or self.edges.size < 2:
            raise ValueError(f"a Hist has nb + 1 edges and (nb,) or (nk, nb) counts, not {self.edges.shape} and {self.counts.shape}")
        rows = self.counts.shape[:-1]
        self.below, self.above, self.nan = (np.array(v, dtype=np.int64) if rows else int(v) for v in (below, above, nan))
        if rows and any(v.shape != rows for v in (self.below, self.above, self.nan)):
            raise ValueError(f"below, above and nan of a per-level Hist have one entry per level ({rows[0]})")

    @classmethod
    def from_rows(cls, edges, rows, per_level: bool) -> "Hist":
        """From one ``(nrows, nb + 3)`` block of a :class:`Histogram` result."""
        rows = np.asarray(rows, dtype=np.int64)
        nb = rows.shape[-1] - _lib.HISTOGRAM_EXTRA
        if not per_level:
            rows = rows[0]
        return cls(edges, rows[..., :nb], rows[..., nb + _lib.HISTOGRAM_BELOW], rows[..., nb + _lib.HISTOGRAM_ABOVE],
                   rows[..., nb + _lib.HISTOGRAM_NAN])

    @property
    def inside(self):
        """The items inside ``[edges[0], edges[-1]]`` (per level: an array)."""
        s = self.counts.sum(axis=-1)
        return s if self.counts.ndim == 2 else int(s)

    @property
    def total(self):
        """Every item of the box (of each level): the bins, ``below``, ``above`` and ``nan``."""
        return self.inside + self.below + self.above + self.nan

    def cdf(self) -> np.ndarray:
        """The cumulative distribution of the in-range items at the UPPER edge of every bin, ``(nb,)`` or ``(nk, nb)``: the
        last entry is 1; NaN where ``inside`` is 0."""
        with np.errstate(all="ignore"):
            return np.cumsum(self.counts, axis=-1) / np.asarray(self.inside, dtype=np.float64)[..., None]

    def quantile(self, q: float):
        """The ``q`` quantile (0 <= q <= 1) of the items INSIDE the edges, taken as spread evenly over their bin: linear inside
        the bin that holds the ``q * inside``-th item.  AN ESTIMATE: its error is at most the width of that bin.  A float, or
        ``(nk,)`` per level; NaN where ``inside`` is 0."""
        q = float(q)
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"a quantile is between 0 and 1, not {q}")
        counts = np.atleast_2d(self.counts)
        cum = np.cumsum(counts, axis=-1)
        inside = cum[:, -1]
        target = q * inside.astype(np.float64)
        b = np.argmax((cum >= target[:, None]) & (cum > 0), axis=-1)  # the first bin that is not empty and reaches the target
        rows = np.arange(counts.shape[0])
        here = counts[rows, b].astype(np.float64)
        with np.errstate(all="ignore"):
            t = (target - (cum[rows, b] - counts[rows, b])) / here
            out = np.where(inside > 0, self.edges[b] + t * (self.edges[b + 1] - self.edges[b]), np.nan)
        return out if self.counts.ndim == 2 else float(out[0])

    def fraction_above(self, x: float):
        """The fraction of the items that are not NaN with a value >= ``x``, for ``x`` on an edge OTHER THAN THE LAST (a value
        off the edges is refused: the counts cannot say it).  For the last edge it is the fraction with a value > ``x``, strictly:
        the last bin is closed, so the items equal to ``edges[-1]`` are counted in it and cannot be told from the rest of that
        bin.  A float, or ``(nk,)`` per level; NaN where every item is a NaN."""
        at = np.flatnonzero(self.edges == float(x))
        if at.size == 0:
            raise ValueError(f"fraction_above takes a value on an edge; {x!r} is not one of the {self.edges.size} edges")
        with np.errstate(all="ignore"):
            out = (self.counts[..., at[0]:].sum(axis=-1) + self.above) / np.asarray(self.total - self.nan, dtype=np.float64)
        return out if self.counts.ndim == 2 else float(out)

    def __repr__(self) -> str:
        return f"Hist(bins={self.edges.size - 1}, counts={self.counts.shape}, total={np.sum(self.total)})"


def merge_histograms(parts: Sequence[Hist]) -> Hist:
    """Add the records of the parts of a decomposed field (or of several steps): every counter adds exactly, so the result IS the
    histogram of the whole, bit for bit, in any order.  The parts must have identical edges and shapes.  No collective is made
    here; gather the records first."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge_histograms needs at least one Hist")
    for p in parts:
        if not isinstance(p, Hist):
            raise TypeError(f"merge_histograms joins Hist records, not {type(p).__name__}")
    first = parts[0]
    for p in parts[1:]:
        if p.edges.shape != first.edges.shape or not np.array_equal(p.edges, first.edges):
            raise ValueError("merge_histograms adds records with identical edges; these differ")
        if p.counts.shape != first.counts.shape:
            raise ValueError(f"merge_histograms adds records of one shape: {first.counts.shape} and {p.counts.shape} differ")
    return Hist(first.edges, sum(p.counts for p in parts), sum(p.below for p in parts), sum(p.above for p in parts),
                sum(p.nan for p in parts))


class Histogram(Bound):
    """The frozen form of :func:`histogram`: arguments are checked (through the library's dry run, which also checks the edges:
    finite and strictly increasing), the descriptors, a float64 device copy of the edges and the int64 result built ONCE;
    ``__call__()`` makes only the ctypes call, on the stream that is current THEN, and does not synchronise; :meth:`get`
    synchronises and returns one :class:`Hist` per field.

    ``result`` is an int64 :class:`DeviceArray` of shape ``(nf, nrows, nb + 3)``, ``nrows`` 1 or ``nk``; the last three columns
    are ``below``, ``above`` and ``nan``.  A call zeroes it first, in stream order; with ``accumulate=True`` a call ADDS to it
    (a run-long PDF) and :meth:`reset` zeroes it.  ``path`` is ``"rows"`` (every field has a unit-stride axis inside a row's
    box) or ``"items"``; ``launches`` the kernels a call enqueues.  The edges cannot be changed: build a new object.  The object
    holds raw pointers and weak references to the CALLER's fields, not the arrays: it refuses to run once one has died."""

    _entry, _dry_run_bit = "gt4mi_field_histogram", _lib.HISTOGRAM_DRY_RUN
    _edges_ptr = _result_ptr = None

    def _arguments(self) -> tuple:
        return (self._fields, self._n, self._extent3, self._size, self.bins, self._edges_ptr, self._edges_host, self._by, self._result_ptr,
                FLAGS, STREAM, Out(ctypes.c_int), Out(ctypes.c_int))

    def __init__(self, fields, *, edges, by: Optional[str] = None, accumulate: bool = False, halo=0, origin: Optional[Sequence[int]] = None,
                 domain: Optional[Sequence[int]] = None):
        fields = _as_list(fields)
        if not fields:
            raise ValueError("histogram needs at least one field")
        if by not in BYS:
            raise ValueError(f"by must be None (the whole box) or 'K' (per level), not {by!r}")
        arrays = [as_device_array(f) for f in fields]
        first = arrays[0]
        for a in arrays:
            if a.dtype not in FLOATS:
                raise TypeError(f"histogram takes float32 or float64 fields, not {a.dtype}")
            if a.dtype != first.dtype:
                raise TypeError(f"the fields of one call share a dtype: {first.dtype} and {a.dtype} differ")
            if a.ndim not in (2, 3):
                raise ValueError(f"histogram takes IJ or IJK fields, not a field of {a.ndim} dimension(s)")
        halo4 = _halo4(halo)
        if min(halo4) < 0:
            raise ValueError(f"halo widths must not be negative: {halo4}")
        try:
            e = np.array(edges, dtype=np.float64)
        except (ValueError, TypeError) as exc:
            raise ValueError(f"edges must be one array of nb + 1 numbers or one per field, all of one length: {exc}") from None
        if e.ndim == 2 and e.shape[0] != len(arrays):
            raise ValueError(f"one set of edges for every field or one per field: {e.shape[0]} sets for {len(arrays)} field(s)")
        if e.ndim not in (1, 2) or e.shape[-1] < 2:
            raise ValueError(f"edges must be one array of nb + 1 >= 2 numbers or one per field, not an array of shape {e.shape}")
        #: ``edges``: the float64 host copy, ``(nb + 1,)`` or ``(nf, nb + 1)``; ``bins``: nb
        self.edges, self.bins, self.by, self.accumulate = np.ascontiguousarray(e), int(e.shape[-1]) - 1, by, bool(accumulate)
        self.origin, self.domain = origin, domain = _box_of(first, halo4, origin, domain, 1)
        self._n, self._size, self._by = len(arrays), first.itemsize, BYS[by]
        self._fields = field_table(arrays, origin)
        self._extent3 = _lib.domain3(domain)
        self._edges_host = self.edges.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
        self._flags = (_lib.HISTOGRAM_ACCUMULATE if self.accumulate else 0) | (_lib.HISTOGRAM_EDGES_PER_FIELD if e.ndim == 2 else 0)
        self.rows = domain[2] if by == "K" else 1

        def allocate(torch, device, outs):
            self._edges_device = torch.from_numpy(self.edges).to(device)
            self.result = DeviceArray(torch.zeros((self._n, self.rows, self.bins + _lib.HISTOGRAM_EXTRA), dtype=torch.int64, device=device))
            self._edges_ptr, self._result_ptr = self._edges_device.data_ptr(), self.result.ptr

        path, self.launches = self._own_buffers("histogram", arrays, allocate)  # (the library's checks: the edges among them)
        self.path = PATHS.get(path)
        self._bind("histogram", arrays, fields)

    @classmethod
    def uniform(cls, fields, lo: float, hi: float, bins: int, **kwargs) -> "Histogram":
        """``bins`` bins of equal width between ``lo`` and ``hi``: the edges are ``numpy.linspace(lo, hi, bins + 1)``, made on the
        host, and THEY are the contract (an item belongs to the bin the comparisons against them name)."""
        if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or bins < 1:
            raise ValueError(f"bins must be a positive int, not {bins!r}")
        return cls(fields, edges=np.linspace(float(lo), float(hi), int(bins) + 1), **kwargs)

    def reset(self) -> None:
        """Zero the result on the current stream, in stream order (for ``accumulate=True``: the start of a new period)."""
        self.result.tensor.zero_()

    def counts(self, entry: int = 0) -> DeviceArray:
        """The device view (no copy) of the bins of one field, ``(nb,)`` or ``(nk, nb)`` int64: what the last call (or the calls
        since the last :meth:`reset`) left there, in stream order."""
        block = self.result[self._index(entry)]
        return block[:, : self.bins] if self.by == "K" else block[0, : self.bins]

    def get(self) -> List[Hist]:
        """Synchronise the device and return one :class:`Hist` per field."""
        import torch

        torch.cuda.synchronize(self.result.tensor.device)
        blocks = self.result.tensor.cpu().numpy()
        return [Hist.from_rows(self.edges[n] if self.edges.ndim == 2 else self.edges, blocks[n], self.by == "K") for n in range(self._n)]


def histogram(*fields, edges, by: Optional[str] = None, halo=0, origin: Optional[Sequence[int]] = None,
              domain: Optional[Sequence[int]] = None) -> List[Hist]:
    """The histograms of ``fields`` over their compute domain, one :class:`Hist` each: one kernel launch on the current stream,
    then a synchronisation.

    ``fields``  :class:`DeviceArray`\\ s (IJK, or IJ: one level) of one dtype, float32 or float64, or anything ``as_device_array``
                accepts, at most 8; they may differ in address, strides and padding.  None is written.
    ``edges``   ``nb + 1`` increasing finite numbers (at most 4096 bins) for every field, or a list of one such array per field, all
                of one length.  Kept as float64.
    ``by``      ``None``: one histogram of the whole box; ``"K"``: one per level (``Hist.counts`` is ``(nk, nb)``).
    ``halo``    an int, ``(hi, hj)`` or ``((lo_i, hi_i), (lo_j, hi_j))``: what surrounds the compute domain and is NOT counted.
                ``origin`` defaults to ``(lo_i, lo_j, 0)``, ``domain`` to what remains of the first field's shape.

    Raises ``ValueError`` / ``TypeError`` (with the library's message) before any GPU work.  In a time loop build a
    :class:`Histogram` once instead and read it a step late."""
    return one_shot(Histogram, fields, edges=edges, by=by, halo=halo, origin=origin, domain=domain)
