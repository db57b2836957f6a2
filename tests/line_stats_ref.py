"""Two restatements of the order in which ``gt4mi_line_stats`` adds (csrc/line_stats.hip.h, header comment): :func:`line` in plain
Python, one line at a time, written as the kernels work; :func:`lines` in numpy, every line of a box at once, written as the
contract reads.  tests/test_line_stats.py holds each against the other bit for bit.

Imports no product code: the segment length ``g`` (GT4MI_LINE_STATS_SEGMENT) is an argument.  ``lines(a, b, axis, g)`` takes the
host copy of the compute-domain box (2-D or 3-D, float32 or float64; ``b`` may have extent 1 along an axis: a broadcast weight) and
returns the nine rows (the eight slots, then the mean) as a ``(9, nB, nA)`` float64 array -- A < B the two remaining axes, the
library's result block of one entry -- bit for bit what the kernels produce.

The order of a line, a function of its length n alone:
  segments  S = ceil(n / g); segment s is the items m in [s g, min(n, (s + 1) g))
  inside    four accumulator sets, set p takes the items with m mod 4 == p in increasing m; sums start at +0.0, min at +inf, max at
            -inf, counts at 0; a set whose sum |x| ended NaN sets min = max = NaN; the segment is (A0 + A1) + (A2 + A3), all four
            sets taking part, also one that owned no item
  across    the S segments are halved level by level, new[i] = old[2 i] + old[2 i + 1], an odd last one carried up unchanged
  mean      sum / count, one division
min / max join as IEEE-754-2019 minimum / maximum: NaN if either is NaN, min(-0, +0) = -0, max(-0, +0) = +0.
"""

from __future__ import annotations

import math

import numpy as np

from stats_ref import same_bits, terms  # noqa: F401  (same_bits: for the tests that compare against this file)

COUNT, NONFINITE, SUM, SUM_ABS, SUM_SQ, MIN, MAX, DOT, MEAN = range(9)
ROWS, SETS = 9, 4
SUMS = (SUM, SUM_ABS, SUM_SQ, DOT)


def segments(n: int, g: int) -> int:
    return -(-int(n) // g)


def halvings(count: int):
    """The number of values at every stage of the halving, from ``count`` down to 1."""
    counts = [int(count)]
    while counts[-1] > 1:
        counts.append((counts[-1] + 1) // 2)
    return counts


def depth(n: int, g: int) -> int:
    """Additions on the longest path from an item to its line's sum: a set's chain (the one onto +0.0 included), the two levels
    that join the sets and the halving levels."""
    return -(-min(int(n), g) // SETS) + 2 + len(halvings(segments(n, g))) - 1


# ---- plain Python: one line, as a lane works through it ---------------------------------------------------------------------------
def _minimum(a: float, b: float) -> float:
    if a != a or b != b:
        return math.nan
    if a == b:
        return a if math.copysign(1.0, a) < 0 else b
    return a if a < b else b


def _maximum(a: float, b: float) -> float:
    if a != a or b != b:
        return math.nan
    if a == b:
        return a if math.copysign(1.0, a) > 0 else b
    return a if a > b else b


def _join(u, v):
    out = [u[k] + v[k] for k in range(8)]
    out[MIN], out[MAX] = _minimum(u[MIN], v[MIN]), _maximum(u[MAX], v[MAX])
    return out


def line(a, b, g: int):
    """The nine values of ONE line: ``a`` and ``b`` (or None) are sequences of Python floats (float64 values of the items)."""
    n = len(a)
    values = []
    for first in range(0, n, g):
        sets = [[0.0, 0.0, 0.0, 0.0, 0.0, math.inf, -math.inf, 0.0] for _ in range(SETS)]
        for m in range(first, min(n, first + g)):
            acc = sets[m % SETS]
            x = a[m] if b is None else a[m] - b[m]
            acc[SUM] = acc[SUM] + x
            acc[SUM_ABS] = acc[SUM_ABS] + abs(x)
            acc[SUM_SQ] = acc[SUM_SQ] + x * x
            if x == x:  # the running extremes skip a NaN item (and order -0 below +0); the NaN is accounted for below
                acc[MIN], acc[MAX] = _minimum(acc[MIN], x), _maximum(acc[MAX], x)
            acc[NONFINITE] += 0.0 if math.isfinite(x) else 1.0
            acc[COUNT] += 1.0
            if b is not None:
                acc[DOT] = acc[DOT] + a[m] * b[m]
        for acc in sets:
            if acc[SUM_ABS] != acc[SUM_ABS]:
                acc[MIN] = acc[MAX] = math.nan
        values.append(_join(_join(sets[0], sets[1]), _join(sets[2], sets[3])))
    while len(values) > 1:
        nxt = [_join(values[2 * i], values[2 * i + 1]) for i in range(len(values) // 2)]
        if len(values) % 2:
            nxt.append(values[-1])
        values = nxt
    out = values[0]
    with np.errstate(all="ignore"):
        return out + [float(np.float64(out[SUM]) / np.float64(out[COUNT]))]


# ---- numpy: every line at once, as the contract reads -------------------------------------------------------------------------------
def _np_minimum(a, b):
    eq = np.where(np.signbit(a), a, b)
    return np.where(np.isnan(a) | np.isnan(b), np.nan, np.where(a < b, a, np.where(b < a, b, eq)))


def _np_maximum(a, b):
    eq = np.where(np.signbit(a), b, a)
    return np.where(np.isnan(a) | np.isnan(b), np.nan, np.where(a > b, a, np.where(b > a, b, eq)))


_JOIN = {"sum": np.add, "min": _np_minimum, "max": _np_maximum}
_START = {"sum": 0.0, "min": np.inf, "max": -np.inf}


def _ordered(term: np.ndarray, g: int, kind: str = "sum") -> np.ndarray:
    """``term`` (n, L) float64, one line per column, joined along axis 0 in the documented order -> (L,)."""
    n, count = term.shape
    nseg, per_set = segments(n, g), g // SETS
    padded = np.zeros((nseg * g, count))
    valid = np.zeros(nseg * g, dtype=bool)
    padded[:n], valid[:n] = term, True
    padded, valid = padded.reshape(nseg, per_set, SETS, count), valid.reshape(nseg, per_set, SETS, 1)
    join = _JOIN[kind]
    with np.errstate(all="ignore"):
        acc = np.full((nseg, SETS, count), _START[kind])
        for step in range(per_set):  # set p takes its items in increasing m
            acc = np.where(valid[:, step], join(acc, padded[:, step]), acc)
        level = join(join(acc[:, 0], acc[:, 1]), join(acc[:, 2], acc[:, 3]))
        while level.shape[0] > 1:
            m = level.shape[0]
            nxt = join(level[0:m - 1:2], level[1::2])
            level = np.concatenate([nxt, level[-1:]], axis=0) if m % 2 else nxt
    return level[0]


def lines(a, b=None, axis: int = 0, g: int = 128) -> np.ndarray:
    x, ax, sq, prod = terms(a, b)
    rest = [d for d in range(3) if d != axis]
    shape = (x.shape[rest[1]], x.shape[rest[0]])  # (nB, nA)

    def columns(t):  # (ni, nj, nk) -> (n, nB * nA): the line axis first, then B, then A (fastest)
        return np.ascontiguousarray(t.transpose(axis, rest[1], rest[0])).reshape(t.shape[axis], -1)

    cx = columns(x)
    out = np.zeros((ROWS, cx.shape[1]))
    out[COUNT] = cx.shape[0]
    out[NONFINITE] = np.count_nonzero(~np.isfinite(cx), axis=0)
    out[SUM], out[SUM_ABS], out[SUM_SQ] = _ordered(cx, g), _ordered(columns(ax), g), _ordered(columns(sq), g)
    out[MIN], out[MAX] = _ordered(cx, g, "min"), _ordered(cx, g, "max")
    if prod is not None:
        out[DOT] = _ordered(columns(prod), g)
    with np.errstate(all="ignore"):
        out[MEAN] = out[SUM] / out[COUNT]
    return out.reshape((ROWS,) + shape)


def by_line(a, b=None, axis: int = 0, g: int = 128) -> np.ndarray:
    """:func:`lines` through :func:`line`: every line of the box on its own, in plain Python (slow: small boxes only)."""
    a3 = terms(a, None)[0]
    b3 = None if b is None else np.broadcast_to(terms(b, None)[0], a3.shape)
    rest = [d for d in range(3) if d != axis]
    out = np.zeros((ROWS, a3.shape[rest[1]], a3.shape[rest[0]]))
    for ib in range(out.shape[1]):
        for ia in range(out.shape[2]):
            index = [slice(None)] * 3
            index[rest[0]], index[rest[1]] = ia, ib
            la = [float(v) for v in a3[tuple(index)]]
            lb = None if b3 is None else [float(v) for v in b3[tuple(index)]]
            out[:, ib, ia] = line(la, lb, g)
    return out


# ---- the host's choice of a kernel, restated ---------------------------------------------------------------------------------------
LANES, TILES, ITEMS = 0, 1, 2


def expected_path(strides, others, domain, axis: int, size: int) -> int:
    """``strides`` / ``others``: the byte strides of every field / every second field of a call.  TILES where the line axis has
    unit stride in all of them, else LANES where another axis has (0 allowed there in a second field), else ITEMS; an axis of
    extent 1 selects nothing."""
    def unit(ax):
        return all(s[ax] == size for s in strides) and all(o[ax] == size or (ax != axis and o[ax] == 0) for o in others)

    if unit(axis) and domain[axis] > 1:
        return TILES
    if any(unit(ax) and domain[ax] > 1 for ax in range(3) if ax != axis):
        return LANES
    return ITEMS
