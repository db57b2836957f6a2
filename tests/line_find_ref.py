"""The contract of ``gt4mi_line_find`` (include/gt4py_amd.h) restated twice: :func:`find_line` in plain Python, one item at a time
on numpy float64 scalars (numpy rounds every scalar operation once and fuses nothing), and :func:`find` / :func:`find_along` in
vectorised numpy, the lines side by side, which is what the tests use on whole boxes.  tests/test_line_find.py compares the two with
each other and with ``numpy.argmax`` / ``numpy.argmin``.  Test infrastructure; imports no product code."""

from __future__ import annotations

import numpy as np

WHATS = ("crossing", "argmax", "argmin")
DIRECTIONS = ("any", "rising", "falling")
ROWS = ("position", "coord", "extra")  # extra: the value at an extremum, the crossings of a line


def find_line(x, what, level=None, direction="any", reverse=False, coord=None, missing=np.nan):
    """One line, item by item: ``x`` (and ``coord``) 1-d arrays of one dtype.  Returns (position, coord, extra) as float64."""
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float64) and what in WHATS and direction in DIRECTIONS
    assert coord is None or np.asarray(coord).dtype == x.dtype
    D = np.float64
    n = len(x)
    y = [D(x[n - 1 - q] if reverse else x[q]) for q in range(n)]  # (the conversion is exact)
    zc = None if coord is None else [D(coord[n - 1 - q] if reverse else coord[q]) for q in range(n)]
    idx = (lambda q: n - 1 - q) if reverse else (lambda q: q)
    missing = D(missing)
    if what != "crossing":
        assert level is None
        best = 0
        for q in range(1, n):
            cand = y[best]
            if not cand != cand and (y[q] != y[q] or (y[q] > cand if what == "argmax" else y[q] < cand)):
                best = q
        position = D(idx(best))
        return position, (position if zc is None else zc[best]), y[best]
    L = D(level)
    found, position, where, crossings = False, missing, missing, 0
    if y[0] == L:
        found, crossings, position = True, 1, D(idx(0))
        where = position if zc is None else zc[0]
    with np.errstate(all="ignore"):
        for q in range(n - 1):
            rise = y[q] < L and y[q + 1] >= L
            fall = y[q] > L and y[q + 1] <= L
            if not {"any": rise or fall, "rising": rise, "falling": fall}[direction]:
                continue
            crossings += 1
            if found:
                continue
            found = True
            t = (L - y[q]) / (y[q + 1] - y[q])
            position = D(n - 1 - q) - t if reverse else D(q) + t
            where = position if zc is None else zc[q] + t * (zc[q + 1] - zc[q])
    return position, where, D(crossings)


def find(x, what, level=None, direction="any", reverse=False, coord=None, missing=np.nan):
    """The same along axis 0 of ``x`` of shape (n, ...); ``coord`` broadcasts against it.  Returns float64 of shape (3, ...):
    the rows of :data:`ROWS`."""
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float64) and what in WHATS and direction in DIRECTIONS
    n, rest = x.shape[0], x.shape[1:]
    y = (x[::-1] if reverse else x).astype(np.float64)
    zc = None
    if coord is not None:
        assert np.asarray(coord).dtype == x.dtype
        zc = np.broadcast_to(coord, x.shape)
        zc = (zc[::-1] if reverse else zc).astype(np.float64)
    idx = (lambda q: float(n - 1 - q)) if reverse else (lambda q: float(q))
    if what != "crossing":
        assert level is None
        cand, best = y[0].copy(), np.zeros(rest, dtype=np.int64)
        for q in range(1, n):
            beyond = y[q] > cand if what == "argmax" else y[q] < cand
            take = ~np.isnan(cand) & (np.isnan(y[q]) | beyond)
            cand, best = np.where(take, y[q], cand), np.where(take, q, best)
        position = ((n - 1 - best) if reverse else best).astype(np.float64)
        where = position if zc is None else np.take_along_axis(zc, best[None], 0)[0]
        return np.stack([position, where, cand])
    L = np.float64(level)
    found = y[0] == L
    crossings = found.astype(np.int64)
    position = np.where(found, idx(0), np.float64(missing))
    where = position.copy() if zc is None else np.where(found, zc[0], np.float64(missing))
    with np.errstate(all="ignore"):
        for q in range(n - 1):
            a, b = y[q], y[q + 1]
            rise, fall = (a < L) & (b >= L), (a > L) & (b <= L)
            hit = {"any": rise | fall, "rising": rise, "falling": fall}[direction]
            crossings = crossings + hit
            new = hit & ~found
            t = (L - a) / (b - a)
            p = idx(q) - t if reverse else idx(q) + t
            c = p if zc is None else zc[q] + t * (zc[q + 1] - zc[q])
            position, where, found = np.where(new, p, position), np.where(new, c, where), found | new
    return np.stack([position, where, crossings.astype(np.float64)])


def find_along(box, axis, what, level=None, direction="any", reverse=False, coord=None, missing=np.nan):
    """:func:`find` along ``axis`` of the IJK array ``box``; the coord is an IJK array or a 1-d array along the line.  Returns
    float64 of shape (3, nA, nB), A < B the two other axes."""
    def lines_first(v):
        v = np.asarray(v)
        return v.reshape((-1, 1, 1)) if v.ndim == 1 else np.moveaxis(v, axis, 0)

    return find(np.moveaxis(np.asarray(box), axis, 0), what, level, direction, reverse, None if coord is None else lines_first(coord), missing)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def same_bits(x, y):
    """Elementwise: the same bits, or NaN on both sides."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return (bits(x) == bits(y)) | (np.isnan(x) & np.isnan(y))
