"""The arithmetic contract of ``gt4mi_line_scan`` (include/gt4py_amd.h) restated twice: :func:`scan_line` in plain Python, one item
at a time on numpy scalars (numpy rounds every scalar operation once, to the operands' dtype, and fuses nothing), and
:func:`scan_along` in vectorised numpy, the lines side by side, which is what the tests use on whole boxes.  tests/test_line_scan.py
compares the two with each other and with ``numpy.cumsum`` / ``maximum.accumulate``.  Test infrastructure; imports no product code."""

from __future__ import annotations

import numpy as np

OPS = ("sum", "max", "min")


def identity(op, dtype):
    return np.dtype(dtype).type({"sum": 0.0, "max": -np.inf, "min": np.inf}[op])


def _accumulator(op, dtype, wide):
    return np.dtype(np.float64 if wide and op == "sum" else dtype)


def scan_line(x, op="sum", exclusive=False, reverse=False, weight=None, wide=False):
    """One line, item by item: ``x`` (and ``weight``) 1-d arrays of one dtype T; returns an array of T."""
    x = np.asarray(x)
    T, A = x.dtype.type, _accumulator(op, x.dtype, wide).type
    assert T in (np.float32, np.float64) and (weight is None or (op == "sum" and np.asarray(weight).dtype == x.dtype))
    n = len(x)
    order = range(n - 1, -1, -1) if reverse else range(n)
    out = np.empty(n, dtype=x.dtype)
    s = A(identity(op, A))
    with np.errstate(all="ignore"):
        for m, i in enumerate(order):
            before = s
            if op == "sum":
                t = A(x[i])
                if weight is not None:
                    t = t * A(weight[i])
                s = t if m == 0 else s + t
            elif m == 0:
                s = x[i]
            elif op == "max":
                s = s if (s != s or s > x[i]) else x[i]
            else:
                s = s if (s != s or s < x[i]) else x[i]
            out[i] = T(before if exclusive else s)
    return out


def scan(x, op="sum", exclusive=False, reverse=False, weight=None, wide=False):
    """The same along axis 0 of ``x`` of shape (n, ...); ``weight`` broadcasts against it.  Selects move items (``np.where``)."""
    x = np.asarray(x)
    T, A = x.dtype, _accumulator(op, x.dtype, wide)
    assert T in (np.float32, np.float64)
    if weight is not None:
        assert op == "sum" and np.asarray(weight).dtype == T
        weight = np.broadcast_to(weight, x.shape)
    if reverse:
        x = x[::-1]
        weight = None if weight is None else weight[::-1]
    n = x.shape[0]
    out = np.empty(x.shape, dtype=T)
    s = np.full(x.shape[1:], identity(op, A), dtype=A)
    with np.errstate(all="ignore"):
        for m in range(n):
            before = s
            if op == "sum":
                t = x[m].astype(A)
                if weight is not None:
                    t = t * weight[m].astype(A)
                s = t if m == 0 else s + t
            elif m == 0:
                s = x[m].copy()
            else:
                keep = (s != s) | ((s > x[m]) if op == "max" else (s < x[m]))
                s = np.where(keep, s, x[m])
            out[m] = (before if exclusive else s).astype(T)
    return out[::-1] if reverse else out


def scan_along(x, axis, op="sum", exclusive=False, reverse=False, weight=None, wide=False):
    """:func:`scan` along ``axis`` of the IJK array ``x``; the weight is an IJK array or a 1-d array along the line."""
    def lines_first(v):
        v = np.asarray(v)
        return v.reshape((-1, 1, 1)) if v.ndim == 1 else np.moveaxis(v, axis, 0)

    out = scan(np.moveaxis(np.asarray(x), axis, 0), op, exclusive, reverse, None if weight is None else lines_first(weight), wide)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def same_bits(x, y):
    """Elementwise: the same bits, or NaN on both sides."""
    x, y = np.asarray(x), np.asarray(y)
    return (bits(x) == bits(y)) | (np.isnan(x) & np.isnan(y))


def same_values(x, y):
    """Elementwise: equal (zeros of either sign are), or NaN on both sides."""
    x, y = np.asarray(x), np.asarray(y)
    return (x == y) | (np.isnan(x) & np.isnan(y))
