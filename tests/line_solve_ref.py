"""The arithmetic contract of ``gt4mi_line_solve`` (include/gt4py_amd.h) restated in plain Python: numpy arrays of the fields'
dtype, one numpy operation per operation of the contract (numpy rounds every elementwise operation once, to the arrays' dtype,
and fuses nothing), the lines side by side along the trailing axes.  Test infrastructure; imports no product code."""

from __future__ import annotations

import numpy as np


def _thomas(a, b, c, d):
    """The non-periodic solve: a, b, c, d of shape (n, ...), one dtype.  a[0] and c[n-1] are never read."""
    n = b.shape[0]
    cp = [None] * n
    dp = [None] * n
    if n > 1:
        cp[0] = c[0] / b[0]
    dp[0] = d[0] / b[0]
    for m in range(1, n):
        den = b[m] - a[m] * cp[m - 1]
        if m < n - 1:
            cp[m] = c[m] / den
        dp[m] = (d[m] - a[m] * dp[m - 1]) / den
    x = [None] * n
    x[n - 1] = dp[n - 1]
    for m in range(n - 2, -1, -1):
        x[m] = dp[m] - cp[m] * x[m + 1]
    return np.stack(x)


def solve(a, b, c, d, periodic=False):
    """x of ``a[m] x[m-1] + b[m] x[m] + c[m] x[m+1] = d[m]`` along axis 0 of arrays of one shape (n, ...) and one dtype."""
    a, b, c, d = np.broadcast_arrays(a, b, c, d)
    assert a.dtype == b.dtype == c.dtype == d.dtype and a.dtype in (np.float32, np.float64)
    T = a.dtype.type
    n = b.shape[0]
    with np.errstate(all="ignore"):
        if not periodic:
            return _thomas(a, b, c, d)
        assert n >= 3
        alpha, beta, gamma = c[n - 1], a[0], -b[0]
        bb = b.copy()
        bb[0] = b[0] - gamma
        bb[n - 1] = b[n - 1] - (alpha * beta) / gamma
        u = np.zeros_like(b)
        u[0], u[n - 1] = gamma, alpha
        q = _thomas(a, bb, c, u)
        y = _thomas(a, bb, c, d)
        fact = (y[0] + (beta * y[n - 1]) / gamma) / ((T(1) + q[0]) + (beta * q[n - 1]) / gamma)
        return y - fact * q


def solve_along(a, b, c, d, axis, periodic=False):
    """:func:`solve` along ``axis`` of the IJK array ``d``; a coefficient is an IJK array or a 1-d array along the line."""
    def lines_first(v):
        v = np.asarray(v)
        return v.reshape((-1, 1, 1)) if v.ndim == 1 else np.moveaxis(v, axis, 0)

    x = solve(lines_first(a), lines_first(b), lines_first(c), np.moveaxis(np.asarray(d), axis, 0), periodic)
    return np.ascontiguousarray(np.moveaxis(x, 0, axis))


def dense(a, b, c, periodic=False):
    """The matrix of one line (1-d coefficients), float64."""
    n = len(b)
    A = np.zeros((n, n))
    for m in range(n):
        A[m, m] = b[m]
        if m > 0:
            A[m, m - 1] = a[m]
        if m < n - 1:
            A[m, m + 1] = c[m]
    if periodic:
        A[0, n - 1] += a[0]
        A[n - 1, 0] += c[n - 1]
    return A


def same_bits(x, y):
    """Elementwise: the same bits, or NaN on both sides."""
    x, y = np.asarray(x), np.asarray(y)
    ut = {4: np.uint32, 8: np.uint64}[x.dtype.itemsize]
    return (np.ascontiguousarray(x).view(ut) == np.ascontiguousarray(y).view(ut)) | (np.isnan(x) & np.isnan(y))
