"""The arithmetic contract of ``gt4mi_horizontal_interp`` (include/gt4py_amd.h) restated twice: ``interp_point`` in plain Python
floats -- IEEE float64, one rounding per operation --, one destination point at a time, and ``interp`` with numpy float64 arrays,
the same operations in the same order elementwise (numpy fuses nothing), which is what the tests of whole fields use.
tests/test_horizontal_interp.py holds the two against each other bit for bit.  Test infrastructure; imports no product code and
(at import) no torch.

float32 inputs are widened exactly (``float(...)`` / ``astype(float64)``); the caller rounds the result once (``numpy.astype``).

Geometry: ``src`` is the READABLE box of a field, the domain grown by ``reach = (lo_i, hi_i, lo_j, hi_j)``: domain point (0, 0) is
``src[lo_i, lo_j]``, the domain has ``ni = src.shape[0] - lo_i - hi_i`` by ``nj`` points.  Positions are in index units of the
domain; in relative mode they are displacements from the destination point's own index."""

from __future__ import annotations

import math

import numpy as np

NEAREST, LINEAR, CUBIC, CUBIC_MONOTONE = "nearest", "linear", "cubic", "cubic_monotone"
METHODS = (NEAREST, LINEAR, CUBIC, CUBIC_MONOTONE)
NAN = float("nan")
QNAN = {4: 0x7FC0_0000, 8: 0x7FF8_0000_0000_0000}  # what nearest stores at a NaN position


# ---- one point, plain Python ---------------------------------------------------------------------------------------------------
def clamp_index(v: int, lo: int, hi: int) -> int:
    return lo if v < lo else (hi if v > hi else v)


def cubic_weights(t: float):
    """Lagrange on the nodes -1, 0, 1, 2."""
    a, c, d = t + 1.0, t - 1.0, t - 2.0
    return [-(((t * c) * d) / 6.0), ((a * c) * d) / 2.0, -(((a * t) * d) / 2.0), ((a * t) * c) / 6.0]


def axis(p: float, index: int, relative: bool, lo: int, n: int, hi: int, method: str):
    """Steps 1-4 for one axis: (clamped indices, weights, the position is NaN).  Indices are in domain units, -lo ... n - 1 + hi."""
    imin, imax = -lo, n - 1 + hi
    xmin, xmax = float(imin), float(imax)
    if relative:
        p = float(index) + p
    x = xmin if p < xmin else (xmax if p > xmax else p)
    nan = x != x
    if method == NEAREST:
        return [clamp_index(imin if nan else math.floor(x + 0.5), imin, imax)], [1.0], nan
    b = imin if nan else math.floor(x)
    t = x - float(b)
    if method == LINEAR:
        return [clamp_index(b + m, imin, imax) for m in (0, 1)], [1.0 - t, t], nan
    return [clamp_index(b + m, imin, imax) for m in (-1, 0, 1, 2)], cubic_weights(t), nan


def combine(w, v) -> float:
    """((w0*v0 + w1*v1) + w2*v2) + w3*v3: every product rounded before its addition."""
    r = w[0] * v[0]
    for m in range(1, len(w)):
        r = r + w[m] * v[m]
    return r


def fmin(a: float, b: float) -> float:
    return b if b < a else a


def fmax(a: float, b: float) -> float:
    return b if b > a else a


def interp_point(level: np.ndarray, pi: float, pj: float, i: int, j: int, method: str, relative: bool, reach):
    """One point of one level (``level``: the readable box, 2-d) as a Python float -- or, for ``nearest``, the source ITEM itself
    (None at a NaN position: the canonical quiet NaN is stored)."""
    lo_i, hi_i, lo_j, hi_j = reach
    ni, nj = level.shape[0] - lo_i - hi_i, level.shape[1] - lo_j - hi_j
    ii, wi, nan_i = axis(float(pi), i, relative, lo_i, ni, hi_i, method)
    jj, wj, nan_j = axis(float(pj), j, relative, lo_j, nj, hi_j, method)
    if method == NEAREST:
        return None if nan_i or nan_j else level[ii[0] + lo_i, jj[0] + lo_j]
    rows = [combine(wi, [float(level[c + lo_i, r + lo_j]) for c in ii]) for r in jj]
    out = combine(wj, rows)
    if method == CUBIC_MONOTONE:
        c00, c10 = float(level[ii[1] + lo_i, jj[1] + lo_j]), float(level[ii[2] + lo_i, jj[1] + lo_j])
        c01, c11 = float(level[ii[1] + lo_i, jj[2] + lo_j]), float(level[ii[2] + lo_i, jj[2] + lo_j])
        mn = fmin(fmin(c00, c10), fmin(c01, c11))
        mx = fmax(fmax(c00, c10), fmax(c01, c11))
        out = mn if out < mn else (mx if out > mx else out)
    return out


# ---- whole fields, numpy: the same operations elementwise ------------------------------------------------------------------------
def _axis_np(p, index, relative, lo, n, hi, method):
    imin, imax = -lo, n - 1 + hi
    xmin, xmax = float(imin), float(imax)
    p = p.astype(np.float64)
    if relative:
        p = index.astype(np.float64) + p
    x = np.where(p < xmin, xmin, np.where(p > xmax, xmax, p))
    nan = x != x
    safe = np.where(nan, xmin, x)
    if method == NEAREST:
        return [np.clip(np.floor(safe + 0.5).astype(np.int64), imin, imax)], [None], nan
    b = np.floor(safe).astype(np.int64)
    t = x - b.astype(np.float64)
    if method == LINEAR:
        return [np.clip(b + m, imin, imax) for m in (0, 1)], [1.0 - t, t], nan
    a, c, d = t + 1.0, t - 1.0, t - 2.0
    w = [-(((t * c) * d) / 6.0), ((a * c) * d) / 2.0, -(((a * t) * d) / 2.0), ((a * t) * c) / 6.0]
    return [np.clip(b + m, imin, imax) for m in (-1, 0, 1, 2)], w, nan


def _combine_np(w, v):
    r = w[0] * v[0]
    for m in range(1, len(w)):
        r = r + w[m] * v[m]
    return r


def interp(src: np.ndarray, pos_i: np.ndarray, pos_j: np.ndarray, method: str, relative: bool = False, reach=(0, 0, 0, 0)) -> np.ndarray:
    """``src`` (ni + lo_i + hi_i, nj + lo_j + hi_j, nk), the readable box -> the domain (ni, nj, nk) in the dtype of ``src``, rounded
    once.  ``pos_i`` / ``pos_j`` are (ni, nj) -- a Field[IJ], every level shares it -- or (ni, nj, nk), float32 or float64."""
    assert method in METHODS and src.ndim == 3
    lo_i, hi_i, lo_j, hi_j = reach
    ni, nj, nk = src.shape[0] - lo_i - hi_i, src.shape[1] - lo_j - hi_j, src.shape[2]
    if pos_i.ndim == 2:
        pos_i = pos_i[:, :, None]
    if pos_j.ndim == 2:
        pos_j = pos_j[:, :, None]
    assert pos_i.shape[:2] == (ni, nj) and pos_j.shape[:2] == (ni, nj)
    pos_i, pos_j = np.broadcast_to(pos_i, (ni, nj, nk)), np.broadcast_to(pos_j, (ni, nj, nk))
    i_of = np.broadcast_to(np.arange(ni)[:, None, None], (ni, nj, nk))
    j_of = np.broadcast_to(np.arange(nj)[None, :, None], (ni, nj, nk))
    k_of = np.broadcast_to(np.arange(nk)[None, None, :], (ni, nj, nk))
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        ii, wi, nan_i = _axis_np(pos_i, i_of, relative, lo_i, ni, hi_i, method)
        jj, wj, nan_j = _axis_np(pos_j, j_of, relative, lo_j, nj, hi_j, method)
        if method == NEAREST:
            out = src[ii[0] + lo_i, jj[0] + lo_j, k_of].copy()  # the items themselves: bit patterns
            ut = {4: np.uint32, 8: np.uint64}[src.dtype.itemsize]
            out.view(ut)[nan_i | nan_j] = QNAN[src.dtype.itemsize]
            return out
        at = lambda c, r: src[c + lo_i, r + lo_j, k_of].astype(np.float64)  # noqa: E731
        rows = [_combine_np(wi, [at(c, r) for c in ii]) for r in jj]
        out = _combine_np(wj, rows)
        if method == CUBIC_MONOTONE:
            c00, c10, c01, c11 = at(ii[1], jj[1]), at(ii[2], jj[1]), at(ii[1], jj[2]), at(ii[2], jj[2])
            fmin_np = lambda a, b: np.where(b < a, b, a)  # noqa: E731
            fmax_np = lambda a, b: np.where(b > a, b, a)  # noqa: E731
            mn = fmin_np(fmin_np(c00, c10), fmin_np(c01, c11))
            mx = fmax_np(fmax_np(c00, c10), fmax_np(c01, c11))
            out = np.where(out < mn, mn, np.where(out > mx, mx, out))
        return out.astype(src.dtype)


def interp_plain(src: np.ndarray, pos_i: np.ndarray, pos_j: np.ndarray, method: str, relative: bool = False, reach=(0, 0, 0, 0)) -> np.ndarray:
    """What ``interp`` returns, from ``interp_point`` in a plain loop (slow: for small fields)."""
    lo_i, hi_i, lo_j, hi_j = reach
    ni, nj, nk = src.shape[0] - lo_i - hi_i, src.shape[1] - lo_j - hi_j, src.shape[2]
    out = np.empty((ni, nj, nk), dtype=src.dtype)
    ut = {4: np.uint32, 8: np.uint64}[src.dtype.itemsize]
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for i in range(ni):
            for j in range(nj):
                for k in range(nk):
                    pi = pos_i[i, j] if pos_i.ndim == 2 else pos_i[i, j, k]
                    pj = pos_j[i, j] if pos_j.ndim == 2 else pos_j[i, j, k]
                    v = interp_point(src[:, :, k], pi, pj, i, j, method, relative, reach)
                    if method == NEAREST:
                        out.view(ut)[i, j, k] = QNAN[src.dtype.itemsize] if v is None else v.view(ut)
                    else:
                        out[i, j, k] = np.float64(v).astype(src.dtype)
    return out


def stencil_touches(mask: np.ndarray, pos_i: np.ndarray, pos_j: np.ndarray, method: str, relative: bool = False, reach=(0, 0, 0, 0)) -> np.ndarray:
    """(ni, nj, nk) bool: the point reads at least one item of the readable box at which ``mask`` (bool, shaped like src) is set,
    whatever its weight -- a weight of zero still multiplies."""
    lo_i, hi_i, lo_j, hi_j = reach
    ni, nj, nk = mask.shape[0] - lo_i - hi_i, mask.shape[1] - lo_j - hi_j, mask.shape[2]
    shape = (ni, nj, nk)
    pos_i = np.broadcast_to(pos_i[:, :, None] if pos_i.ndim == 2 else pos_i, shape)
    pos_j = np.broadcast_to(pos_j[:, :, None] if pos_j.ndim == 2 else pos_j, shape)
    i_of, j_of, k_of = (np.broadcast_to(np.arange(n).reshape([-1 if ax == a else 1 for a in range(3)]), shape) for ax, n in enumerate(shape))
    ii, _, _ = _axis_np(pos_i, i_of, relative, lo_i, ni, hi_i, method)
    jj, _, _ = _axis_np(pos_j, j_of, relative, lo_j, nj, hi_j, method)
    out = np.zeros(shape, dtype=bool)
    for c in ii:
        for r in jj:
            out |= mask[c + lo_i, r + lo_j, k_of]
    return out


def same_bits(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """Elementwise: equal bit patterns, or both NaN (payloads are not compared)."""
    assert got.dtype == want.dtype and got.shape == want.shape
    ut = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return (np.ascontiguousarray(got).view(ut) == np.ascontiguousarray(want).view(ut)) | (np.isnan(got) & np.isnan(want))
