"""The arithmetic contract of ``gt4mi_departure_interp`` (include/gt4py_amd.h) restated twice: ``interp3_point`` in plain Python
floats -- IEEE float64, one rounding per operation --, one destination point at a time, and ``interp3`` with numpy float64 arrays,
the same operations in the same order elementwise (numpy fuses nothing), which is what the tests of whole fields use.
tests/test_departure_interp.py holds the two against each other bit for bit.  Test infrastructure; imports no product code and
(at import) no torch.  The per-axis steps, the weights and the combination are those of tests/horizontal_interp_ref.py.

float32 inputs are widened exactly (``float(...)`` / ``astype(float64)``); the caller rounds the result once (``numpy.astype``).

Geometry: ``src`` is the READABLE box of a field, the domain grown by ``reach = (lo_i, hi_i, lo_j, hi_j)`` along I and J, with all
``nk`` levels: domain point (0, 0, 0) is ``src[lo_i, lo_j, 0]``.  Positions are in index units of the domain (levels along K); in
relative mode they are displacements from the destination point's own index on all three axes."""

from __future__ import annotations

import numpy as np

from horizontal_interp_ref import (CUBIC, CUBIC_MONOTONE, LINEAR, METHODS, NEAREST, QNAN, _axis_np, _combine_np, axis, combine, cubic_weights,  # noqa: F401
                                   fmax, fmin, same_bits)


# ---- one point, plain Python ---------------------------------------------------------------------------------------------------
def plane_value(level, ii, wi, jj, wj, lo_i: int, lo_j: int) -> float:
    """P of one level (``level``: the readable box of that level, 2-d): the rows combined along I, the same expression along J."""
    rows = [combine(wi, [float(level[c + lo_i, r + lo_j]) for c in ii]) for r in jj]
    return combine(wj, rows)


def interp3_point(src: np.ndarray, pi: float, pj: float, pk: float, i: int, j: int, k: int, method: str, relative: bool, reach):
    """One point (``src``: the readable box, 3-d) as a Python float -- or, for ``nearest``, the source ITEM itself (None at a NaN
    position: the canonical quiet NaN is stored)."""
    lo_i, hi_i, lo_j, hi_j = reach
    ni, nj, nk = src.shape[0] - lo_i - hi_i, src.shape[1] - lo_j - hi_j, src.shape[2]
    ii, wi, nan_i = axis(float(pi), i, relative, lo_i, ni, hi_i, method)
    jj, wj, nan_j = axis(float(pj), j, relative, lo_j, nj, hi_j, method)
    if method == NEAREST:
        kk, _, nan_k = axis(float(pk), k, relative, 0, nk, 0, NEAREST)
        return None if nan_i or nan_j or nan_k else src[ii[0] + lo_i, jj[0] + lo_j, kk[0]]
    p = lambda level: plane_value(src[:, :, level], ii, wi, jj, wj, lo_i, lo_j)  # noqa: E731
    kl, wl, _ = axis(float(pk), k, relative, 0, nk, 0, LINEAR)  # b_k, b_k + 1 (each clamped); 1 - t_k, t_k
    if method == LINEAR:
        return wl[0] * p(kl[0]) + wl[1] * p(kl[1])
    b = kl[0]  # (x_k is clamped to [0, nk - 1]: clamping b_k again changes nothing)
    if 1 <= b <= nk - 3:
        kc, wc, _ = axis(float(pk), k, relative, 0, nk, 0, CUBIC)
        out = combine(wc, [p(level) for level in kc])
    else:
        out = wl[0] * p(kl[0]) + wl[1] * p(kl[1])
    if method == CUBIC_MONOTONE:
        c = {(a, b_, c_): float(src[ii[1 + a] + lo_i, jj[1 + b_] + lo_j, kl[c_]]) for a in (0, 1) for b_ in (0, 1) for c_ in (0, 1)}
        mn = fmin(fmin(fmin(c[0, 0, 0], c[1, 0, 0]), fmin(c[0, 1, 0], c[1, 1, 0])), fmin(fmin(c[0, 0, 1], c[1, 0, 1]), fmin(c[0, 1, 1], c[1, 1, 1])))
        mx = fmax(fmax(fmax(c[0, 0, 0], c[1, 0, 0]), fmax(c[0, 1, 0], c[1, 1, 0])), fmax(fmax(c[0, 0, 1], c[1, 0, 1]), fmax(c[0, 1, 1], c[1, 1, 1])))
        out = mn if out < mn else (mx if out > mx else out)
    return out


# ---- whole fields, numpy: the same operations elementwise ------------------------------------------------------------------------
def _broadcast_positions(pos_i, pos_j, pos_k, shape):
    assert pos_k.shape == shape, "pos_k is always IJK"
    pos_i = np.broadcast_to(pos_i[:, :, None] if pos_i.ndim == 2 else pos_i, shape)
    pos_j = np.broadcast_to(pos_j[:, :, None] if pos_j.ndim == 2 else pos_j, shape)
    return pos_i, pos_j, pos_k


def _index_fields(shape):
    return [np.broadcast_to(np.arange(n).reshape([-1 if ax == a else 1 for a in range(3)]), shape) for ax, n in enumerate(shape)]


def interp3(src: np.ndarray, pos_i: np.ndarray, pos_j: np.ndarray, pos_k: np.ndarray, method: str, relative: bool = False,
            reach=(0, 0, 0, 0)) -> np.ndarray:
    """``src`` (ni + lo_i + hi_i, nj + lo_j + hi_j, nk), the readable box -> the domain (ni, nj, nk) in the dtype of ``src``, rounded
    once.  ``pos_i`` / ``pos_j`` are (ni, nj) -- a Field[IJ] -- or (ni, nj, nk), ``pos_k`` is (ni, nj, nk); float32 or float64."""
    assert method in METHODS and src.ndim == 3
    lo_i, hi_i, lo_j, hi_j = reach
    shape = ni, nj, nk = src.shape[0] - lo_i - hi_i, src.shape[1] - lo_j - hi_j, src.shape[2]
    pos_i, pos_j, pos_k = _broadcast_positions(pos_i, pos_j, pos_k, shape)
    i_of, j_of, k_of = _index_fields(shape)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        ii, wi, nan_i = _axis_np(pos_i, i_of, relative, lo_i, ni, hi_i, method)
        jj, wj, nan_j = _axis_np(pos_j, j_of, relative, lo_j, nj, hi_j, method)
        if method == NEAREST:
            kk, _, nan_k = _axis_np(pos_k, k_of, relative, 0, nk, 0, NEAREST)
            out = src[ii[0] + lo_i, jj[0] + lo_j, kk[0]].copy()  # the items themselves: bit patterns
            ut = {4: np.uint32, 8: np.uint64}[src.dtype.itemsize]
            out.view(ut)[nan_i | nan_j | nan_k] = QNAN[src.dtype.itemsize]
            return out
        at = lambda c, r, level: src[c + lo_i, r + lo_j, level].astype(np.float64)  # noqa: E731
        p = lambda level: _combine_np(wj, [_combine_np(wi, [at(c, r, level) for c in ii]) for r in jj])  # noqa: E731
        kl, wl, _ = _axis_np(pos_k, k_of, relative, 0, nk, 0, LINEAR)
        out = wl[0] * p(kl[0]) + wl[1] * p(kl[1])
        if method != LINEAR:
            kc, wc, _ = _axis_np(pos_k, k_of, relative, 0, nk, 0, CUBIC)
            full = (kl[0] >= 1) & (kl[0] <= nk - 3)
            out = np.where(full, _combine_np(wc, [p(level) for level in kc]), out)  # (clamped levels: every load is valid)
        if method == CUBIC_MONOTONE:
            fmin_np = lambda a, b: np.where(b < a, b, a)  # noqa: E731
            fmax_np = lambda a, b: np.where(b > a, b, a)  # noqa: E731
            c = {(a, b, d): at(ii[1 + a], jj[1 + b], kl[d]) for a in (0, 1) for b in (0, 1) for d in (0, 1)}
            fold = lambda f: f(f(f(c[0, 0, 0], c[1, 0, 0]), f(c[0, 1, 0], c[1, 1, 0])), f(f(c[0, 0, 1], c[1, 0, 1]), f(c[0, 1, 1], c[1, 1, 1])))  # noqa: E731
            mn, mx = fold(fmin_np), fold(fmax_np)
            out = np.where(out < mn, mn, np.where(out > mx, mx, out))
        return out.astype(src.dtype)


def interp3_plain(src: np.ndarray, pos_i: np.ndarray, pos_j: np.ndarray, pos_k: np.ndarray, method: str, relative: bool = False,
                  reach=(0, 0, 0, 0)) -> np.ndarray:
    """What ``interp3`` returns, from ``interp3_point`` in a plain loop (slow: for small fields)."""
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
                    v = interp3_point(src, pi, pj, pos_k[i, j, k], i, j, k, method, relative, reach)
                    if method == NEAREST:
                        out.view(ut)[i, j, k] = QNAN[src.dtype.itemsize] if v is None else v.view(ut)
                    else:
                        out[i, j, k] = np.float64(v).astype(src.dtype)
    return out


def stencil_touches(mask: np.ndarray, pos_i: np.ndarray, pos_j: np.ndarray, pos_k: np.ndarray, method: str, relative: bool = False,
                    reach=(0, 0, 0, 0)) -> np.ndarray:
    """(ni, nj, nk) bool: the point reads at least one item of the readable box at which ``mask`` (bool, shaped like src) is set,
    whatever its weight -- a weight of zero still multiplies.  Along K a cubic reads four levels where 1 <= b_k <= nk - 3 and the
    two levels b_k, b_k + 1 otherwise."""
    lo_i, hi_i, lo_j, hi_j = reach
    shape = ni, nj, nk = mask.shape[0] - lo_i - hi_i, mask.shape[1] - lo_j - hi_j, mask.shape[2]
    pos_i, pos_j, pos_k = _broadcast_positions(pos_i, pos_j, pos_k, shape)
    i_of, j_of, k_of = _index_fields(shape)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        ii, _, _ = _axis_np(pos_i, i_of, relative, lo_i, ni, hi_i, method)
        jj, _, _ = _axis_np(pos_j, j_of, relative, lo_j, nj, hi_j, method)
        if method == NEAREST:
            levels = [(_axis_np(pos_k, k_of, relative, 0, nk, 0, NEAREST)[0][0], True)]
        else:
            kl, _, _ = _axis_np(pos_k, k_of, relative, 0, nk, 0, LINEAR)
            levels = [(kl[0], True), (kl[1], True)]
            if method != LINEAR:
                kc, _, _ = _axis_np(pos_k, k_of, relative, 0, nk, 0, CUBIC)
                full = (kl[0] >= 1) & (kl[0] <= nk - 3)
                levels += [(kc[0], full), (kc[3], full)]
    out = np.zeros(shape, dtype=bool)
    for level, read in levels:
        for c in ii:
            for r in jj:
                out |= mask[c + lo_i, r + lo_j, level] & read
    return out
