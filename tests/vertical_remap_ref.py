"""The arithmetic contract of ``gt4mi_vertical_remap`` (include/gt4py_amd.h) restated in plain Python floats -- IEEE float64, one
rounding per operation --, in a plain loop per column.  Test infrastructure; imports no product code and (at import) no torch.

float32 inputs are widened exactly by ``float(...)``; the caller rounds the result once (``numpy.astype``)."""

from __future__ import annotations

import math

import numpy as np

PCM, PLM = "pcm", "plm"
NAN, INF = float("nan"), float("inf")


def div(a: float, b: float) -> float:
    """One IEEE division (Python raises where IEEE returns an infinity or a NaN)."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)


def slopes(zs, q):
    """``s[k]`` of the piecewise linear method: limited, 0 in the two end cells and at extrema."""
    ns = len(q)
    s = [0.0] * ns
    for k in range(1, ns - 1):
        dl, dr = q[k] - q[k - 1], q[k + 1] - q[k]
        if dl * dr > 0.0:
            hm, hc, hp = zs[k] - zs[k - 1], zs[k + 1] - zs[k], zs[k + 2] - zs[k + 1]
            g = div(q[k + 1] - q[k - 1], 0.5 * hm + hc + 0.5 * hp) * hc
            a = abs(g)
            b, c = 2.0 * abs(dl), 2.0 * abs(dr)
            if b < a:
                a = b
            if c < a:
                a = c
            s[k] = math.copysign(a, g)
    return s


def remap_column(zs, zd, q, method: str):
    """(target means, number of terms) of one column; ``zs``, ``zd``, ``q`` are sequences of Python floats."""
    ns, nd = len(q), len(zd) - 1
    assert len(zs) == ns + 1 and ns >= 1 and nd >= 1 and method in (PCM, PLM)
    s = slopes(zs, q) if method == PLM else None
    out, terms, k = [], 0, 0
    for m in range(nd):
        lo, hi = zd[m], zd[m + 1]
        d = hi - lo
        while k < ns - 1 and not (zs[k + 1] > lo):
            k += 1
        acc, first = 0.0, True
        while True:
            l = lo if k == 0 else (zs[k] if zs[k] > lo else lo)  # noqa: E741
            r = hi if k == ns - 1 else (zs[k + 1] if zs[k + 1] < hi else hi)
            w = div(r - l, d)
            if method == PLM:
                h = zs[k + 1] - zs[k]
                xl, xr = div(l - zs[k], h), div(r - zs[k], h)
                v = q[k] + s[k] * (0.5 * (xl + xr) - 0.5)
            else:
                v = q[k]
            t = w * v
            acc = t if first else acc + t
            first = False
            terms += 1
            if k == ns - 1 or zs[k + 1] >= hi:
                break
            k += 1
        out.append(acc)
    return out, terms


def _column(edges: np.ndarray, i: int, j: int):
    return [float(x) for x in (edges if edges.ndim == 1 else edges[i, j])]


def remap(q: np.ndarray, zs: np.ndarray, zd: np.ndarray, method: str) -> np.ndarray:
    """``q`` (ni, nj, ns) -> float64 (ni, nj, nd); ``zs`` / ``zd`` are (ni, nj, n + 1) or one column (n + 1,) for all."""
    ni, nj, _ = q.shape
    nd = zd.shape[-1] - 1
    out = np.empty((ni, nj, nd), dtype=np.float64)
    for i in range(ni):
        for j in range(nj):
            out[i, j], _ = remap_column(_column(zs, i, j), _column(zd, i, j), [float(x) for x in q[i, j]], method)
    return out


def remap_as(q: np.ndarray, zs: np.ndarray, zd: np.ndarray, method: str) -> np.ndarray:
    """The result in the dtype of ``q``: rounded once."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return remap(q, zs, zd, method).astype(q.dtype)


def same_bits(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """Elementwise: equal bit patterns, or both NaN (payloads are not compared)."""
    assert got.dtype == want.dtype and got.shape == want.shape
    ut = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    return (np.ascontiguousarray(got).view(ut) == np.ascontiguousarray(want).view(ut)) | (np.isnan(got) & np.isnan(want))
