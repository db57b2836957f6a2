"""The contract of ``gt4mi_overlap_table`` and ``gt4mi_horizontal_remap`` (include/gt4py_amd.h) restated in plain Python floats --
IEEE float64, one rounding per operation --, one function for the table of an axis and one for a field.  Test infrastructure;
imports no product code and (at import) no torch.

float32 inputs are widened exactly by ``float(...)``; the caller rounds the result once (``numpy.astype``)."""

from __future__ import annotations

import numpy as np

from vertical_remap_ref import div, same_bits, slopes  # noqa: F401  (same_bits: for the tests)

PCM, PLM = "pcm", "plm"


def axis_table(xs, xd):
    """``(ptr, cell, w, h, c, den)`` of one axis as Python lists; ``xs`` / ``xd``: ns + 1 / nd + 1 Python floats, finite and strictly
    increasing.  The loop is ``vertical_remap_ref.remap_column``'s."""
    ns, nd = len(xs) - 1, len(xd) - 1
    assert ns >= 1 and nd >= 1
    ptr, cell, w, h, c, den = [], [], [], [], [], []
    k = 0
    for m in range(nd):
        lo, hi = xd[m], xd[m + 1]
        d = hi - lo
        ptr.append(len(cell))
        while k < ns - 1 and not (xs[k + 1] > lo):
            k += 1
        while True:
            l = lo if k == 0 else (xs[k] if xs[k] > lo else lo)  # noqa: E741
            r = hi if k == ns - 1 else (xs[k + 1] if xs[k + 1] < hi else hi)
            hk = xs[k + 1] - xs[k]
            xl, xr = div(l - xs[k], hk), div(r - xs[k], hk)
            cell.append(k)
            w.append(div(r - l, d))
            h.append(hk)
            c.append(0.5 * (xl + xr) - 0.5)
            den.append(1.0 if k == 0 or k == ns - 1 else 0.5 * (xs[k] - xs[k - 1]) + hk + 0.5 * (xs[k + 2] - xs[k + 1]))
            if k == ns - 1 or xs[k + 1] >= hi:
                break
            k += 1
    ptr.append(len(cell))
    return ptr, cell, w, h, c, den


def _floats(x):
    return [float(v) for v in x]


def remap_level(q, xs_i, xs_j, table_i, table_j, method: str):
    """One level: ``q`` is a list (over I) of lists (over J) of Python floats; returns the destination level in the same form."""
    ns_i, ns_j = len(q), len(q[0])
    ptr_i, cell_i, w_i, _, c_i, _ = table_i
    ptr_j, cell_j, w_j, _, c_j, _ = table_j
    if method == PLM:  # the limited slopes of every source cell along I and along J: 0 in the end cells of the axis and at extrema
        s_i = [slopes(xs_i, [q[a][b] for a in range(ns_i)]) for b in range(ns_j)]  # [b][a]
        s_j = [slopes(xs_j, q[a]) for a in range(ns_i)]  # [a][b]
    out = []
    for m_i in range(len(ptr_i) - 1):
        row_out = []
        for m_j in range(len(ptr_j) - 1):
            acc = 0.0
            for tb in range(ptr_j[m_j], ptr_j[m_j + 1]):
                b = cell_j[tb]
                row = 0.0
                for ta in range(ptr_i[m_i], ptr_i[m_i + 1]):
                    a = cell_i[ta]
                    v = q[a][b]
                    if method == PLM:
                        v = (v + s_i[b][a] * c_i[ta]) + s_j[a][b] * c_j[tb]
                    t = w_i[ta] * v
                    row = t if ta == ptr_i[m_i] else row + t
                t = w_j[tb] * row
                acc = t if tb == ptr_j[m_j] else acc + t
            row_out.append(acc)
        out.append(row_out)
    return out


def remap(q: np.ndarray, src_edges, dst_edges, method: str) -> np.ndarray:
    """``q`` (ns_i, ns_j, nk) -> float64 (nd_i, nd_j, nk); ``src_edges`` / ``dst_edges`` are pairs (along I, along J) of 1-d arrays."""
    assert method in (PCM, PLM)
    xs_i, xs_j = (_floats(e) for e in src_edges)
    xd_i, xd_j = (_floats(e) for e in dst_edges)
    assert q.shape[:2] == (len(xs_i) - 1, len(xs_j) - 1)
    table_i, table_j = axis_table(xs_i, xd_i), axis_table(xs_j, xd_j)
    out = np.empty((len(xd_i) - 1, len(xd_j) - 1, q.shape[2]), dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(q.shape[2]):
            level = [[float(x) for x in column] for column in q[:, :, k]]
            out[:, :, k] = remap_level(level, xs_i, xs_j, table_i, table_j, method)
    return out


def remap_as(q: np.ndarray, src_edges, dst_edges, method: str) -> np.ndarray:
    """The result in the dtype of ``q``: rounded once."""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return remap(q, src_edges, dst_edges, method).astype(q.dtype)
