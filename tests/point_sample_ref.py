"""The contract of ``gt4mi_point_sample`` (include/gt4py_amd.h) restated twice.  ``sample_plain`` goes point by point through
``horizontal_interp_ref.interp_point`` (column mode) and ``departure_interp_ref.interp3_point`` (point mode) with ``relative=False``
and adds what the entry adds: the fill rule and the one rounding to the item type.  ``sample`` is the whole-array form the GPU tests
use: in absolute mode a value depends on the position items alone, not on which point of a domain asks for it, so the list of points
is laid out, chunk by chunk, as the position FIELDS of ``horizontal_interp_ref.interp`` / ``departure_interp_ref.interp3`` -- no
arithmetic is written down a third time.  tests/test_point_sample.py holds the two against each other bit for bit.  Test
infrastructure; imports no product code and (at import) no torch.

Geometry: ``src`` is the READABLE box of a field, the domain grown by ``reach = (lo_i, hi_i, lo_j, hi_j)`` along I and J, all ``nk``
levels; positions are in index units of the domain.  Column mode (``pos_k is None``) returns ``(npoints, nk)``, point mode
``(npoints,)``, in the dtype of ``src``."""

from __future__ import annotations

import numpy as np

import departure_interp_ref as D
import horizontal_interp_ref as H
from horizontal_interp_ref import METHODS, NEAREST, QNAN, same_bits  # noqa: F401

UINT = {4: np.uint32, 8: np.uint64}


def fill_item(fill_value: float, dtype) -> np.ndarray:
    """``fill_value`` (a double) rounded ONCE to the item type."""
    with np.errstate(over="ignore"):
        return np.float64(fill_value).astype(dtype)


def bounds(src_shape, reach, point_mode: bool):
    """(xmin, xmax) per position array, as floats: the readable box along I and J, the levels along K."""
    lo_i, hi_i, lo_j, hi_j = reach
    ni, nj, nk = src_shape[0] - lo_i - hi_i, src_shape[1] - lo_j - hi_j, src_shape[2]
    out = [(float(-lo_i), float(ni - 1 + hi_i)), (float(-lo_j), float(nj - 1 + hi_j))]
    return out + [(0.0, float(nk - 1))] if point_mode else out


def is_filled(items, limits) -> bool:
    """The fill rule for one point: any of its position items satisfies p < xmin, p > xmax or p != p."""
    return any(float(p) < xmin or float(p) > xmax or float(p) != float(p) for p, (xmin, xmax) in zip(items, limits))


def _store(out_flat_bits, at, v, dtype):
    """One result item: the source item itself or the canonical quiet NaN for nearest (``v`` an item or None), else rounded once."""
    if v is None:
        out_flat_bits[at] = QNAN[np.dtype(dtype).itemsize]
    elif isinstance(v, np.generic) and v.dtype == dtype:
        out_flat_bits[at] = v.view(UINT[v.itemsize])
    else:
        with np.errstate(over="ignore", invalid="ignore"):
            out_flat_bits[at] = np.float64(v).astype(dtype).view(UINT[np.dtype(dtype).itemsize])


def sample_plain(src: np.ndarray, pos_i, pos_j, pos_k=None, method: str = "linear", reach=(0, 0, 0, 0), outside: str = "clamp",
                 fill_value: float = float("nan")) -> np.ndarray:
    """Point by point, in plain Python (slow: for small lists)."""
    assert method in METHODS and outside in ("clamp", "fill") and src.ndim == 3
    point_mode = pos_k is not None
    npoints, nk = len(pos_i), src.shape[2]
    limits = bounds(src.shape, reach, point_mode)
    out = np.empty((npoints,) if point_mode else (npoints, nk), dtype=src.dtype)
    bits = out.view(UINT[src.dtype.itemsize])
    fill_bits = fill_item(fill_value, src.dtype).view(UINT[src.dtype.itemsize])
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for p in range(npoints):
            items = (pos_i[p], pos_j[p]) + ((pos_k[p],) if point_mode else ())
            if outside == "fill" and is_filled(items, limits):
                bits[p] = fill_bits  # every level
            elif point_mode:
                _store(bits, p, D.interp3_point(src, pos_i[p], pos_j[p], pos_k[p], 0, 0, 0, method, False, reach), src.dtype)
            else:
                for k in range(nk):
                    _store(bits, (p, k), H.interp_point(src[:, :, k], pos_i[p], pos_j[p], 0, 0, method, False, reach), src.dtype)
    return out


def sample(src: np.ndarray, pos_i, pos_j, pos_k=None, method: str = "linear", reach=(0, 0, 0, 0), outside: str = "clamp",
           fill_value: float = float("nan")) -> np.ndarray:
    """The whole list at once, through the numpy forms of the two interpolators' restatements."""
    assert method in METHODS and outside in ("clamp", "fill") and src.ndim == 3
    point_mode = pos_k is not None
    lo_i, hi_i, lo_j, hi_j = reach
    ni, nj, nk = src.shape[0] - lo_i - hi_i, src.shape[1] - lo_j - hi_j, src.shape[2]
    positions = [np.asarray(p) for p in ((pos_i, pos_j, pos_k) if point_mode else (pos_i, pos_j))]
    npoints = positions[0].shape[0]
    assert all(p.shape == (npoints,) for p in positions)
    # a chunk of the list as position fields over the domain: (ni, nj) of them in column mode, (ni, nj, nk) in point mode
    grid = (ni, nj, nk) if point_mode else (ni, nj)
    per_chunk = int(np.prod(grid))
    chunks = -(-npoints // per_chunk)
    padded = [np.concatenate([p, np.zeros(chunks * per_chunk - npoints, dtype=p.dtype)]) for p in positions]
    parts = []
    for c in range(chunks):
        fields = [p[c * per_chunk:(c + 1) * per_chunk].reshape(grid) for p in padded]
        if point_mode:
            parts.append(D.interp3(src, *fields, method, False, reach).reshape(per_chunk))
        else:
            parts.append(H.interp(src, *fields, method, False, reach).reshape(per_chunk, nk))
    out = np.concatenate(parts)[:npoints] if parts else np.empty((0,) if point_mode else (0, nk), dtype=src.dtype)
    if outside == "fill":
        filled = np.zeros(npoints, dtype=bool)
        for p, (xmin, xmax) in zip(positions, bounds(src.shape, reach, point_mode)):
            x = p.astype(np.float64)
            filled |= (x < xmin) | (x > xmax) | (x != x)
        out = out.copy()
        out[filled] = fill_item(fill_value, src.dtype)
    return np.ascontiguousarray(out)
