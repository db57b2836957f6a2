"""The arithmetic contract of ``gt4mi_vertical_interp`` (include/gt4py_amd.h) restated twice: ``interp_column`` in plain Python
floats -- IEEE float64, one rounding per operation --, one column at a time, the bracket index carried from target to target as
the contract says; and ``interp`` with numpy float64 arrays, the same operations in the same order elementwise (numpy fuses
nothing), the hunt as masked steps, which is what the tests of whole fields use.  tests/test_vertical_interp.py holds the two
against each other bit for bit.  Test infrastructure; imports no product code and (at import) no torch.

float32 inputs are widened exactly (``float(...)`` / ``astype(float64)``); the result is rounded once (``numpy.astype``)."""

from __future__ import annotations

import math

import numpy as np

NEAREST, LINEAR, CUBIC, CUBIC_MONOTONE = "nearest", "linear", "cubic", "cubic_monotone"
METHODS = (NEAREST, LINEAR, CUBIC, CUBIC_MONOTONE)
CLAMP, EXTEND, FILL = "clamp", "linear", "fill"
OUTSIDE = (CLAMP, EXTEND, FILL)
NAN, INF = float("nan"), float("inf")
QNAN = {4: 0x7FC0_0000, 8: 0x7FF8_0000_0000_0000}  # what a NaN fill_value and nearest at a NaN target store
UINT = {4: np.uint32, 8: np.uint64}


def div(a: float, b: float) -> float:
    """One IEEE division (Python raises where IEEE returns an infinity or a NaN)."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)


# ---- one column, plain Python ----------------------------------------------------------------------------------------------------
def hunt(z, x: float, k: int) -> int:
    """Step 1: the only two places where the bracket index changes."""
    ns = len(z)
    while k < ns - 2 and z[k + 1] <= x:
        k += 1
    while k > 0 and z[k] > x:
        k -= 1
    return k


def lagrange_weights(x: float, z0: float, z1: float, z2: float, z3: float):
    """w_a = (product of (x - z_b), b != a, left to right) / (product of (z_a - z_b), b != a, left to right)."""
    x0, x1, x2, x3 = x - z0, x - z1, x - z2, x - z3
    return [div((x1 * x2) * x3, ((z0 - z1) * (z0 - z2)) * (z0 - z3)),
            div((x0 * x2) * x3, ((z1 - z0) * (z1 - z2)) * (z1 - z3)),
            div((x0 * x1) * x3, ((z2 - z0) * (z2 - z1)) * (z2 - z3)),
            div((x0 * x1) * x2, ((z3 - z0) * (z3 - z1)) * (z3 - z2))]


def plan_target(z, x: float, k: int, method: str, outside: str):
    """Steps 1 to 3 up to the weights, for all fields of a call: (the carried k, what to do).  What to do is ("fill",), ("nan",),
    ("item", index), ("linear", k, t) or ("cubic", k, weights)."""
    ns = len(z)
    k = hunt(z, x, k)
    below, above = x < z[0], x > z[ns - 1]
    extend = False
    if below or above:
        if outside == FILL:
            return k, ("fill",)
        if outside == CLAMP:
            x = z[0] if below else z[ns - 1]
        else:
            extend = True
    t = div(x - z[k], z[k + 1] - z[k])
    if method == NEAREST:
        if extend:
            return k, ("item", 0 if below else ns - 1)
        if x != x:
            return k, ("nan",)
        return k, ("item", k + 1 if t >= 0.5 else k)
    if method == LINEAR or extend or k < 1 or k > ns - 3:
        return k, ("linear", k, t)
    return k, ("cubic", k, lagrange_weights(x, z[k - 1], z[k], z[k + 1], z[k + 2]))


def apply_plan(plan, q, method: str):
    """One field's value for a plan: a Python float, or for the bit-moving cases ("fill",) / ("nan",) / ("item", index) as they are."""
    if plan[0] in ("fill", "nan", "item"):
        return plan
    if plan[0] == "linear":
        _, k, t = plan
        return (1.0 - t) * q[k] + t * q[k + 1]
    _, k, w = plan
    out = ((w[0] * q[k - 1] + w[1] * q[k]) + w[2] * q[k + 1]) + w[3] * q[k + 2]
    if method == CUBIC_MONOTONE:
        a, b = q[k], q[k + 1]
        mn = b if b < a else a
        mx = b if b > a else a
        out = mn if out < mn else (mx if out > mx else out)
    return out


def interp_column(z, x, q, method: str, outside: str, k: int = 0):
    """(results, brackets) of one column of one field: ``z``, ``x``, ``q`` are sequences of Python floats, ``k`` where the bracket
    index starts (the contract: 0).  A result is a Python float, ("fill",), ("nan",) or ("item", index of the source item that is
    moved)."""
    assert len(z) == len(q) >= 2 and method in METHODS and outside in OUTSIDE
    out, ks = [], []
    for xm in x:
        k, plan = plan_target(z, xm, k, method, outside)
        ks.append(k)
        out.append(apply_plan(plan, q, method))
    return out, ks


def fill_item(fill_value: float, dtype) -> np.ndarray:
    """``fill_value`` as an item of ``dtype``: rounded once; NaN is the canonical quiet NaN."""
    dtype = np.dtype(dtype)
    item = np.empty((), dtype=dtype)
    if fill_value != fill_value:
        item.view(UINT[dtype.itemsize])[...] = QNAN[dtype.itemsize]
    else:
        with np.errstate(over="ignore", under="ignore"):
            item[...] = np.float64(fill_value).astype(dtype)
    return item


def _column(c: np.ndarray, i: int, j: int):
    return [float(v) for v in (c if c.ndim == 1 else c[i, j])]


def interp_plain(q: np.ndarray, z: np.ndarray, x: np.ndarray, method: str, outside: str = CLAMP, fill_value: float = NAN) -> np.ndarray:
    """What ``interp`` returns, from ``interp_column`` in a plain loop (slow: for small fields)."""
    ni, nj, _ = q.shape
    nd = x.shape[-1]
    out = np.empty((ni, nj, nd), dtype=q.dtype)
    ut = UINT[q.dtype.itemsize]
    fill = fill_item(fill_value, q.dtype)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for i in range(ni):
            for j in range(nj):
                col, _ = interp_column(_column(z, i, j), _column(x, i, j), [float(v) for v in q[i, j]], method, outside)
                for m, v in enumerate(col):
                    if not isinstance(v, tuple):
                        out[i, j, m] = np.float64(v).astype(q.dtype)
                    elif v[0] == "fill":
                        out[i, j, m] = fill
                    elif v[0] == "nan":
                        out.view(ut)[i, j, m] = QNAN[q.dtype.itemsize]
                    else:
                        out[i, j, m] = q[i, j, v[1]]  # the item itself
    return out


# ---- whole fields, numpy: the same operations elementwise ------------------------------------------------------------------------
def interp(q: np.ndarray, z: np.ndarray, x: np.ndarray, method: str, outside: str = CLAMP, fill_value: float = NAN) -> np.ndarray:
    """``q`` (ni, nj, ns) -> (ni, nj, nd) in the dtype of ``q``, rounded once; ``z`` is (ni, nj, ns) or one column (ns,) for all,
    ``x`` (ni, nj, nd) or (nd,), float32 or float64."""
    assert method in METHODS and outside in OUTSIDE and q.ndim == 3
    ni, nj, ns = q.shape
    nd = x.shape[-1]
    assert ns >= 2 and z.shape[-1] == ns
    z = np.broadcast_to(z.astype(np.float64), (ni, nj, ns))
    x_all = np.broadcast_to(x.astype(np.float64), (ni, nj, nd))
    ii, jj = np.meshgrid(np.arange(ni), np.arange(nj), indexing="ij")
    at = lambda a, kk: a[ii, jj, kk]  # noqa: E731
    out = np.empty((ni, nj, nd), dtype=q.dtype)
    ut = UINT[q.dtype.itemsize]
    fill = fill_item(fill_value, q.dtype)
    k = np.zeros((ni, nj), dtype=np.int64)
    z_first, z_last = z[..., 0], z[..., ns - 1]
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        for m in range(nd):
            xm = x_all[..., m]
            while True:  # (at most ns - 2 rounds: k only grows, below ns - 2)
                go = (k < ns - 2) & (at(z, np.minimum(k + 1, ns - 1)) <= xm)
                if not go.any():
                    break
                k = k + go
            while True:
                go = (k > 0) & (at(z, k) > xm)
                if not go.any():
                    break
                k = k - go
            below, above = xm < z_first, xm > z_last
            outer = below | above
            if outside == CLAMP:
                xm = np.where(below, z_first, np.where(above, z_last, xm))
            extend = outer & (outside == EXTEND)
            zk, zk1 = at(z, k), at(z, k + 1)
            t = (xm - zk) / (zk1 - zk)
            if method == NEAREST:
                kk = np.where(extend, np.where(below, 0, ns - 1), np.where(t >= 0.5, k + 1, k))
                res = at(q, kk).copy()  # the items themselves: bit patterns
                res.view(ut)[xm != xm] = QNAN[q.dtype.itemsize]
            else:
                q1, q2 = at(q, k).astype(np.float64), at(q, k + 1).astype(np.float64)
                val = (1.0 - t) * q1 + t * q2
                if method != LINEAR:
                    cubic = ~extend & (k >= 1) & (k <= ns - 3)
                    km, kp = np.maximum(k - 1, 0), np.minimum(k + 2, ns - 1)  # (where not cubic: computed, not used)
                    z0, z3 = at(z, km), at(z, kp)
                    q0, q3 = at(q, km).astype(np.float64), at(q, kp).astype(np.float64)
                    x0, x1, x2, x3 = xm - z0, xm - zk, xm - zk1, xm - z3
                    w0 = ((x1 * x2) * x3) / (((z0 - zk) * (z0 - zk1)) * (z0 - z3))
                    w1 = ((x0 * x2) * x3) / (((zk - z0) * (zk - zk1)) * (zk - z3))
                    w2 = ((x0 * x1) * x3) / (((zk1 - z0) * (zk1 - zk)) * (zk1 - z3))
                    w3 = ((x0 * x1) * x2) / (((z3 - z0) * (z3 - zk)) * (z3 - zk1))
                    c = ((w0 * q0 + w1 * q1) + w2 * q2) + w3 * q3
                    if method == CUBIC_MONOTONE:
                        mn, mx = np.where(q2 < q1, q2, q1), np.where(q2 > q1, q2, q1)
                        c = np.where(c < mn, mn, np.where(c > mx, mx, c))
                    val = np.where(cubic, c, val)
                res = val.astype(q.dtype)
            if outside == FILL:
                res[outer] = fill
            out[..., m] = res
    return out


def same_bits(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """Elementwise: equal bit patterns, or both NaN (payloads are not compared)."""
    assert got.dtype == want.dtype and got.shape == want.shape
    ut = UINT[got.dtype.itemsize]
    return (np.ascontiguousarray(got).view(ut) == np.ascontiguousarray(want).view(ut)) | (np.isnan(got) & np.isnan(want))
