"""``gt4py_amd.vertical.interpolate_levels`` without a GPU: the two restatements of the arithmetic contract
(tests/vertical_interp_ref.py) against each other bit for bit, path independence, known answers, every refusal of the C entry
through the dry run (made-up addresses that are never dereferenced), the declaration, the kernels' resources and the Python
interface's argument checks."""

import math

import numpy as np
import pytest

import entry_checks as E
import vertical_interp_ref as V
from entry_checks import INV, OOB, UNS, as_arg, int64s
from gt4py_amd import _lib, vertical

HOST = (8, 9, 5)  # the shape of a host field where a test states none
EPS = float(np.finfo(np.float64).eps)
LEVELS = [2, 3, 4, 5, 6, 17]
KINDS = ["inside", "reversed", "shuffled", "on_levels", "outside_both_ends", "nan"]


# ---- columns -----------------------------------------------------------------------------------------------------------------------
def _coords(rng, shape_ij, ns, cdtype):
    """Strictly increasing source coordinates that hold values of ``cdtype``, as float64."""
    z = rng.uniform(-2, 2, shape_ij + (1,)) + np.cumsum(rng.uniform(0.05, 1.0, shape_ij + (ns,)), axis=2)
    z = z.astype(cdtype).astype(np.float64)
    assert (np.diff(z, axis=2) > 0).all()
    return z


def _targets(kind, rng, z, nd, cdtype):
    lo, hi = z[..., :1], z[..., -1:]
    inside = lo + (hi - lo) * rng.uniform(0, 1, z.shape[:2] + (nd,))
    if kind == "inside":
        x = inside
    elif kind == "reversed":
        x = np.sort(inside, axis=2)[..., ::-1]
    elif kind == "shuffled":
        x = rng.permuted(np.sort(inside, axis=2), axis=2)
    elif kind == "on_levels":  # every target IS a source level: the <= and > ties, t == 0 (and t == 1 at the last one)
        x = np.take_along_axis(z, rng.integers(0, z.shape[2], z.shape[:2] + (nd,)), axis=2)
    elif kind == "outside_both_ends":
        x = inside.copy()
        x[..., 0::3] = lo - rng.uniform(0.01, 3, x[..., 0::3].shape)
        x[..., 1::3] = hi + rng.uniform(0.01, 3, x[..., 1::3].shape)
    elif kind == "nan":
        x = inside.copy()
        x[..., nd // 2] = np.nan
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x).astype(cdtype).astype(np.float64)


def _values(rng, shape, fdtype):
    return (280.0 + rng.uniform(-40, 40, shape)).astype(fdtype)


# ---- the two restatements ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cdtype", [np.float32, np.float64])
@pytest.mark.parametrize("fdtype", [np.float32, np.float64])
@pytest.mark.parametrize("method", V.METHODS)
def test_the_two_restatements_agree_bit_for_bit(method, fdtype, cdtype):
    rng = np.random.default_rng([1, V.METHODS.index(method), np.dtype(fdtype).itemsize, np.dtype(cdtype).itemsize])
    shape_ij = (3, 2)
    for ns in LEVELS:
        z = _coords(rng, shape_ij, ns, cdtype)
        q = _values(rng, shape_ij + (ns,), fdtype)
        for kind in KINDS:
            x = _targets(kind, rng, z, 7, cdtype)
            for outside in V.OUTSIDE:
                for fill in ((V.NAN, -999.25) if outside == V.FILL else (V.NAN,)):
                    a = V.interp(q, z.astype(cdtype), x.astype(cdtype), method, outside, fill)
                    b = V.interp_plain(q, z.astype(cdtype), x.astype(cdtype), method, outside, fill)
                    assert a.dtype == b.dtype == np.dtype(fdtype)
                    assert V.same_bits(a, b).all(), (method, ns, kind, outside)
                    if kind == "outside_both_ends" and outside == V.FILL:
                        outer = (x < z[..., :1]) | (x > z[..., -1:])
                        assert outer.any() and V.same_bits(a[outer], np.broadcast_to(V.fill_item(fill, fdtype), a[outer].shape).copy()).all()
                        if fill != fill:
                            assert (a.view(V.UINT[a.itemsize])[outer] == V.QNAN[a.itemsize]).all()
    # a shared Field[K] on either side is the same column everywhere
    z1, x1 = z[0, 0].astype(cdtype), x[1, 1].astype(cdtype)
    a = V.interp(q, z1, x1, method, V.EXTEND)
    assert V.same_bits(a, V.interp(q, np.broadcast_to(z1, q.shape), np.broadcast_to(x1, shape_ij + x1.shape), method, V.EXTEND)).all()
    assert V.same_bits(a, V.interp_plain(q, z1, x1, method, V.EXTEND)).all()


def test_nearest_moves_bit_patterns_and_a_nan_target_stores_the_canonical_nan():
    z = [0.0, 1.0, 2.0, 4.0]
    payload = np.array([0x7FA0_BEEF], dtype=np.uint32).view(np.float32)[0]
    q = np.array([[[1.0, payload, -0.0, 3.0]]], dtype=np.float32)
    x = np.array([0.9, 1.5, 2.99, 3.0, V.NAN, -5.0, 9.0])
    for outside, ends in ((V.CLAMP, (0, 3)), (V.EXTEND, (0, 3))):
        out = V.interp(q, np.array(z), x, V.NEAREST, outside)
        want_index = [1, 2, 2, 3, None, ends[0], ends[1]]  # t == 0.5 goes up
        bits = out.view(np.uint32)[0, 0]
        for m, kk in enumerate(want_index):
            assert bits[m] == (V.QNAN[4] if kk is None else q.view(np.uint32)[0, 0, kk]), (outside, m)
    col, ks = V.interp_column(z, [float(v) for v in x], [1.0, 2.0, 3.0, 4.0], V.NEAREST, V.FILL)
    assert col == [("item", 1), ("item", 2), ("item", 2), ("item", 3), ("nan",), ("fill",), ("fill",)] and ks == [0, 1, 2, 2, 2, 0, 2]


# ---- path independence ---------------------------------------------------------------------------------------------------------
def test_permuting_the_targets_permutes_the_results_and_changes_no_bit():
    rng = np.random.default_rng(2)
    for ns in LEVELS:
        z = _coords(rng, (2, 3), ns, np.float64)
        q = _values(rng, (2, 3, ns), np.float64)
        x = np.concatenate([_targets("outside_both_ends", rng, z, 6, np.float64), _targets("on_levels", rng, z, 5, np.float64)], axis=2)
        perm = rng.permutation(x.shape[2])
        for method in V.METHODS:
            for outside in V.OUTSIDE:
                a = V.interp(q, z, x, method, outside, -1.0)
                b = V.interp(q, z, np.ascontiguousarray(x[..., perm]), method, outside, -1.0)
                assert V.same_bits(a[..., perm], b).all(), (method, outside, ns)


def test_the_hunt_lands_on_the_same_bracket_wherever_it_starts():
    rng = np.random.default_rng(3)
    for ns in LEVELS:
        z = [float(v) for v in _coords(rng, (1, 1), ns, np.float64)[0, 0]]
        targets = z + [z[0] - 1.0, z[-1] + 1.0, -math.inf, math.inf] + [float(v) for v in rng.uniform(z[0], z[-1], 20)]
        for x in targets:
            below = [k for k in range(ns - 1) if z[k] <= x]
            want = max(below) if below else 0
            assert {V.hunt(z, x, start) for start in range(ns - 1)} == {want}, (ns, x)
        for start in range(ns - 1):  # a NaN target leaves k where it was
            assert V.hunt(z, V.NAN, start) == start
    # degenerate coordinates end too, inside 0 ... ns-2
    for z in ([3.0, 2.0, 1.0, 0.0], [0.0] * 4, [V.NAN] * 4, [0.0, V.NAN, 2.0, 1.0]):
        for x in (-1.0, 0.0, 1.5, 5.0, V.NAN):
            for start in range(3):
                assert 0 <= V.hunt(z, x, start) <= 2
                out, _ = V.interp_column(z, [x], [1.0, 2.0, 3.0, 4.0], V.CUBIC_MONOTONE, V.EXTEND, start)
                assert len(out) == 1


# ---- known answers ---------------------------------------------------------------------------------------------------------------
def test_linear_reproduces_a_linear_function_and_is_exact_at_the_source_levels():
    """f = a + b z.  With t = (x - z_k) / h exact, out = f_k + t (f_{k+1} - f_k); the evaluation rounds t, 1 - t, the two products and
    the sum, each relative to a term of size at most max|f|: 5 eps max|f| covers them, plus 2 eps max|f| for the roundings in f
    itself at the two nodes and 1 for the comparison value: 8 eps max|f|."""
    rng = np.random.default_rng(4)
    worst = 0.0
    for ns in LEVELS:
        z = _coords(rng, (4, 4), ns, np.float64)
        a, b = rng.uniform(-5, 5, (4, 4, 1)), rng.uniform(-3, 3, (4, 4, 1))
        q = a + b * z
        x = _targets("shuffled", rng, z, 9, np.float64)
        scale = np.abs(q).max(axis=2, keepdims=True)
        for method in (V.LINEAR, V.CUBIC, V.CUBIC_MONOTONE):
            out = V.interp(q, z, x, method)
            err = np.abs(out - (a + b * x)) / (EPS * scale)
            if method == V.LINEAR:
                worst = max(worst, float(err.max()))
                assert err.max() <= 8, (ns, err.max())
        # at the source levels: t == 0 (or 1 at the last): (1 - 0) * q[k] + 0 * q[k+1] is q[k] exactly
        for method in (V.NEAREST, V.LINEAR):
            assert V.same_bits(V.interp(q, z, z, method), q).all(), (method, ns)
        # the line extended: the same bound, with max|f| taken over the targets too
        xo = np.concatenate([z[..., :1] - 1.5, z[..., -1:] + 2.5], axis=2)
        out = V.interp(q, z, xo, V.CUBIC, V.EXTEND)
        want = a + b * xo
        big = np.maximum(scale, np.abs(want).max(axis=2, keepdims=True)) * (1 + np.abs(xo - z[..., [0, -1]]) / np.diff(z, axis=2)[..., [0, -1]])
        assert (np.abs(out - want) <= 8 * EPS * big).all()
    print(f"linear: worst error {worst:.2f} eps max|f|")


def test_cubic_reproduces_a_cubic_polynomial_in_the_interior_intervals():
    """Lagrange on four nodes is exact for a cubic in exact arithmetic.  In floating point each weight w_a carries 3 subtractions, 4
    multiplications and 1 division (8 roundings, relative), each product w_a q_a one more, and the three additions at most 3 more on
    partial sums bounded by sum |w_a q_a|: |out - p(x)| <= 12 eps sum_a |w_a| |q_a| + the roundings of q_a themselves (1 eps each,
    inside the same sum) <= 13 eps L max|q_a|, with L = sum_a |w_a| the Lebesgue function of the four nodes at x -- the condition
    of the weights, computed here from the nodes in use -- and 1 eps max|p| for the comparison value."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for ns in (4, 5, 6, 17):
        z = _coords(rng, (4, 4), ns, np.float64)
        c = rng.uniform(-2, 2, (4, 4, 4, 1))
        poly = lambda v: ((c[:, :, 3] * v + c[:, :, 2]) * v + c[:, :, 1]) * v + c[:, :, 0]  # noqa: E731
        q = poly(z)
        lo, hi = z[..., 1:2], z[..., ns - 2 : ns - 1]  # the interior intervals: k = 1 ... ns-3
        x = lo + (hi - lo) * rng.uniform(0, 1, (4, 4, 11))
        x = np.minimum(x, np.nextafter(hi, -np.inf))
        out = V.interp(q, z, x, V.CUBIC)
        for i in range(4):
            for j in range(4):
                zc = [float(v) for v in z[i, j]]
                for m in range(x.shape[2]):
                    xm = float(x[i, j, m])
                    k = V.hunt(zc, xm, 0)
                    assert 1 <= k <= ns - 3
                    w = V.lagrange_weights(xm, *zc[k - 1 : k + 3])
                    lebesgue = sum(abs(v) for v in w)
                    qmax = float(np.abs(q[i, j, k - 1 : k + 3]).max())
                    want = float(poly(x)[i, j, m])
                    bound = EPS * (13 * lebesgue * qmax + abs(want))
                    err = abs(float(out[i, j, m]) - want)
                    worst = max(worst, err / bound)
                    assert err <= bound, (ns, i, j, m, err, bound)
    print(f"cubic: worst error {worst:.3f} of the bound")
    # the end intervals (and every interval when ns < 4) are linear: equal to the linear method bit for bit
    for ns in (2, 3, 4, 6):
        z = _coords(rng, (2, 2), ns, np.float64)
        q = _values(rng, (2, 2, ns), np.float64)
        for k in ([0, ns - 2] if ns >= 4 else range(ns - 1)):
            x = z[..., k : k + 1] + (z[..., k + 1 : k + 2] - z[..., k : k + 1]) * rng.uniform(0, 1, (2, 2, 5))
            x = np.minimum(x, np.nextafter(z[..., k + 1 : k + 2], -np.inf)) if k < ns - 2 else x
            for method in (V.CUBIC, V.CUBIC_MONOTONE):
                assert V.same_bits(V.interp(q, z, x, method), V.interp(q, z, x, V.LINEAR)).all(), (ns, k, method)


def test_cubic_monotone_never_leaves_the_brackets_two_values():
    rng = np.random.default_rng(6)
    clipped = 0
    for ns in (4, 5, 6, 17):
        z = _coords(rng, (4, 4), ns, np.float64)
        q = rng.uniform(-1, 1, (4, 4, ns)) * 10.0 ** rng.integers(-2, 3, (4, 4, 1))  # rough: the cubic overshoots
        lo, hi = z[..., 1:2], z[..., ns - 2 : ns - 1]
        x = np.minimum(lo + (hi - lo) * rng.uniform(0, 1, (4, 4, 13)), np.nextafter(hi, -np.inf))
        out = V.interp(q, z, x, V.CUBIC_MONOTONE)
        raw = V.interp(q, z, x, V.CUBIC)
        for i in range(4):
            for j in range(4):
                zc = [float(v) for v in z[i, j]]
                for m in range(x.shape[2]):
                    k = V.hunt(zc, float(x[i, j, m]), 0)
                    a, b = q[i, j, k], q[i, j, k + 1]
                    assert min(a, b) <= out[i, j, m] <= max(a, b)
                    assert out[i, j, m] == min(max(raw[i, j, m], min(a, b)), max(a, b))
        clipped += int((out != raw).sum())
    assert clipped > 50  # the limiter was at work


def test_outside_values():
    z, q = [1.0, 2.0, 4.0], [10.0, 20.0, 60.0]
    x = [0.0, 5.0, 1.0, 4.0]
    for method in (V.LINEAR, V.CUBIC, V.CUBIC_MONOTONE):
        assert V.interp_column(z, x, q, method, V.CLAMP)[0] == [10.0, 60.0, 10.0, 60.0]
        assert V.interp_column(z, x, q, method, V.EXTEND)[0] == [0.0, 80.0, 10.0, 60.0]
        assert V.interp_column(z, x, q, method, V.FILL)[0] == [("fill",), ("fill",), 10.0, 60.0]  # the end levels are inside
    assert V.fill_item(1e300, np.float32) == np.inf and V.fill_item(0.1, np.float32) == np.float32(0.1)
    assert V.fill_item(-math.nan, np.float64).view(np.uint64) == V.QNAN[8]
    assert V.div(1.0, 0.0) == math.inf and V.div(-1.0, 0.0) == -math.inf and math.isnan(V.div(0.0, 0.0))
    assert V.same_bits(np.array([np.nan, -0.0]), np.array([-np.nan, 0.0])).tolist() == [True, False]


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_header_signature_and_the_abi_is_still_8():
    # the header states the contract and that the reference has no counterpart; the enums of header and binding agree
    E.check_binding("gt4mi_vertical_interp",
                    ["const gt4mi_field* dst", "const gt4mi_field* src", "int nfields", "const gt4mi_field* src_coord",
                     "const gt4mi_field* dst_coord", "const int64_t extent_ij[2]", "int64_t ns", "int64_t nd", "int elem_size",
                     "int coord_elem_size", "int method", "int outside", "double fill_value", "int flags", "void* stream", "int* launches"],
                    prefix="VINTERP",
                    constants=("NEAREST", "LINEAR", "CUBIC", "CUBIC_MONOTONE", "OUTSIDE_CLAMP", "OUTSIDE_LINEAR", "OUTSIDE_FILL", "DRY_RUN"),
                    phrases=("no reference counterpart", "user stencils", "while k < ns-2 and z[k+1] <= x", "while k > 0 and z[k] > x",
                             "(1.0 - t) * q[k] + t * q[k+1]", "((w0*q0 + w1*q1) + w2*q2) + w3*q3", "k < 1 or k > ns-3", "canonical quiet NaN",
                             "Path independence", "no address depends on the data"))
    assert vertical.INTERP_METHODS == {"nearest": 0, "linear": 1, "cubic": 2, "cubic_monotone": 3}
    assert vertical.OUTSIDE == {"clamp": 0, "linear": 1, "fill": 2}


DST, SRC, ZS, ZD = 0x10_0000, 0x4000_0000, 0x8000_0000, 0xC000_0000  # made-up device addresses, far apart
NS, ND = 5, 3


def _field(ptr, nk, shape_ij=(6, 6), strides=None, origin=(1, 1, 0), itemsize=8):  # (nk first; this file's plane)
    return E.field(ptr, (*shape_ij, nk), strides, origin, itemsize)


def _call(dst, src, zs, zd, nfields=1, extent=(4, 4), ns=NS, nd=ND, size=8, coord_size=8, method=1, outside=0, fill=math.nan, flags=0):
    return E.call("gt4mi_vertical_interp", as_arg(dst), as_arg(src), nfields, as_arg(zs), as_arg(zd), int64s(extent), ns, nd, size, coord_size,
                  method, outside, fill, flags | _lib.VINTERP_DRY_RUN, None, outs=(77,))


def test_every_refusal_of_the_c_entry_without_a_gpu():
    """Every check runs before the first launch: these calls carry made-up device addresses and the dry-run flag.  Return code and
    the BYTES of the message."""
    d, s, zs, zd = _field(DST, ND), _field(SRC, NS), _field(ZS, NS), _field(ZD, ND)
    rc, msg, launches = _call(d, s, zs, zd)
    assert rc == 0 and launches == 1, msg
    for method in range(4):
        for outside in range(3):
            for size, coord_size in ((4, 4), (4, 8), (8, 4), (8, 8)):
                args = [_field(p, n, itemsize=i) for p, n, i in ((DST, ND, size), (SRC, NS, size), (ZS, NS, coord_size), (ZD, ND, coord_size))]
                rc, msg, launches = _call(*args, size=size, coord_size=coord_size, method=method, outside=outside, fill=-1.5)
                assert rc == 0 and launches == 1, msg

    def refused(code, message, *args, **kwargs):
        rc, msg, launches = _call(*args, **kwargs)
        assert (rc, msg, launches) == (code, message, 0), (rc, msg, launches)

    # null tables, null coordinate fields, null extent, null data
    refused(INV, b"vertical_interp: dst is null", None, s, zs, zd)
    refused(INV, b"vertical_interp: src is null", d, None, zs, zd)
    refused(INV, b"vertical_interp: src_coord is null", d, s, None, zd)
    refused(INV, b"vertical_interp: dst_coord is null", d, s, zs, None)
    refused(INV, b"vertical_interp: extent_ij is null", d, s, zs, zd, extent=None)
    for n, what in enumerate(("dst", "src", "src_coord", "dst_coord")):
        args = [d, s, zs, zd]
        args[n] = _field(0, 8)
        refused(INV, f"vertical_interp: {what} 0 is null".encode(), *args)
    # counts, extents, method, outside, flags
    refused(INV, b"vertical_interp: nfields = 0, at least one pair is needed", d, s, zs, zd, nfields=0)
    refused(INV, b"vertical_interp: nfields = -2, at least one pair is needed", d, s, zs, zd, nfields=-2)
    levels = b"vertical_interp: ns = %d source and nd = %d target levels, at least two source levels and one target level are needed"
    refused(INV, levels % (1, ND), d, s, zs, zd, ns=1)  # one level has nothing to interpolate between
    refused(INV, levels % (0, ND), d, s, zs, zd, ns=0)
    refused(INV, levels % (NS, 0), d, s, zs, zd, nd=0)
    refused(INV, levels % (NS, -1), d, s, zs, zd, nd=-1)
    refused(INV, levels % (2**31, ND), d, s, zs, zd, ns=2**31)
    refused(INV, b"vertical_interp: invalid extent -1 along axis 1", d, s, zs, zd, extent=(4, -1))
    refused(INV, b"vertical_interp: invalid extent 2147483648 along axis 0", d, s, zs, zd, extent=(2**31, 4))
    refused(INV, b"vertical_interp: unknown method 4", d, s, zs, zd, method=4)
    refused(INV, b"vertical_interp: unknown method -1", d, s, zs, zd, method=-1)
    refused(INV, b"vertical_interp: unknown outside value 3", d, s, zs, zd, outside=3)
    refused(INV, b"vertical_interp: unknown outside value -1", d, s, zs, zd, outside=-1)
    refused(INV, b"vertical_interp: unknown bits in flags 0x102", d, s, zs, zd, flags=2)
    # item sizes other than 4 or 8
    refused(UNS, b"vertical_interp: field item size 2 is not supported (float32 or float64)", d, s, zs, zd, size=2)
    refused(UNS, b"vertical_interp: coordinate item size 16 is not supported (float32 or float64)", d, s, zs, zd, coord_size=16)
    # a box that does not fit its field: I, J, and the levels of every role (a coordinate field has as many as its fields)
    refused(OOB, b"vertical_interp: dst 0: origin 1 + extent 6 along axis 0 is outside the array (shape 6)", d, s, zs, zd, extent=(6, 4))
    refused(OOB, b"vertical_interp: src 0: origin 1 + extent 6 along axis 1 is outside the array (shape 6)", _field(DST, ND, (8, 8)), s, zs, zd,
            extent=(4, 6))
    refused(OOB, b"vertical_interp: dst 0: origin 1 + extent 4 along axis 2 is outside the array (shape 3)".replace(b"origin 1", b"origin 0"),
            d, s, zs, zd, nd=ND + 1)
    refused(OOB, b"vertical_interp: src 0: origin 0 + extent 6 along axis 2 is outside the array (shape 5)", d, s, zs, zd, ns=NS + 1)
    refused(OOB, b"vertical_interp: src_coord 0: origin 0 + extent 5 along axis 2 is outside the array (shape 4)", d, s, _field(ZS, NS - 1), zd)
    refused(OOB, b"vertical_interp: dst_coord 0: origin 0 + extent 3 along axis 2 is outside the array (shape 2)", d, s, zs, _field(ZD, ND - 1))
    refused(OOB, b"vertical_interp: src 0: negative origin -1 along axis 1", d, _field(SRC, NS, origin=(1, -1, 0)), zs, zd)
    # strides and alignment the kernels do not take
    refused(UNS, b"vertical_interp: dst 0: byte stride 52 along axis 1 is not a multiple of the item size", _field(DST, ND, strides=(8, 52, 312)),
            s, zs, zd)
    refused(UNS, b"vertical_interp: src_coord 0 is not aligned to its item size", d, s, _field(ZS + 4, NS), zd)
    refused(UNS, b"vertical_interp: src 0 is not aligned to its item size", d, _field(SRC + 2, NS), zs, zd)
    # stride 0: refused for a dst on an extent above 1, fine on an extent of 1; a src and the coordinate fields broadcast, and a
    # broadcast axis of a coordinate field has no shape to check
    hint = b" (only a src or a coordinate field may be broadcast)"
    refused(INV, b"vertical_interp: dst 0 has stride 0 along axis 0" + hint, _field(DST, ND, strides=(0, 8, 48)), s, zs, zd)
    refused(INV, b"vertical_interp: dst 0 has stride 0 along axis 2" + hint, _field(DST, ND, strides=(8, 48, 0)), s, zs, zd)
    rc, msg, _ = _call(_field(DST, 1, strides=(8, 48, 0)), s, zs, _field(ZD, 1), nd=1)
    assert rc == 0, msg
    rc, msg, _ = _call(d, _field(SRC, NS, strides=(0, 0, 8)), zs, zd)
    assert rc == 0, msg
    column = lambda ptr, n: _lib.Field.make(ptr, (1, 1, n), (0, 0, 8), (0, 0, 0))  # noqa: E731  (a Field[K])
    rc, msg, launches = _call(d, s, column(ZS, NS), column(ZD, ND))
    assert rc == 0 and launches == 1, msg
    refused(OOB, b"vertical_interp: src_coord 0: origin 0 + extent 5 along axis 2 is outside the array (shape 4)", d, s, column(ZS, NS - 1),
            column(ZD, ND))
    # overlap in memory: a dst against its src, another pair's src, either coordinate field, another dst; a byte apart is fine
    refused(UNS, b"vertical_interp: dst 0 and src 0 overlap in memory", d, _field(DST, NS), zs, zd)
    first, last = 8 * (1 + 6), 8 * (4 + 6 * 4 + 36 * (ND - 1))  # byte offsets of the dst box's first and last item
    refused(UNS, b"vertical_interp: dst 0 and src 0 overlap in memory", d, _field(DST + last - first, NS), zs, zd)  # src's first item IS dst's last
    rc, msg, _ = _call(d, _field(DST + last - first + 8, NS), zs, zd)  # the byte ranges of the BOXES do not meet
    assert rc == 0, msg
    refused(UNS, b"vertical_interp: dst 0 and src_coord overlap in memory", d, s, _field(DST + 64, NS), zd)
    refused(UNS, b"vertical_interp: dst 0 and dst_coord overlap in memory", d, s, zs, column(DST + 8 * 40, ND))
    two = lambda a, b: E.table((a, b))  # noqa: E731
    refused(UNS, b"vertical_interp: dst 0 and src 1 overlap in memory", two(d, _field(DST + 0x1000, ND)), two(s, _field(DST + 64, NS)), zs, zd,
            nfields=2)
    refused(UNS, b"vertical_interp: dst 0 and dst 1 overlap in memory", two(d, _field(DST + 128, ND)), two(s, _field(SRC + 0x1000, NS)), zs, zd,
            nfields=2)
    rc, msg, launches = _call(two(d, _field(DST + 0x1000, ND)), two(s, s), zs, zd, nfields=2)  # one src for two dsts is fine
    assert rc == 0 and launches == 1, msg
    rc, msg, _ = _call(_field(DST, NS), s, zs, zs, nd=NS)  # and so is one coordinate field on both sides (the identity)
    assert rc == 0, msg
    # an extent with a zero entry: OK, nothing to launch -- after the checks
    rc, msg, launches = _call(d, s, zs, zd, extent=(4, 0))
    assert rc == 0 and launches == 0, msg
    refused(OOB, b"vertical_interp: dst 0: origin 1 + extent 7 along axis 0 is outside the array (shape 6)", d, s, zs, zd, extent=(7, 0))


def test_launches_are_one_per_eight_pairs():
    d = E.table(_field(DST + n * 0x1000, ND) for n in range(9))
    s = E.table(_field(SRC + n * 0x1000, NS) for n in range(9))
    zs, zd = _field(ZS, NS), _field(ZD, ND)
    assert [_call(d, s, zs, zd, nfields=n)[::2] for n in (1, 8, 9)] == [(0, 1), (0, 1), (0, 2)]


def test_the_kernels_are_in_the_resource_log_without_scratch():
    kernels = E.kernel_resources(r"vertical_interp_kernel")
    # 2 field types x 2 coordinate types x 4 methods x the register budgets for 1, 4 and 8 entries
    assert len(kernels) == 48 and len({name for name, *_ in kernels}) == 48, kernels
    for name, scratch, waves, lds in kernels:
        assert int(scratch) == 0 and int(waves) >= 2 and int(lds) == 0, (name, scratch, waves, lds)


# ---- the Python interface: every refusal before any GPU work ---------------------------------------------------------------
def _good(**over):
    args = dict(dst=E.host_field((8, 9, 3)), src=E.host_field(HOST), src_coord=E.host_field((8, 9, 5)), dst_coord=E.host_field((3,)))
    args.update(over)
    return args.pop("dst"), args.pop("src"), args


@pytest.mark.parametrize("kwargs, error, match", [
    (dict(halo=2.0), ValueError, "halo must be"),
    (dict(halo=((1, 1.5), (1, 1))), TypeError, "halo widths must be ints"),
    (dict(halo=-1), ValueError, "must not be negative"),
    (dict(halo=5), ValueError, "leave no domain"),
    (dict(halo=2, origin=(1, 2, 0)), ValueError, "negative origin -1 along axis 0"),
    (dict(origin=(0, 0, 0, 0)), ValueError, "at most three entries"),
    (dict(origin=(0, 0, 5)), ValueError, "leaves no level"),
    (dict(origin=(0, 0, 4)), ValueError, "ns = 1 source"),  # one source level left: the library's refusal
    (dict(method="pcm"), ValueError, "method must be one of"),
    (dict(outside="wrap"), ValueError, "outside must be one of"),
    (dict(outside="fill", fill_value="0"), TypeError, "fill_value must be a Python float"),
    (dict(halo=((1, 2), (0, 3)), method="cubic_monotone", outside="fill", fill_value=-999.0), TypeError, "device fields"),  # all checks passed
    (dict(), TypeError, "device fields"),
])
def test_python_refusals_need_no_gpu(kwargs, error, match):
    dst, src, coords = _good()
    if kwargs.get("origin") == (0, 0, 4):
        coords["dst_coord"] = E.host_field((7,))  # (origin 4 leaves 3 of them)
        dst = E.host_field((8, 9, 7))
    with pytest.raises(error, match=match):
        vertical.interpolate_levels(dst, src, **coords, **kwargs)
    with pytest.raises(error, match=match):
        vertical.VerticalInterp([dst], [src], **coords, **kwargs)


def test_python_refusals_about_the_fields_themselves():
    import torch

    R = vertical.interpolate_levels
    dst, src, coords = _good()
    with pytest.raises(ValueError, match="at least one"):
        R([], [], **coords)
    with pytest.raises(ValueError, match="2 destination.s. and 1 source"):  # unequal list lengths
        R([dst, E.host_field((8, 9, 3))], [src], **coords)
    with pytest.raises(TypeError, match="host"):
        R(torch.zeros(8, 9, 3, dtype=torch.float64), src, **coords)  # as_device_array's own refusal of a host array
    with pytest.raises(TypeError):
        R(dst, np.zeros((8, 9, 5)), **coords)
    with pytest.raises(TypeError):
        R(dst, src, src_coord=np.zeros((8, 9, 5)), dst_coord=coords["dst_coord"])
    with pytest.raises(ValueError, match="takes IJK fields"):
        R(E.host_field((8, 9)), src, **coords)
    with pytest.raises(ValueError, match="dst_coord must be an IJK field or a Field.K."):
        R(dst, src, src_coord=coords["src_coord"], dst_coord=E.host_field((9, 3)))
    # dtypes: the fields share one, the coordinate fields share one (not necessarily the same), all float32 or float64
    with pytest.raises(TypeError, match="share a dtype"):
        R(E.host_field((8, 9, 3), "float32"), src, **coords)
    with pytest.raises(TypeError, match="interpolate_levels takes float32 or float64 fields"):
        R(E.host_field((8, 9, 3), "int64"), E.host_field(HOST, dtype="int64"), **coords)
    with pytest.raises(TypeError, match="src_coord and dst_coord share a dtype"):
        R(dst, src, src_coord=coords["src_coord"], dst_coord=E.host_field((3,), "float32"))
    with pytest.raises(TypeError, match="coordinate fields are float32 or float64"):
        R(dst, src, src_coord=E.host_field((8, 9, 5), "int32"), dst_coord=E.host_field((3,), "int32"))
    with pytest.raises(TypeError, match="device fields"):  # float32 fields against float64 coordinates is a combination of its own
        R(E.host_field((8, 9, 3), "float32"), E.host_field(HOST, dtype="float32"), **coords)
    # levels: the sources share theirs, a coordinate field has exactly as many
    with pytest.raises(ValueError, match="sources of one call share their number of levels: 5 and 4"):
        R([dst, E.host_field((8, 9, 3))], [src, E.host_field((8, 9, 4))], **coords)
    with pytest.raises(ValueError, match="src_coord has 6 levels along K, the sources have 5"):
        R(dst, src, src_coord=E.host_field((8, 9, 6)), dst_coord=coords["dst_coord"])
    with pytest.raises(ValueError, match="dst_coord has 4 levels along K, the destinations have 3"):
        R(dst, src, src_coord=coords["src_coord"], dst_coord=E.host_field((4,)))
    with pytest.raises(ValueError, match="ns = 1 source"):
        R(dst, E.host_field((8, 9, 1)), src_coord=E.host_field((1,)), dst_coord=coords["dst_coord"])
    # a field onto itself; a dst that is also the coordinate field
    x = E.host_field((8, 9, 5))
    with pytest.raises(TypeError, match="dst 0 and src 0 overlap in memory"):
        R(x, x, src_coord=coords["src_coord"], dst_coord=E.host_field((5,)))
    z = E.host_field((8, 9, 5))
    with pytest.raises(TypeError, match="dst 0 and src_coord overlap in memory"):
        R(z, E.host_field((8, 9, 5)), src_coord=z, dst_coord=E.host_field((5,)))


def test_a_frozen_interpolation_knows_its_box_and_refuses_to_run_after_an_array_died(monkeypatch):
    """The weak references are taken last, behind the device check: what they guard is shown on a VerticalInterp whose device
    check is made to pass for host memory -- the call itself is never reached, the dead reference is found first."""
    E.on_device(monkeypatch)
    dsts, srcs = [E.host_field((8, 9, 3)) for _ in range(9)], [E.host_field((10, 9, 5)) for _ in range(9)]
    zs, zd = E.host_field((8, 9, 5), "float32"), E.host_field((3,), "float32")
    vi = vertical.VerticalInterp(dsts, srcs, src_coord=zs, dst_coord=zd, method="cubic", outside="fill", fill_value=-1, halo=1)
    assert (vi.ns, vi.nd, vi.launches, vi.extent, vi.domain, vi.origin, vi.method, vi.outside) == (5, 3, 2, (8, 9), (6, 7), (1, 1, 0), "cubic", "fill")
    assert vertical.VerticalInterp(dsts[:8], srcs[:8], src_coord=zs, dst_coord=zd).launches == 1
    del zd
    E.refuses_a_dead_array(vi)
