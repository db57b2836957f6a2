"""``gt4py_amd.linefind`` without a GPU: the contract's restatement (tests/line_find_ref.py), plain Python against vectorised numpy
and both against ``numpy.argmax`` / ``numpy.argmin``, directed crossing cases, every refusal of the C entry through the dry run
(made-up addresses that are never dereferenced), the declaration, the kernels' resources and the Python interface's argument
checks."""

import ctypes

import numpy as np
import pytest

import entry_checks as E
import line_find_ref as R
from entry_checks import INV, OOB, UNS, as_arg, int64s
from gt4py_amd import _lib, linefind

HOST = (8, 9, 5)  # the shape of a host field where a test states none
NAN = float("nan")


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _lines(rng, n, dtype, lines=6):
    """Small integers and halves around the level 0.5: crossings, items equal to the level and ties are all common."""
    return (rng.integers(-4, 5, (n, lines)) / 2.0).astype(dtype)


def test_the_two_restatements_agree_bit_for_bit():
    rng = np.random.default_rng(1)
    for dtype in (np.float32, np.float64):
        for n in (1, 2, 3, 17, 40):
            x = _lines(rng, n, dtype)
            z = np.cumsum(rng.uniform(0.5, 2, x.shape), axis=0).astype(dtype)
            x[rng.integers(0, n), 2] = np.nan
            x[rng.integers(0, n), 3] = np.inf
            x[rng.integers(0, n), 4] = -np.inf
            modes = [("crossing", 0.5, d) for d in R.DIRECTIONS] + [("crossing", 0.3, "any"), ("argmax", None, "any"), ("argmin", None, "any")]
            for what, level, direction in modes:
                for reverse in (False, True):
                    for coord in (None, z, z[:, :1]):
                        whole = R.find(x, what, level, direction, reverse, coord, missing=-7.0)
                        assert whole.dtype == np.float64 and whole.shape == (3,) + x.shape[1:]
                        for l in range(x.shape[1]):
                            zl = None if coord is None else coord[:, min(l, coord.shape[1] - 1)]
                            one = R.find_line(x[:, l], what, level, direction, reverse, zl, missing=-7.0)
                            assert R.same_bits(whole[:, l], np.array(one)).all(), (dtype, n, what, direction, reverse, l, whole[:, l], one)


def test_the_extrema_are_numpy_argmax_and_argmin_along_each_axis():
    rng = np.random.default_rng(2)
    for dtype in (np.float32, np.float64):
        box = (rng.integers(-3, 4, (7, 6, 9)) / 2.0).astype(dtype)  # many ties
        box[2, 3, :] = [1, np.nan, 5, np.nan, 2, 0, 0, 0, 0]  # the first NaN wins
        box[:, 1, 4] = [3, 9, -9, 9, -9, 3, np.nan]  # a NaN in the last item; ties of both extremes in front of it
        box[4, :, 2] = [-0.0, 0.0, -0.0, 0.0, -0.0, 0.0]  # signed zeros are equal: the first stays
        z = rng.uniform(0, 1, box.shape).astype(dtype)
        for axis in range(3):
            n = box.shape[axis]
            for what, arg in (("argmax", np.argmax), ("argmin", np.argmin)):
                got = R.find_along(box, axis, what, coord=z)
                want = arg(box, axis=axis)
                assert np.array_equal(got[0], want.astype(np.float64)), (dtype, axis, what)
                assert R.same_bits(got[2], np.take_along_axis(box, np.expand_dims(want, axis), axis).squeeze(axis).astype(np.float64)).all()
                assert np.array_equal(got[1], np.take_along_axis(z, np.expand_dims(want, axis), axis).squeeze(axis).astype(np.float64))
                assert np.array_equal(R.find_along(box, axis, what)[1], got[0])  # no coord: the position
                back = R.find_along(box, axis, what, reverse=True)
                want = n - 1 - arg(np.flip(box, axis), axis=axis)  # the tie from the far end, in forward units
                assert np.array_equal(back[0], want.astype(np.float64)), (dtype, axis, what)
    line = np.array([1.0, 5.0, 5.0, 2.0])
    for f in (R.find_line, lambda *a, **k: R.find(np.asarray(a[0])[:, None], *a[1:], **k)[:, 0]):
        assert [float(v) for v in f(line, "argmax")] == [1.0, 1.0, 5.0]
        assert [float(v) for v in f(line, "argmax", reverse=True)] == [2.0, 2.0, 5.0]
        got = f(np.array([1.0, NAN, 7.0, NAN]), "argmin", reverse=True)
        assert float(got[0]) == 3.0 and np.isnan(got[2])
        assert float(f(np.array([0.0, -0.0]), "argmin")[0]) == 0.0 and float(f(np.array([-0.0, 0.0]), "argmax")[0]) == 0.0


def _both(x, *args, dtype=np.float64, coord=None, **kwargs):
    """A line through both restatements (they must agree): (position, coord, extra) as floats."""
    x = np.asarray(x, dtype=dtype)
    coord = None if coord is None else np.asarray(coord, dtype=dtype)
    one = R.find_line(x, *args, coord=coord, **kwargs)
    many = R.find(x[:, None], *args, coord=None if coord is None else coord[:, None], **kwargs)[:, 0]
    assert R.same_bits(np.array(one), many).all(), (one, many)
    return tuple(float(v) for v in one)


def test_directed_crossing_cases():
    for dtype in (np.float32, np.float64):
        C = lambda x, *a, **k: _both(x, "crossing", *a, dtype=dtype, **k)  # noqa: E731
        # item 0 equal to the level: found at q = 0, t = 0, for every direction; the pairs behind it still count
        for direction in R.DIRECTIONS:
            assert C([2, 3, 1], 2.0, direction) == (0.0, 0.0, 2.0 if direction != "rising" else 1.0)
        # (the reverse scan of the same line starts at 1: the pair (1, 3) rises, the pair (3, 2) falls and ends ON the level)
        assert C([2, 3, 1], 2.0, "any", reverse=True) == (1.5, 1.5, 2.0) and C([2, 3, 1], 2.0, "rising", reverse=True) == (1.5, 1.5, 1.0)
        assert C([2, 3, 1], 2.0, "falling", reverse=True) == (0.0, 0.0, 1.0)
        assert C([2, 3, 1], 2.0, coord=[10, 20, 40]) == (0.0, 10.0, 2.0)
        assert C([1, 3, 2], 2.0, reverse=True, coord=[10, 20, 40]) == (2.0, 40.0, 2.0)  # item 0 of the REVERSE scan
        # -0.0 against the level 0: equal
        assert C([-0.0, 1], 0.0) == (0.0, 0.0, 1.0) and C([1, -0.0, -1], 0.0) == (1.0, 1.0, 1.0)
        # a pair (L, L) is no strict crossing; neither is touching the level from one side and leaving to the same side
        assert C([1, 2, 2, 3], 2.0) == (1.0, 1.0, 1.0)  # the pair (1, 2) rises and ends ON the level; (2, 2) and (2, 3) are none
        assert C([3, 2, 2, 1], 2.0) == (1.0, 1.0, 1.0)
        pos, _, count = C([1, 1, 1], 2.0)
        assert np.isnan(pos) and count == 0.0
        # rising only and falling only on a line that does both
        hill = [0, 4, 0, 4]
        assert C(hill, 1.0, "any") == (0.25, 0.25, 3.0)
        assert C(hill, 1.0, "rising") == (0.25, 0.25, 2.0)
        assert C(hill, 1.0, "falling") == (1.75, 1.75, 1.0)
        # reverse finds the last pair: position = n-1-q - t; rising and falling are in SCAN order
        assert C(hill, 1.0, "any", reverse=True) == (2.25, 2.25, 3.0)  # scan pair q = 0 is items (3, 2): 4 -> 0, t = 0.75
        assert C(hill, 1.0, "falling", reverse=True) == (2.25, 2.25, 2.0)
        assert C(hill, 1.0, "rising", reverse=True) == (1.75, 1.75, 1.0)  # scan pair q = 1: items (2, 1): 0 -> 4, t = 0.25
        # a NaN beside the crossing makes none; the next true pair is found
        assert C([0, NAN, 4, 0, 4], 1.0) == (2.75, 2.75, 2.0)
        assert C([0, NAN, 4], 1.0, missing=-1.0) == (-1.0, -1.0, 0.0)
        # a NaN level finds nothing; missing is returned in position and coord
        assert C([0, 4, 0], NAN, missing=-5.0, coord=[1, 2, 3]) == (-5.0, -5.0, 0.0)
        pos, crd, count = C([0, 4, 0], 9.0, coord=[1, 2, 3])
        assert np.isnan(pos) and np.isnan(crd) and count == 0.0
        # infinities: a jump to +inf crosses every finite level at t = 0
        assert C([0, np.inf], 1.0) == (0.0, 0.0, 1.0)
        # n = 1: no pair, only the equality rule
        assert C([2], 2.0, coord=[7]) == (0.0, 7.0, 1.0) and C([2], 2.0, reverse=True) == (0.0, 0.0, 1.0)
        assert C([2], 1.0, missing=-1.0) == (-1.0, -1.0, 0.0)
        # crossings counted on a line with several
        assert C([0, 2, 0, 2, 0, 2, 0], 1.0)[2] == 6.0 and C([0, 2, 0, 2, 0, 2, 0], 1.0, "falling")[2] == 3.0
        # coord interpolation: a 1-d coord and a per-line coord
        assert C([0, 4, 8], 5.0, coord=[100, 200, 1000]) == (1.25, 400.0, 1.0)
        assert C([0, 4, 8], 5.0, coord=[100, 200, 1000], reverse=True) == (1.25, 400.0, 1.0)
    box = np.array([[0.0, 0.0], [4.0, 2.0], [8.0, 4.0]]).reshape(3, 2, 1)  # two lines along axis 0
    z_line, z_box = np.array([100.0, 200.0, 1000.0]), np.array([[100.0, 0.0], [200.0, 10.0], [1000.0, 30.0]]).reshape(3, 2, 1)
    got = R.find_along(box, 0, "crossing", 3.0, coord=z_line)
    assert got.shape == (3, 2, 1) and got[:, :, 0].T.tolist() == [[0.75, 175.0, 1.0], [1.5, 600.0, 1.0]]
    got = R.find_along(box, 0, "crossing", 3.0, coord=z_box)
    assert got[:, :, 0].T.tolist() == [[0.75, 175.0, 1.0], [1.5, 20.0, 1.0]]
    # t is the float64 quotient whatever the fields' type
    x32 = np.array([0.1, 0.7], dtype=np.float32)
    t = (np.float64(0.3) - np.float64(x32[0])) / (np.float64(x32[1]) - np.float64(x32[0]))
    assert _both(x32, "crossing", 0.3, dtype=np.float32)[0] == float(t)


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_header_signature_and_the_abi_is_still_8():
    fp, i64p, c_int, ip = ctypes.POINTER(_lib.Field), ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.POINTER(ctypes.c_int)
    E.check_binding("gt4mi_line_find",
                    ["const gt4mi_field* fields", "int nfields", "const gt4mi_field* coord", "const int64_t extent[3]", "int axis",
                     "int elem_size", "int what", "int direction", "const double* level", "double missing", "double* result", "int flags",
                     "void* stream", "int* path", "int* launches"],
                    argtypes=[fp, c_int, fp, i64p, c_int, c_int, c_int, c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.c_void_p,
                              c_int, ctypes.c_void_p, ip, ip],
                    prefix="FIND", constants=("CROSSING", "ARGMAX", "ARGMIN", "ANY", "RISING", "FALLING", "POSITION", "COORD", "EXTRA", "ROWS",
                                              "REVERSE", "DRY_RUN"),
                    phrases=("y[q] < L && y[q+1] >= L", "y[q] > L && y[q+1] <= L", "t = (L - y[q]) / (y[q+1] - y[q])", "double(n-1-q) - t",
                             "zc[q] + t * (zc[q+1] - zc[q])", "no FMA", "numpy.argmax", "the first NaN met wins", "no early exit", "cupy"))


FLD, CRD, RES = 0x10_0000, 0x4000_0000, 0x8000_0000  # made-up addresses, far apart
SHAPE = (6, 7, 5)
CROSSING, ARGMAX, ARGMIN = _lib.FIND_CROSSING, _lib.FIND_ARGMAX, _lib.FIND_ARGMIN
LEVEL = object()


def _field(ptr, shape=SHAPE, *rest, **kwargs):  # (this file's shape)
    return E.field(ptr, shape, *rest, **kwargs)


def _call(fields, coord=None, nfields=1, extent=(4, 5, 5), axis=0, size=8, what=CROSSING, direction=0, level=LEVEL, result=RES, flags=0):
    if level is LEVEL:
        level = (ctypes.c_double * max(nfields, 1))(*([273.15] * max(nfields, 1))) if what == CROSSING else None
    rc, msg, path, launches = E.call("gt4mi_line_find", as_arg(fields), nfields, as_arg(coord), int64s(extent), axis, size, what, direction,
                                     level, NAN, result, flags | _lib.FIND_DRY_RUN, None, outs=(77, 77))
    return rc, msg, launches, path


def test_every_refusal_of_the_c_entry_without_a_gpu():
    """Every check runs before the first launch: these calls carry made-up device addresses and the dry-run flag."""
    T = _lib.LINE_PATH_TILES
    for what in (CROSSING, ARGMAX, ARGMIN):
        for direction in ((0, 1, 2) if what == CROSSING else (0,)):
            for flags in (0, _lib.FIND_REVERSE):
                for result in (RES, None):  # a dry run needs no result
                    rc, msg, launches, path = _call(_field(FLD), what=what, direction=direction, flags=flags, result=result)
                    assert rc == 0 and launches == 1 and path == T, msg
    rc, msg, launches, path = _call(_field(FLD), _field(CRD))
    assert rc == 0 and launches == 1 and path == T, msg
    rc, msg, launches, _ = _call(_field(FLD, itemsize=4), _field(CRD, itemsize=4), size=4, what=ARGMAX)
    assert rc == 0 and launches == 1, msg
    # null pointers
    rc, msg, launches, path = _call(None)
    assert rc == INV and b"line_find: fields is null" in msg and launches == 0 and path == -1
    rc, msg, *_ = _call(_field(FLD), extent=None)
    assert rc == INV and b"line_find: extent is null" in msg
    rc, msg, launches, _ = _call(_field(0))
    assert rc == INV and b"line_find: field 0 is null" in msg and launches == 0
    rc, msg, launches, _ = _call(_field(FLD), _field(0))
    assert rc == INV and b"line_find: coord 0 is null" in msg and launches == 0
    rc, msg, launches, _ = _call(_field(FLD), level=None)
    assert rc == INV and b"line_find: level is null" in msg and launches == 0
    rc, msg, launches, path = _call(_field(FLD), result=None, flags=0)  # (the dry-run bit is added by _call: still fine)
    assert rc == 0
    lib = _lib.load()
    rc = lib.gt4mi_line_find(ctypes.byref(_field(FLD)), 1, None, (ctypes.c_int64 * 3)(4, 5, 5), 0, 8, ARGMAX, 0, None, NAN, None, 0, None, None, None)
    assert rc == INV and b"line_find: result is null" in lib.gt4mi_last_error()  # a real call without a result: refused in front of any launch
    # counts, extents, axis, what, direction, flags, item size
    for n in (0, -2):
        rc, msg, launches, _ = _call(_field(FLD), nfields=n)
        assert rc == INV and b"nfields = %d, at least one field is needed" % n in msg and launches == 0
    rc, msg, *_ = _call(_field(FLD), extent=(4, -1, 5))
    assert rc == INV and b"invalid extent -1 along axis 1" in msg
    rc, msg, *_ = _call(_field(FLD), extent=(4, 2 ** 31, 5))
    assert rc == INV and b"invalid extent 2147483648 along axis 1" in msg
    for axis in (-1, 3):
        rc, msg, *_ = _call(_field(FLD), axis=axis)
        assert rc == INV and b"axis %d is not 0 (I), 1 (J) or 2 (K)" % axis in msg
    for what in (-1, 3):
        rc, msg, *_ = _call(_field(FLD), what=what)
        assert rc == INV and b"what %d is not GT4MI_FIND_CROSSING, GT4MI_FIND_ARGMAX or GT4MI_FIND_ARGMIN" % what in msg
    for direction in (-1, 3):
        rc, msg, *_ = _call(_field(FLD), direction=direction)
        assert rc == INV and b"direction %d is not GT4MI_FIND_ANY, GT4MI_FIND_RISING or GT4MI_FIND_FALLING" % direction in msg
    for flags in (2, 128, 512):
        rc, msg, *_ = _call(_field(FLD), flags=flags)
        assert rc == INV and b"unknown bits in flags" in msg
    for size in (2, 16):
        rc, msg, *_ = _call(_field(FLD), size=size)
        assert rc == UNS and b"item size %d is not supported" % size in msg
    # a level and a direction go with a crossing only
    for what in (ARGMAX, ARGMIN):
        rc, msg, launches, _ = _call(_field(FLD), what=what, level=(ctypes.c_double * 1)(1.0))
        assert rc == INV and b"a level and a direction go with GT4MI_FIND_CROSSING only, what is %d" % what in msg and launches == 0
        rc, msg, launches, _ = _call(_field(FLD), what=what, direction=_lib.FIND_RISING)
        assert rc == INV and b"go with GT4MI_FIND_CROSSING only" in msg and launches == 0
    # a box that does not fit its field, per role and axis
    for n, what in enumerate((b"field 0", b"coord 0")):
        args = [_field(p, (8, 9, 6)) for p in (FLD, CRD)]
        args[n] = _field(args[n].data, SHAPE)
        for axis, extent in ((0, (6, 5, 5)), (1, (4, 7, 5)), (2, (4, 5, 6))):
            rc, msg, launches, _ = _call(*args, extent=extent)
            assert rc == OOB and what in msg and b"axis %d is outside the array" % axis in msg and launches == 0, msg
    rc, msg, *_ = _call(_field(FLD, origin=(1, -1, 0)))
    assert rc == OOB and b"field 0: negative origin -1 along axis 1" in msg
    rc, msg, *_ = _call(_field(FLD, origin=(3, 1, 0)))
    assert rc == OOB and b"field 0: origin 3 + extent 4 along axis 0 is outside the array (shape 6)" in msg
    two = lambda a, b: E.table((a, b))  # noqa: E731
    rc, msg, *_ = _call(two(_field(FLD), _field(FLD + 0x10000, origin=(3, 1, 0))), nfields=2)
    assert rc == OOB and b"field 1: origin 3" in msg
    # strides and alignment
    rc, msg, *_ = _call(_field(FLD, strides=(8, 52, 336)))
    assert rc == UNS and b"multiple of the item size" in msg
    rc, msg, *_ = _call(_field(FLD), _field(CRD + 4))
    assert rc == UNS and b"coord 0 is not aligned to its item size" in msg
    rc, msg, launches, _ = _call(_field(FLD, strides=(0, 8, 56)))
    assert rc == INV and b"field 0 has stride 0 along axis 0 (only the coord may be broadcast)" in msg and launches == 0
    # a 1-d coord along the line axis: broadcast, exempt from the shape check on the other axes, n items needed
    for axis in range(3):
        n = (4, 5, 5)[axis]
        rc, msg, launches, _ = _call(_field(FLD), E.line(CRD, n, axis), axis=axis)
        assert rc == 0 and launches == 1, msg
        rc, msg, *_ = _call(_field(FLD), E.line(CRD, n - 1, axis), axis=axis)
        assert rc == OOB and b"coord 0" in msg and b"axis %d" % axis in msg, msg
    rc, msg, *_ = _call(_field(FLD), E.line(CRD, 5, 1), axis=0)  # 1-d along the wrong axis
    assert rc == OOB and b"coord 0" in msg
    # the result: aligned to 8 bytes, clear of every field and of the coord (a 4 x 5 x 5 box along I: 25 lines, 3 doubles each per field)
    rc, msg, launches, _ = _call(_field(FLD), result=RES + 4)
    assert rc == INV and b"line_find: result is not aligned to 8 bytes" in msg and launches == 0
    first = FLD + 8 * (1 + 6)  # the first item of the box
    rc, msg, launches, _ = _call(_field(FLD), result=first)
    assert rc == INV and b"line_find: result overlaps field 0" in msg and launches == 0
    rc, msg, *_ = _call(_field(FLD), result=first - 3 * 25 * 8 + 8)  # its last double meets the box's first item
    assert rc == INV and b"result overlaps field 0" in msg
    rc, msg, *_ = _call(_field(FLD), result=first - 3 * 25 * 8)  # ends in front of it
    assert rc == 0, msg
    rc, msg, *_ = _call(two(_field(FLD), _field(RES)), nfields=2, result=RES)
    assert rc == INV and b"result overlaps field 1" in msg
    rc, msg, *_ = _call(_field(FLD), _field(RES))
    assert rc == INV and b"result overlaps coord" in msg
    rc, msg, *_ = _call(_field(FLD), E.line(RES + 64, 4, 0))
    assert rc == INV and b"result overlaps coord" in msg
    rc, msg, *_ = _call(_field(FLD), _field(FLD))  # a field as its own coord is fine: nothing is written
    assert rc == 0, msg
    # too many lines for one launch
    huge = _lib.Field.make(FLD, (2, 2 ** 16, 2 ** 15), (8, 16, 2 ** 20), (0, 0, 0))
    rc, msg, launches, _ = _call(huge, extent=(2, 2 ** 16, 2 ** 15), axis=0, result=None)
    assert rc == UNS and b"line_find: too many lines for one launch" in msg and launches == 0
    # an extent with a zero entry: OK, nothing to launch -- after the checks
    rc, msg, launches, _ = _call(_field(FLD), extent=(4, 0, 5))
    assert rc == 0 and launches == 0, msg
    rc, msg, launches, _ = _call(_field(FLD), extent=(7, 0, 5))
    assert rc == OOB and launches == 0


def _restated_path(strides, coord_strides, extent, axis, itemsize=8):
    """include/gt4py_amd.h's rule: TILES where the line axis has unit stride in every field and is longer than 1; else LANES where
    another axis has (the coord may be broadcast along it); else ITEMS."""
    def unit(ax):
        if any(s[ax] != itemsize for s in strides):
            return False
        return coord_strides is None or coord_strides[ax] == itemsize or (ax != axis and coord_strides[ax] == 0)

    if unit(axis) and extent[axis] > 1:
        return _lib.LINE_PATH_TILES
    return _lib.LINE_PATH_LANES if any(unit(ax) and extent[ax] > 1 for ax in range(3) if ax != axis) else _lib.LINE_PATH_ITEMS


def test_launches_are_one_per_eight_fields_and_the_path_follows_the_strides():
    f = E.table(_field(FLD + n * 0x10000) for n in range(9))
    assert [_call(f, nfields=n)[2] for n in (1, 3, 8, 9)] == [1, 1, 1, 2]
    L, T, IT = _lib.LINE_PATH_LANES, _lib.LINE_PATH_TILES, _lib.LINE_PATH_ITEMS
    ifirst, kfirst, jfirst = (8, 48, 336), (280, 40, 8), (56, 8, 336)
    seen = set()
    for extent in ((4, 5, 5), (1, 5, 5), (4, 1, 5), (4, 5, 1), (1, 1, 5), (4, 1, 1)):
        for axis in range(3):
            for s0 in (ifirst, kfirst, jfirst):
                for s1 in (ifirst, kfirst, jfirst):
                    line = [0, 0, 0]
                    line[axis] = 8
                    for sz in (None, ifirst, kfirst, tuple(line)):
                        z = None if sz is None else E.line(CRD, extent[axis], axis) if sz == tuple(line) else _field(CRD, strides=sz)
                        pair = E.table((_field(FLD, strides=s0), _field(FLD + 0x10000, strides=s1)))
                        rc, msg, launches, path = _call(pair, z, nfields=2, extent=extent, axis=axis, what=ARGMIN)
                        assert rc == 0 and path == _restated_path([s0, s1], sz, extent, axis), (extent, axis, s0, s1, sz, path, msg)
                        seen.add((axis, path))
    assert seen == {(axis, path) for axis in range(3) for path in (L, T, IT)}
    # what the layouts are for
    for axis, want in ((0, T), (1, L), (2, L)):
        assert _call(_field(FLD), axis=axis)[3] == want
    for axis, want in ((0, L), (1, L), (2, T)):
        assert _call(_field(FLD, layout="kfirst"), _field(CRD, layout="kfirst"), axis=axis)[3] == want
    for axis in range(3):  # a coord of another layout than the fields: item by item
        assert _call(_field(FLD), _field(CRD, layout="kfirst"), axis=axis)[3] == IT
    assert _call(_field(FLD), extent=(1, 5, 5), axis=0)[3] == IT  # a line of one point has no run to tile


def test_the_kernels_are_in_the_resource_log_without_scratch():
    kernels = E.kernel_resources(r"line_find\S*kernel")
    # (float, float64) x the register budgets for 1, 4 and 8 entries x (lanes, items, tiles)
    assert len(kernels) == 18 and len({name for name, *_ in kernels}) == 18, kernels
    for name, scratch, waves, lds in kernels:
        assert int(scratch) == 0 and int(waves) >= 2, (name, scratch, waves, lds)
        assert (int(lds) > 0) == ("tile" in name) and int(lds) <= 18 * 1024, (name, lds)


# ---- the Python interface: every refusal before any GPU work ---------------------------------------------------------------
@pytest.mark.parametrize("kwargs, error, match", [
    (dict(level=1.0, halo=2.0), ValueError, "halo must be"),
    (dict(level=1.0, halo=-1), ValueError, "must not be negative"),
    (dict(level=1.0, halo=5), ValueError, "leave no domain"),
    (dict(level=1.0, halo=2, origin=(1, 2, 0)), ValueError, "line_find: field 0: negative origin -1 along axis 0"),
    (dict(level=1.0, origin=(0, 0, 0, 0)), ValueError, "at most three entries"),
    (dict(level=1.0, axis="X"), ValueError, "axis must be"),
    (dict(level=1.0, axis=3), ValueError, "axis must be"),
    (dict(what="first"), ValueError, "what must be one of"),
    (dict(level=1.0, direction="up"), ValueError, "direction must be one of"),
    (dict(what="argmax", level=1.0), ValueError, "a level and a direction go with what='crossing' only, not with what='argmax'"),
    (dict(what="argmin", direction="rising"), ValueError, "go with what='crossing' only, not with what='argmin'"),
    (dict(), ValueError, "what='crossing' needs a level"),
    (dict(level=[1.0, 2.0]), ValueError, "2 levels for 1 field"),
    (dict(level="warm"), ValueError, "could not convert"),
    (dict(what="argmax", axis=1, reverse=True, missing=-1.0), TypeError, "device fields"),
    (dict(level=273.15, axis="I", direction="falling"), TypeError, "device fields"),  # all checks passed: refused for being host memory
])
def test_python_refusals_need_no_gpu(kwargs, error, match):
    field = E.host_field(HOST)
    with pytest.raises(error, match=match):
        linefind.find_lines(field, **kwargs)
    with pytest.raises(error, match=match):
        linefind.LineFind([field], **kwargs)


def test_python_refusals_about_the_fields_themselves():
    import torch

    F = linefind.find_lines
    field, z = E.host_field(HOST), E.host_field(HOST)
    with pytest.raises(ValueError, match="at least one field"):
        F(level=1.0)
    with pytest.raises(ValueError, match="at least one field"):
        linefind.LineFind([], level=1.0)
    with pytest.raises(TypeError, match="host"):
        F(torch.zeros(8, 9, 5, dtype=torch.float64), level=1.0)  # as_device_array's own refusal
    with pytest.raises(TypeError):
        F(field, level=1.0, coord=np.zeros(5))
    with pytest.raises(ValueError, match="takes IJK fields"):
        F(E.host_field((8, 9)), level=1.0)
    with pytest.raises(ValueError, match="coord must be an IJK field or a 1-d array along J"):
        F(field, level=1.0, coord=E.host_field((8, 9)), axis="J")
    with pytest.raises(TypeError, match="share a dtype: float64 and float32 differ"):
        F(field, E.host_field(HOST, dtype="float32"), level=1.0)
    with pytest.raises(TypeError, match="share a dtype: float64 and float32 differ"):
        F(field, level=1.0, coord=E.host_field((5,), "float32"))
    with pytest.raises(TypeError, match="float32 or float64 fields, not int64"):
        F(E.host_field(HOST, dtype="int64"), what="argmax")
    with pytest.raises(ValueError, match="coord has 8 items, a line of 5 points along K needs 5"):
        F(field, level=1.0, coord=E.host_field((8,)))
    with pytest.raises(ValueError, match="share their length along K: 5 and 6 differ"):
        F(field, E.host_field((8, 9, 6)), level=1.0)
    with pytest.raises(TypeError, match="device fields"):
        F(field, E.host_field((9, 11, 5)), what="argmin", coord=E.host_field((5,)))  # along I and J the smaller array sets the domain
    with pytest.raises(TypeError, match="device fields"):
        F(field, level=1.0, coord=field)  # a field as its own coord


def test_a_frozen_search_knows_its_box_its_sections_and_its_levels(monkeypatch):
    """The device check is made to pass for host memory: the call itself is never reached."""
    E.on_device(monkeypatch)
    for count, launches in ((1, 1), (8, 1), (9, 2)):
        fields = [E.host_field((10, 9, 5), "float32") for _ in range(count)]
        z = E.host_field((9,), "float32")
        lf = linefind.LineFind(fields, axis="J", level=[float(k) for k in range(count)], direction="rising", reverse=True, coord=z, missing=-1.0,
                               halo=((1, 1), (0, 0)))
        assert (lf.n, lf.lines, lf.launches, lf.extent, lf.domain, lf.origin, lf.axis, lf.what, lf.path) == \
            (9, 50, launches, (10, 9, 5), (8, 9, 5), (1, 0, 0), 1, "crossing", "lanes")
        assert (lf.direction, lf.reverse, lf.missing, lf.level) == ("rising", True, -1.0, tuple(float(k) for k in range(count)))
        assert lf.result.shape == (count, 3, 5, 10) and lf.result.dtype == np.float64 and not hasattr(lf, "workspace")
    # the sections: (nA, nB) views of the rows, by name and per mode
    for row, name in enumerate(("position", "coord", "crossings")):
        s = lf.section(name, 8)
        assert s.shape == (10, 5) and s.strides == (8, 80) and s.ptr == lf.result.ptr + 8 * 50 * (8 * 3 + row)
    with pytest.raises(ValueError, match="no section 'value': the rows of what='crossing' are position, coord, crossings"):
        lf.section("value")
    with pytest.raises(IndexError, match="entry 9 of 9"):
        lf.section("coord", 9)
    jet = linefind.LineFind(fields[0], axis=2, what="argmax")
    assert jet.path == "tiles" and jet.axis == 2 and jet.level is None  # torch's C order: K is contiguous
    assert jet.section("value").ptr == jet.result.ptr + 8 * 90 * 2 and jet.section("value").shape == (10, 9)
    with pytest.raises(ValueError, match="no section 'crossings': the rows of what='argmax' are position, coord, value"):
        jet.section("crossings")
    with pytest.raises(ValueError, match="a level goes with what='crossing' only"):
        jet.set_level(1.0)
    with pytest.raises(RuntimeError, match="has not been called yet"):
        jet.get()
    # set_level replaces the values that the NEXT call passes, in the same native array: nothing is rebuilt
    before, native = lf._before, lf._level
    lf.set_level(250.0)
    assert lf.level == (250.0,) * 9
    lf.set_level(np.arange(9) + 0.5)
    assert lf.level == tuple(k + 0.5 for k in range(9)) and lf._before is before and lf._level is native and native in before
    with pytest.raises(ValueError, match="3 levels for 9 field"):
        lf.set_level([1.0, 2.0, 3.0])
    assert lf.level == tuple(k + 0.5 for k in range(9))
    # Found: (nA, nB) arrays from a (3, nB, nA) block
    block = np.arange(3 * 2 * 4, dtype=np.float64).reshape(3, 2, 4)
    found = linefind.Found.from_rows(block, "crossing")
    assert found.position.shape == (4, 2) and found.position[3, 1] == block[0, 1, 3] and found.value is None
    assert found.crossings.dtype == np.int64 and found.crossings[2, 0] == int(block[2, 0, 2])
    found = linefind.Found.from_rows(block, "argmin")
    assert found.crossings is None and found.value[1, 1] == block[2, 1, 1] and found.coord[0, 1] == block[1, 1, 0]
    with pytest.raises(ValueError, match=r"\(3, nB, nA\)"):
        linefind.Found.from_rows(block[:2], "argmin")
    del z
    E.refuses_a_dead_array(lf)
