"""``gt4py_amd.linescan`` without a GPU: the contract's restatement (tests/line_scan_ref.py), plain Python against vectorised numpy
and both against ``numpy.cumsum`` (bit for bit) and ``maximum.accumulate`` / ``minimum.accumulate`` (by value: numpy's choice
between signed zeros is not relied on, the contract's own is pinned by directed cases), every refusal of the C entry through the dry
run (made-up addresses that are never dereferenced), the declaration, the kernels' resources and the Python interface's argument
checks."""

import numpy as np
import pytest

import entry_checks as E
import line_scan_ref as R
from entry_checks import INV, OOB, UNS, as_arg, int64s
from gt4py_amd import _lib, linescan

HOST = (8, 9, 5)  # the shape of a host field where a test states none
FLAG_SETS = [(False, False), (True, False), (False, True), (True, True)]  # (exclusive, reverse)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _lines(rng, n, dtype, lines=5):
    """Mixed signs and magnitudes, so that almost every addition rounds."""
    return (rng.uniform(-1, 1, (n, lines)) * 10.0 ** rng.integers(-3, 4, (n, lines))).astype(dtype)


def test_the_two_restatements_agree_bit_for_bit():
    rng = np.random.default_rng(1)
    for dtype in (np.float32, np.float64):
        for n in (1, 2, 3, 17, 40):
            x, w = _lines(rng, n, dtype), _lines(rng, n, dtype)
            x[rng.integers(0, n), 2] = np.nan
            x[rng.integers(0, n), 3] = np.inf
            for exclusive, reverse in FLAG_SETS:
                for op, weight, wide in (("sum", None, False), ("sum", w, False), ("sum", w, True), ("sum", None, True), ("max", None, False),
                                         ("min", None, True)):
                    whole = R.scan(x, op, exclusive, reverse, weight, wide)
                    assert whole.dtype == dtype and whole.shape == x.shape
                    for l in range(x.shape[1]):
                        one = R.scan_line(x[:, l], op, exclusive, reverse, None if weight is None else weight[:, l], wide)
                        assert R.same_bits(whole[:, l], one).all(), (dtype, n, op, exclusive, reverse, wide, l)
            # a 1-d weight is the same weight on every line
            assert R.same_bits(R.scan(x, "sum", weight=w[:, :1]), R.scan(x, "sum", weight=np.repeat(w[:, :1], x.shape[1], 1))).all()


def test_the_sum_is_numpy_cumsum_bit_for_bit():
    rng = np.random.default_rng(2)
    for dtype in (np.float32, np.float64):
        for n in (1, 2, 7, 130, 1000):
            x = _lines(rng, n, dtype)
            assert (R.bits(R.scan(x, "sum")) == R.bits(np.cumsum(x, axis=0))).all(), (dtype, n)
            assert (R.bits(R.scan(x, "sum", reverse=True)) == R.bits(np.cumsum(x[::-1], axis=0)[::-1])).all()
            # along a strided axis of a C-ordered array, and along its contiguous one
            box = _lines(rng, n, dtype, 12).reshape(n, 4, 3)
            for axis in range(3):
                assert (R.bits(R.scan_along(box, axis)) == R.bits(np.cumsum(box, axis=axis))).all(), (dtype, n, axis)
            # exclusive: the inclusive scan moved on by one item behind a +0.0
            ex = R.scan(x, "sum", exclusive=True)
            assert (R.bits(ex[0]) == 0).all() and (R.bits(ex[1:]) == R.bits(np.cumsum(x, axis=0)[:-1])).all()
    x = _lines(rng, 1000, np.float32)
    wide = R.scan(x, "sum", wide=True)
    assert wide.dtype == np.float32 and (R.bits(wide) == R.bits(np.cumsum(x, axis=0, dtype=np.float64).astype(np.float32))).all()
    w = _lines(rng, 1000, np.float32)
    assert (R.bits(R.scan(x, "sum", weight=w)) == R.bits(np.cumsum(x * w, axis=0))).all()
    assert (R.bits(R.scan(x, "sum", weight=w, wide=True)) ==
            R.bits(np.cumsum(x.astype(np.float64) * w.astype(np.float64), axis=0).astype(np.float32))).all()
    x64 = _lines(rng, 100, np.float64)
    assert (R.bits(R.scan(x64, "sum", wide=True)) == R.bits(R.scan(x64, "sum"))).all()  # (no effect on float64)


def test_directed_sums():
    for dtype in (np.float32, np.float64):
        T = dtype
        # a leading -0.0 stays -0.0 (the start is t[0], not 0 + t[0]); the exclusive first item is +0.0
        x = np.array([-0.0, -0.0, 0.0, -0.0], dtype=T)
        for f in (R.scan, R.scan_line):
            got = f(x, "sum")
            assert np.signbit(got).tolist() == [True, True, False, False]
            assert (R.bits(got) == R.bits(np.cumsum(x))).all()
            assert np.signbit(f(x, "sum", exclusive=True)).tolist() == [False, True, True, False]
            assert np.signbit(f(x, "sum", reverse=True)).tolist() == [False, False, False, True]
            # inf + -inf is NaN from there on
            got = f(np.array([1.0, np.inf, 2.0, -np.inf, 3.0], dtype=T), "sum")
            assert got[:3].tolist() == [1.0, np.inf, np.inf] and np.isnan(got[3:]).all()
            # a weight of -0.0 on the first item: the product's sign is kept
            assert np.signbit(f(np.array([1.0, 2.0], dtype=T), "sum", weight=np.array([-0.0, 1.0], dtype=T))).tolist() == [True, False]
    # 4096 ones and 2 ** -20 each: float32 loses every small term, float64 keeps them all until the one rounding of the store
    x = np.full(4096, 1.0 + 2.0 ** -20, dtype=np.float32)
    narrow, wide = R.scan(x[:, None], "sum")[:, 0], R.scan(x[:, None], "sum", wide=True)[:, 0]
    assert (R.bits(narrow) == R.bits(np.cumsum(x))).all()
    assert (R.bits(wide) == R.bits(np.cumsum(x, dtype=np.float64).astype(np.float32))).all()
    assert wide[-1] == np.float32(4096 * (1.0 + 2.0 ** -20)) and narrow[-1] != wide[-1]
    assert (R.bits(R.scan_line(x, "sum", wide=True)) == R.bits(wide)).all()


def test_max_and_min_agree_with_numpy_by_value_and_the_tie_rule_is_the_contracts():
    rng = np.random.default_rng(3)
    for dtype in (np.float32, np.float64):
        for n in (1, 2, 9, 130):
            x = _lines(rng, n, dtype)
            x[rng.integers(0, n, 3), [0, 1, 2]] = [np.nan, np.inf, -np.inf]
            x[rng.integers(0, n, 2), [3, 3]] = [0.0, -0.0]
            for op, acc in (("max", np.maximum), ("min", np.minimum)):
                assert R.same_values(R.scan(x, op), acc.accumulate(x, axis=0)).all(), (dtype, n, op)
                assert R.same_values(R.scan(x, op, reverse=True), acc.accumulate(x[::-1], axis=0)[::-1]).all()
        T = dtype
        pz, nz, nan = T(0.0), T(-0.0), T(np.nan)
        for f in (R.scan, R.scan_line):
            for op in ("max", "min"):
                # on a tie the newer item is taken, signed zeros included
                assert np.signbit(f(np.array([pz, nz], dtype=T), op)).tolist() == [False, True], op
                assert np.signbit(f(np.array([nz, pz], dtype=T), op)).tolist() == [True, False], op
                # a NaN, once met, stays: first, middle and last place
                assert np.isnan(f(np.array([nan, 1, 2], dtype=T), op)).tolist() == [True, True, True]
                assert np.isnan(f(np.array([1, nan, 2], dtype=T), op)).tolist() == [False, True, True]
                assert np.isnan(f(np.array([1, 2, nan], dtype=T), op)).tolist() == [False, False, True]
                assert np.isnan(f(np.array([1, nan, 2], dtype=T), op, reverse=True)).tolist() == [True, True, False]
            # the exclusive first item is the identity, also in front of a NaN
            assert f(np.array([nan, 1], dtype=T), "max", exclusive=True).tolist()[0] == -np.inf
            assert f(np.array([3, 1], dtype=T), "min", exclusive=True).tolist() == [np.inf, 3.0]
            assert f(np.array([3, 1, 2], dtype=T), "max", exclusive=True, reverse=True).tolist() == [2.0, 2.0, -np.inf]
        # a select moves bits: the payload of a NaN comes out as it went in
        payload = np.array([0x7FC0_1234 if dtype == np.float32 else 0x7FF8_0000_0000_1234], dtype=R.bits(np.zeros(1, T)).dtype).view(T)[0]
        for f in (R.scan, R.scan_line):
            got = f(np.array([1, payload, 5], dtype=T), "max", wide=True)  # (wide has no effect on max)
            assert (R.bits(got[1:]) == R.bits(np.array([payload, payload], dtype=T))).all()


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_header_signature_and_the_abi_is_still_8():
    E.check_binding("gt4mi_line_scan",
                  ["const gt4mi_field* dst", "const gt4mi_field* src", "int nfields", "const gt4mi_field* weight", "const int64_t extent[3]",
                   "int axis", "int elem_size", "int op", "int flags", "void* stream", "int* path", "int* launches"],
                  prefix="SCAN", constants=("SUM", "MAX", "MIN", "EXCLUSIVE", "REVERSE", "WIDE", "DRY_RUN", "PATH_LANES", "PATH_TILES", "PATH_ITEMS"),
                  phrases=("s[0] = t[0]", "s[m] = s[m-1] + t[m]", "s[m-1] != s[m-1] or s[m-1] > x[m]", "no FMA", "numpy.cumsum", "in-place", "cupy"))


DST, SRC, WGT = 0x10_0000, 0x4000_0000, 0x8000_0000  # made-up addresses, far apart
SHAPE = (6, 7, 5)
SUM, MAX, MIN = _lib.SCAN_SUM, _lib.SCAN_MAX, _lib.SCAN_MIN


def _field(ptr, shape=SHAPE, *rest, **kwargs):  # (this file's shape)
    return E.field(ptr, shape, *rest, **kwargs)


def _call(dst, src, weight=None, nfields=1, extent=(4, 5, 5), axis=0, size=8, op=SUM, flags=0):
    rc, msg, path, launches = E.call("gt4mi_line_scan", as_arg(dst), as_arg(src), nfields, as_arg(weight), int64s(extent), axis, size, op,
                                   flags | _lib.SCAN_DRY_RUN, None, outs=(77, 77))
    return rc, msg, launches, path


def test_every_refusal_of_the_c_entry_without_a_gpu():
    """Every check runs before the first launch: these calls carry made-up device addresses and the dry-run flag."""
    L, T, IT = _lib.SCAN_PATH_LANES, _lib.SCAN_PATH_TILES, _lib.SCAN_PATH_ITEMS
    for op in (SUM, MAX, MIN):
        for flags in range(8):  # every combination of EXCLUSIVE, REVERSE and WIDE
            rc, msg, launches, path = _call(_field(DST), _field(SRC), op=op, flags=flags)
            assert rc == 0 and launches == 1 and path == T, msg
    rc, msg, launches, path = _call(_field(DST), _field(SRC), _field(WGT))
    assert rc == 0 and launches == 1 and path == T, msg
    for size in (4, 8):
        rc, msg, launches, path = _call(*[_field(p, itemsize=size) for p in (DST, SRC, WGT)], size=size, flags=_lib.SCAN_WIDE)
        assert rc == 0 and launches == 1, msg
    # null pointers
    rc, msg, launches, path = _call(None, _field(SRC))
    assert rc == INV and b"line_scan: dst is null" in msg and launches == 0 and path == -1
    rc, msg, launches, path = _call(_field(DST), None)
    assert rc == INV and b"line_scan: src is null" in msg and launches == 0 and path == -1
    rc, msg, *_ = _call(_field(DST), _field(SRC), extent=None)
    assert rc == INV and b"extent is null" in msg
    for n, what in enumerate((b"dst 0 is null", b"src 0 is null", b"weight 0 is null")):
        args = [_field(DST), _field(SRC), _field(WGT)]
        args[n] = _field(0)
        rc, msg, launches, _ = _call(*args)
        assert rc == INV and what in msg and launches == 0, msg
    # counts, extents, axis, op, flags, item size
    for n in (0, -2):
        rc, msg, launches, _ = _call(_field(DST), _field(SRC), nfields=n)
        assert rc == INV and b"nfields" in msg and launches == 0
    rc, msg, *_ = _call(_field(DST), _field(SRC), extent=(4, -1, 5))
    assert rc == INV and b"invalid extent -1 along axis 1" in msg
    for axis in (-1, 3):
        rc, msg, *_ = _call(_field(DST), _field(SRC), axis=axis)
        assert rc == INV and b"axis %d is not 0 (I), 1 (J) or 2 (K)" % axis in msg
    for op in (-1, 3):
        rc, msg, *_ = _call(_field(DST), _field(SRC), op=op)
        assert rc == INV and b"op %d is not GT4MI_SCAN_SUM, GT4MI_SCAN_MAX or GT4MI_SCAN_MIN" % op in msg
    for flags in (8, 128, 512):
        rc, msg, *_ = _call(_field(DST), _field(SRC), flags=flags)
        assert rc == INV and b"unknown bits in flags" in msg
    for size in (2, 16):
        rc, msg, *_ = _call(_field(DST), _field(SRC), size=size)
        assert rc == UNS and b"item size %d is not supported" % size in msg
    # a weight goes with the sum only
    for op in (MAX, MIN):
        rc, msg, launches, _ = _call(_field(DST), _field(SRC), _field(WGT), op=op)
        assert rc == INV and b"a weight goes with GT4MI_SCAN_SUM only, op is %d" % op in msg and launches == 0
    # a box that does not fit its field, per role and axis
    for n, what in enumerate((b"dst 0", b"src 0", b"weight 0")):
        args = [_field(p, (8, 9, 6)) for p in (DST, SRC, WGT)]
        args[n] = _field(args[n].data, SHAPE)
        for axis, extent in ((0, (6, 5, 5)), (1, (4, 7, 5)), (2, (4, 5, 6))):
            rc, msg, launches, _ = _call(*args, extent=extent)
            assert rc == OOB and what in msg and b"axis %d is outside the array" % axis in msg and launches == 0, msg
    rc, msg, *_ = _call(_field(DST), _field(SRC, origin=(1, -1, 0)))
    assert rc == OOB and b"src 0: negative origin -1 along axis 1" in msg
    rc, msg, *_ = _call(_field(DST, origin=(3, 1, 0)), _field(SRC))
    assert rc == OOB and b"dst 0: origin 3 + extent 4 along axis 0 is outside the array (shape 6)" in msg
    # strides and alignment
    rc, msg, *_ = _call(_field(DST, strides=(8, 52, 336)), _field(SRC))
    assert rc == UNS and b"multiple of the item size" in msg
    rc, msg, *_ = _call(_field(DST), _field(SRC), _field(WGT + 4))
    assert rc == UNS and b"weight 0 is not aligned to its item size" in msg
    rc, msg, launches, _ = _call(_field(DST, strides=(0, 8, 56)), _field(SRC))
    assert rc == INV and b"dst 0 has stride 0 along axis 0 (only a src or the weight may be broadcast)" in msg and launches == 0
    rc, msg, *_ = _call(_field(DST), _field(SRC, strides=(8, 0, 0)))
    assert rc == 0, msg  # a src may be broadcast
    # a 1-d weight along the line axis: broadcast, exempt from the shape check on the other axes, n items needed
    for axis in range(3):
        n = (4, 5, 5)[axis]
        rc, msg, launches, _ = _call(_field(DST), _field(SRC), E.line(WGT, n, axis), axis=axis)
        assert rc == 0 and launches == 1, msg
        rc, msg, *_ = _call(_field(DST), _field(SRC), E.line(WGT, n - 1, axis), axis=axis)
        assert rc == OOB and b"weight 0" in msg and b"axis %d" % axis in msg, msg
    rc, msg, *_ = _call(_field(DST), _field(SRC), E.line(WGT, 5, 1), axis=0)  # 1-d along the wrong axis
    assert rc == OOB and b"weight 0" in msg
    # overlap in memory: a dst against a shifted src, another pair's src, the weight, another dst
    rc, msg, launches, _ = _call(_field(DST), _field(DST + 8))
    assert rc == UNS and b"line_scan: dst 0 and src 0 overlap in memory" in msg and launches == 0
    rc, msg, *_ = _call(_field(DST), _field(DST, (6, 7, 5), (8, 56, 336)))  # the same start, another pitch
    assert rc == UNS and b"dst 0 and src 0 overlap in memory" in msg
    rc, msg, *_ = _call(_field(DST), _field(SRC), _field(DST))
    assert rc == UNS and b"dst 0 and weight overlap in memory" in msg
    rc, msg, *_ = _call(_field(DST), _field(SRC), E.line(DST + 80, 4, 0))
    assert rc == UNS and b"dst 0 and weight overlap in memory" in msg
    two = lambda a, b: E.table((a, b))  # noqa: E731
    rc, msg, *_ = _call(two(_field(DST), _field(DST + 0x10000)), two(_field(SRC), _field(DST)), nfields=2)
    assert rc == UNS and b"dst 0 and src 1 overlap in memory" in msg
    rc, msg, *_ = _call(two(_field(DST), _field(DST + 64)), two(_field(SRC), _field(SRC + 0x10000)), nfields=2)
    assert rc == UNS and b"dst 0 and dst 1 overlap in memory" in msg
    rc, msg, *_ = _call(two(_field(DST), _field(DST)), two(_field(DST), _field(DST)), nfields=2)
    assert rc == UNS and b"overlap in memory" in msg  # in place twice over one array
    # THE allowed overlap: dst[n] is src[n], the same box; one src for two dsts and the src as its own weight are fine as well
    rc, msg, launches, _ = _call(_field(DST), _field(DST))
    assert rc == 0 and launches == 1, msg
    rc, msg, *_ = _call(two(_field(DST), _field(DST + 0x10000)), two(_field(DST), _field(DST + 0x10000)), _field(WGT), nfields=2)
    assert rc == 0, msg
    rc, msg, *_ = _call(two(_field(DST), _field(DST + 0x10000)), two(_field(SRC), _field(SRC)), nfields=2)
    assert rc == 0, msg
    rc, msg, *_ = _call(_field(DST), _field(SRC), _field(SRC))
    assert rc == 0, msg
    # an extent with a zero entry: OK, nothing to launch -- after the checks
    rc, msg, launches, _ = _call(_field(DST), _field(SRC), extent=(4, 0, 5))
    assert rc == 0 and launches == 0, msg
    rc, msg, launches, _ = _call(_field(DST), _field(SRC), extent=(7, 0, 5))
    assert rc == OOB and launches == 0


def _restated_path(strides, weight_strides, extent, axis, itemsize=8):
    """include/gt4py_amd.h's rule: TILES where the line axis has unit stride in every field and is longer than 1; else LANES where
    another axis has (the weight may be broadcast along it); else ITEMS."""
    def unit(ax):
        if any(s[ax] != itemsize for s in strides):
            return False
        return weight_strides is None or weight_strides[ax] == itemsize or (ax != axis and weight_strides[ax] == 0)

    if unit(axis) and extent[axis] > 1:
        return _lib.SCAN_PATH_TILES
    return _lib.SCAN_PATH_LANES if any(unit(ax) and extent[ax] > 1 for ax in range(3) if ax != axis) else _lib.SCAN_PATH_ITEMS


def test_launches_are_one_per_eight_pairs_and_the_path_follows_the_strides():
    d = E.table(_field(DST + n * 0x10000) for n in range(9))
    s = E.table(_field(SRC + n * 0x10000) for n in range(9))
    assert [_call(d, s, nfields=n)[2] for n in (1, 3, 8, 9)] == [1, 1, 1, 2]
    L, T, IT = _lib.SCAN_PATH_LANES, _lib.SCAN_PATH_TILES, _lib.SCAN_PATH_ITEMS
    ifirst, kfirst, jfirst = (8, 48, 336), (280, 40, 8), (56, 8, 336)
    seen = set()
    for extent in ((4, 5, 5), (1, 5, 5), (4, 1, 5), (4, 5, 1), (1, 1, 5), (4, 1, 1)):
        for axis in range(3):
            for sd in (ifirst, kfirst, jfirst):
                for ss in (ifirst, kfirst, jfirst):
                    line = [0, 0, 0]
                    line[axis] = 8
                    for sw in (None, ifirst, kfirst, tuple(line)):
                        w = None if sw is None else E.line(WGT, extent[axis], axis) if sw == tuple(line) else _field(WGT, strides=sw)
                        rc, msg, launches, path = _call(_field(DST, strides=sd), _field(SRC, strides=ss), w, extent=extent, axis=axis)
                        assert rc == 0 and path == _restated_path([sd, ss], sw, extent, axis), (extent, axis, sd, ss, sw, path, msg)
                        seen.add((axis, path))
    assert seen == {(axis, path) for axis in range(3) for path in (L, T, IT)}
    # what the layouts are for
    for axis, want in ((0, T), (1, L), (2, L)):
        assert _call(_field(DST), _field(SRC), axis=axis)[3] == want
    for axis, want in ((0, L), (1, L), (2, T)):
        assert _call(_field(DST, layout="kfirst"), _field(SRC, layout="kfirst"), _field(WGT, layout="kfirst"), axis=axis)[3] == want
    for axis in range(3):  # fields that disagree: item by item
        assert _call(_field(DST), _field(SRC, layout="kfirst"), axis=axis)[3] == IT
        assert _call(_field(DST), _field(SRC), _field(WGT, layout="kfirst"), axis=axis)[3] == IT
    assert _call(_field(DST), _field(SRC), extent=(1, 5, 5), axis=0)[3] == IT  # a line of one point has no run to tile


def test_the_kernels_are_in_the_resource_log_without_scratch():
    kernels = E.kernel_resources(r"line_scan\S*kernel")
    # (float, float64, float accumulated in float64) x the register budgets for 1, 4 and 8 entries x (lanes, items, tiles)
    assert len(kernels) == 27 and len({name for name, *_ in kernels}) == 27, kernels
    for name, scratch, waves, lds in kernels:
        assert int(scratch) == 0 and int(waves) >= 2, (name, scratch, waves, lds)
        assert (int(lds) > 0) == ("tile" in name) and int(lds) <= 18 * 1024, (name, lds)


# ---- the Python interface: every refusal before any GPU work ---------------------------------------------------------------
@pytest.mark.parametrize("kwargs, error, match", [
    (dict(halo=2.0), ValueError, "halo must be"),
    (dict(halo=-1), ValueError, "must not be negative"),
    (dict(halo=5), ValueError, "leave no domain"),
    (dict(halo=2, origin=(1, 2, 0)), ValueError, "line_scan: dst 0: negative origin -1 along axis 0"),
    (dict(origin=(0, 0, 0, 0)), ValueError, "at most three entries"),
    (dict(origin=(0, 0, 5)), ValueError, "leave no domain"),
    (dict(axis="X"), ValueError, "axis must be one of"),
    (dict(axis=0), ValueError, "axis must be one of"),
    (dict(op="prod"), ValueError, "op must be one of"),
    (dict(op=0), ValueError, "op must be one of"),
    (dict(op="max", weight=None, exclusive=True, reverse=True, wide=True), TypeError, "device fields"),
    (dict(), TypeError, "device fields"),  # all checks passed: refused for being host memory
])
def test_python_refusals_need_no_gpu(kwargs, error, match):
    dst, src = E.host_field(HOST), E.host_field(HOST)
    with pytest.raises(error, match=match):
        linescan.scan_lines(dst, src, **kwargs)
    with pytest.raises(error, match=match):
        linescan.LineScan([dst], [src], **kwargs)


def test_python_refusals_about_the_fields_themselves():
    import torch

    S = linescan.scan_lines
    dst, src, w = E.host_field(HOST), E.host_field(HOST), E.host_field(HOST)
    with pytest.raises(ValueError, match="at least one"):
        S([], [])
    with pytest.raises(ValueError, match="2 destination.s. and 1 source.s. were passed"):
        S([dst, E.host_field(HOST)], [src])
    with pytest.raises(TypeError, match="host"):
        S(torch.zeros(8, 9, 5, dtype=torch.float64), src)  # as_device_array's own refusal
    with pytest.raises(TypeError):
        S(dst, np.zeros((8, 9, 5)))
    with pytest.raises(TypeError):
        S(dst, src, weight=np.zeros(8))
    with pytest.raises(ValueError, match="takes IJK fields"):
        S(E.host_field((8, 9)), src)
    with pytest.raises(ValueError, match="weight must be an IJK field or a 1-d array along J"):
        S(dst, src, weight=E.host_field((8, 9)), axis="J")
    # a weight goes with the sum
    for op in ("max", "min"):
        with pytest.raises(ValueError, match=f"a weight goes with op='sum' only, not with op='{op}'"):
            S(dst, src, weight=w, op=op)
    # one dtype for everything, float32 or float64
    with pytest.raises(TypeError, match="share a dtype: float64 and float32 differ"):
        S(dst, E.host_field(HOST, dtype="float32"))
    with pytest.raises(TypeError, match="share a dtype: float64 and float32 differ"):
        S(dst, src, weight=E.host_field((8,), "float32"))
    with pytest.raises(TypeError, match="float32 or float64 fields, not int64"):
        S(E.host_field(HOST, dtype="int64"), E.host_field(HOST, dtype="int64"))
    # the weight's shape: a 1-d array holds exactly n items along the line axis; IJK arrays agree along it
    with pytest.raises(TypeError, match="device fields"):
        S(dst, src, weight=E.host_field((8,)))
    with pytest.raises(ValueError, match="weight has 8 items, a line of 9 points along J needs 9"):
        S(dst, src, weight=E.host_field((8,)), axis="J")
    with pytest.raises(ValueError, match="weight has 8 items, a line of 10 points along I needs 10"):
        S(E.host_field((10, 9, 5)), E.host_field((10, 9, 5)), weight=E.host_field((8,)), halo=1)
    with pytest.raises(ValueError, match="share their length along I: 8 and 10 differ"):
        S(dst, E.host_field((10, 9, 5)))
    with pytest.raises(TypeError, match="device fields"):  # along J and K the smaller array sets the domain
        S(dst, E.host_field((8, 11, 6)))
    # an origin or a box outside a shape (the library's words)
    with pytest.raises(ValueError, match="leave no domain"):
        S(dst, src, origin=(9, 0, 0))
    with pytest.raises(ValueError, match="line_scan: dst 0: negative origin -1 along axis 1"):
        S(dst, src, halo=((0, 0), (1, 0)), origin=(0, 0, 0))
    # overlaps come from the library; in place is fine up to the device check
    with pytest.raises(TypeError, match="line_scan: dst 0 and weight overlap in memory"):
        S(dst, src, weight=dst)
    with pytest.raises(TypeError, match="line_scan: dst 0 and src 1 overlap in memory"):
        S([dst, E.host_field(HOST)], [src, dst])
    other = E.host_field(HOST)
    with pytest.raises(TypeError, match="line_scan: dst 0 and dst 1 overlap in memory"):
        S([dst, dst], [src, other])
    with pytest.raises(TypeError, match="device fields"):
        S(dst, dst)
    with pytest.raises(TypeError, match="device fields"):
        S([dst, other], [dst, other], weight=w)


def test_a_frozen_scan_knows_its_box_and_refuses_to_run_after_an_array_died(monkeypatch):
    """The weak references are taken last, behind the device check: what they guard is shown on a LineScan whose device check
    is made to pass for host memory -- the call itself is never reached, the dead reference is found first."""
    E.on_device(monkeypatch)
    for count, launches in ((1, 1), (8, 1), (9, 2)):
        dsts, srcs = [E.host_field((10, 9, 5), "float32") for _ in range(count)], [E.host_field((12, 9, 5), "float32") for _ in range(count)]
        w = E.host_field((9,), "float32")
        sc = linescan.LineScan(dsts, srcs, axis="J", weight=w, wide=True, exclusive=True, halo=1)
        assert (sc.n, sc.lines, sc.launches, sc.extent, sc.domain, sc.origin, sc.axis, sc.op, sc.path) == \
            (9, 50, launches, (10, 9, 5), (8, 7, 5), (1, 1, 0), "J", "sum", "lanes")
        assert (sc.exclusive, sc.reverse, sc.wide) == (True, False, True) and not hasattr(sc, "workspace")
    assert linescan.LineScan(dsts[0], dsts[0], axis="K", op="min", reverse=True).path == "tiles"  # torch's C order: K is contiguous
    del w
    E.refuses_a_dead_array(sc)
