"""Statistics along lines (``gt4mi_line_stats``, ``diagnostics.LineStats``) without a GPU: the two restatements of the documented
order (tests/line_stats_ref.py) against each other and against exact arithmetic, the C entry's declaration, constants, refusals,
dry run and paths, ``Lines`` / ``merge_lines``, the Python refusals, and the kernels' resources."""

import ctypes
import math
import re

import numpy as np
import pytest

import entry_checks as E
import line_stats_ref as R
from entry_checks import INV, OOB, UNS, int64s
from gt4py_amd import _lib, diagnostics

HOST = (8, 9, 3)  # the shape of a host field where a test states none
G = _lib.LINE_STATS_SEGMENT
U = 2.0 ** -53
LENGTHS = [1, 2, 3, 4, 5, G - 1, G, G + 1, 2 * G + 3, 3 * G, 5 * G + 1]
PARAMS = ["const gt4mi_field* fields", "const gt4mi_field* others", "int nfields", "const int64_t domain[3]", "int axis", "int elem_size",
          "void* workspace", "int64_t workspace_bytes", "double* result", "int flags", "void* stream", "int64_t* workspace_needed",
          "int* launches", "int* path"]


def _seeded(rng, shape, dtype, special=True):
    """Numbers over five decades; with ``special`` also NaN, +-inf, +-0.0 and denormals sprinkled in."""
    a = (rng.standard_normal(shape) * 10.0 ** rng.integers(-2, 3, shape)).astype(dtype)
    if special and a.size >= 8:
        flat = a.reshape(-1)
        values = [np.nan, np.inf, -np.inf, 0.0, -0.0, np.finfo(dtype).smallest_subnormal, -3 * np.finfo(dtype).smallest_subnormal]
        for v in values:
            flat[rng.integers(0, flat.size, max(1, flat.size // 40))] = v
    return a


# ---- the reference against itself and against exact arithmetic ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_two_restatements_agree_bit_for_bit(dtype):
    rng = np.random.default_rng(11)
    assert any(len(R.halvings(R.segments(n, G))) > 1 and R.segments(n, G) % 2 for n in LENGTHS)  # a carried value is in the list
    for n in LENGTHS:
        for special in (False, True):
            a, b = _seeded(rng, (n, 3, 2), dtype, special), _seeded(rng, (n, 3, 2), dtype, False)
            w = rng.uniform(0.5, 2.0, (n, 3, 1)).astype(dtype)
            for other in (None, b, w):
                fast, slow = R.lines(a, other, 0, G), R.by_line(a, other, 0, G)
                assert fast.shape == slow.shape == (9, 2, 3) and R.same_bits(fast, slow), (n, dtype, special)
                if not special and other is None:
                    assert not np.isnan(fast).any()
    # the same line along another axis of another box: the same bits
    a = _seeded(rng, (2 * G + 3, 4, 3), dtype)
    want = R.lines(a, None, 0, G)  # [:, k, j]
    assert R.same_bits(R.lines(np.ascontiguousarray(a.transpose(1, 0, 2)), None, 1, G), want)  # a box (j, n, k): [:, k, j] again
    assert R.same_bits(R.lines(np.ascontiguousarray(a.transpose(1, 2, 0)), None, 2, G), want)  # a box (j, k, n): [:, k, j] again
    assert R.same_bits(R.lines(np.ascontiguousarray(a.transpose(2, 0, 1)), None, 1, G), want.transpose(0, 2, 1))  # (k, n, j): [:, j, k]


def test_the_order_is_observable_and_within_the_bound_of_fsum():
    """The reference's sum differs from the left-to-right sum in its last bits on seeded lines (so a test against it tells the
    orders apart), and every sum stays within depth * 2^-53 * sum |term| of math.fsum: the terms are float64 numbers before they
    are added, each passes through at most `depth` additions, the first of them onto +0.0 and exact."""
    rng = np.random.default_rng(12)
    differ = 0
    for n in LENGTHS:
        a, b = _seeded(rng, (n, 5, 1), np.float64, False), rng.uniform(-2, 2, (n, 5, 1))
        depth = R.depth(n, G)
        assert depth == -(-min(n, G) // 4) + 2 + math.ceil(math.log2(R.segments(n, G))) and depth ** 2 < 2 ** 53
        for other in (None, b):
            got = R.lines(a, other, 0, G)[:, 0, :]
            for slot, term in zip((R.SUM, R.SUM_ABS, R.SUM_SQ, R.DOT), R.terms(a, other)):
                if term is None:
                    assert not got[slot].any()
                    continue
                for j in range(5):
                    column = term[:, j, 0]
                    exact, scale = math.fsum(column), math.fsum(np.abs(column))
                    assert abs(got[slot, j] - exact) <= depth * U * scale, (n, slot, j, got[slot, j], exact)
                    left = 0.0
                    for v in column:
                        left = left + float(v)
                    differ += slot == R.SUM and left != got[slot, j]
    assert differ > 0


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_order_free_slots_equal_numpys(dtype):
    rng = np.random.default_rng(13)
    for n in LENGTHS:
        a = _seeded(rng, (4, n, 3), dtype)
        got = R.lines(a, None, 1, G)  # [:, k, i]
        x = a.astype(np.float64).transpose(2, 0, 1)  # [k, i, n]
        assert np.array_equal(got[R.COUNT], np.full((3, 4), n)) and np.array_equal(got[R.NONFINITE], (~np.isfinite(x)).sum(axis=2))
        assert np.array_equal(got[R.MIN], x.min(axis=2), equal_nan=True) and np.array_equal(got[R.MAX], x.max(axis=2), equal_nan=True)
    z = np.zeros((6, 2, 1), dtype)
    z[1::2, 0], z[:, 1] = -0.0, -0.0  # a line of both zeros, a line of -0.0 only
    got = R.lines(z, None, 0, G)[:, 0, :]
    assert np.signbit(got[R.MIN]).tolist() == [True, True] and np.signbit(got[R.MAX]).tolist() == [False, True]
    assert np.signbit(got[R.SUM]).tolist() == [False, False]  # the sums start at +0.0


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
def test_binding_header_and_constants_agree():
    FP, c_int, vp, i64 = ctypes.POINTER(_lib.Field), ctypes.c_int, ctypes.c_void_p, ctypes.c_int64
    E.check_binding("gt4mi_line_stats", PARAMS,
                    argtypes=[FP, FP, c_int, ctypes.POINTER(i64), c_int, c_int, vp, i64, vp, c_int, vp, ctypes.POINTER(i64), ctypes.POINTER(c_int),
                              ctypes.POINTER(c_int)],
                    prefix="LINE_STATS", constants=("MEAN", "ROWS", "PATH_LANES", "PATH_TILES", "PATH_ITEMS"),
                    phrases=("no reference counterpart", "function of n alone", "(A0 (+) A1) (+) (A2 (+) A3)", "new[i] = old[2i] (+) old[2i + 1]",
                             "result[((entry * 9 + row) * nB + b) * nA + a]", "nfields * lines * S * 8 * 8", "2^30 (line, segment) pairs"))
    text = (E.ROOT / "include" / "gt4py_amd.h").read_text()
    define = re.search(r"#ifndef GT4MI_LINE_STATS_SEGMENT\n#define GT4MI_LINE_STATS_SEGMENT (\d+)", text)
    assert define and int(define.group(1)) == G and G % 4 == 0
    assert (_lib.LINE_STATS_MEAN, _lib.LINE_STATS_ROWS) == (8, 9) == (R.MEAN, R.ROWS) and diagnostics.LINE_ROWS[R.MEAN] == "mean"
    # the library was built with the same G: G items are one segment, one more makes two
    for n, segments in ((G, 1), (G + 1, 2)):
        f = ctypes.byref(_lib.Field.make(0x10000, (n, 3, 2), (8, 8 * n, 24 * n), (0, 0, 0)))
        rc, msg, launches, needed, _ = _call(f, domain=(n, 3, 2), workspace=None, result=None)
        assert rc == 0 and needed == 6 * segments * 64 and launches == 1 + (segments > 1), (n, msg, needed)


FIELD = (0x10000, (6, 6, 2), (8, 48, 288), (1, 1, 0))  # a fake device address: no call below reaches the GPU
WORK, RESULT = 0x900000, 0xA00000
NEEDED = 1 * 8 * 1 * 64  # domain (4, 4, 2) along I: 8 lines of one segment


def _field(ptr=FIELD[0], shape=FIELD[1], strides=FIELD[2], origin=FIELD[3]):  # (everything defaults to FIELD)
    return E.field(ptr, shape, strides, origin)


def _call(fields, others=None, nfields=1, domain=(4, 4, 2), axis=0, elem_size=8, workspace=WORK, workspace_bytes=1 << 20, result=RESULT,
          flags=_lib.STATS_DRY_RUN):
    rc, msg, needed, launches, path = E.call("gt4mi_line_stats", fields, others, nfields, int64s(domain), axis, elem_size, workspace,
                                             workspace_bytes, result, flags, None, outs=(ctypes.c_int64(-5), 77, 55))
    return rc, msg, launches, needed, path


def test_argument_errors_of_the_c_entry_without_a_gpu():
    f = ctypes.byref(_field())

    def refused(status, needle, *args, **kwargs):
        kwargs.setdefault("flags", 0)  # a real call: the refusal is what keeps it from the GPU
        rc, msg, launches, _, _ = _call(*args, **kwargs)
        assert rc == status and needle in msg and launches == 0, (rc, msg, launches)

    refused(INV, b"line_stats: fields is null", None)
    refused(INV, b"line_stats: field 0 is null", ctypes.byref(_field(ptr=0)))
    refused(INV, b"line_stats: nfields = 0", f, nfields=0)
    refused(INV, b"line_stats: nfields = -2", f, nfields=-2)
    refused(UNS, b"line_stats: nfields = 65536, more than 65535 fields", f, nfields=65536)
    refused(INV, b"domain is null", f, domain=None)
    refused(INV, b"line_stats: axis 3 is not 0 (I), 1 (J) or 2 (K)", f, axis=3)
    refused(INV, b"line_stats: axis -1 is not", f, axis=-1)
    refused(UNS, b"line_stats: item size 2", f, elem_size=2)
    refused(UNS, b"line_stats: item size 16", f, elem_size=16)
    refused(INV, b"line_stats: empty domain", f, domain=(4, 0, 2))
    refused(INV, b"line_stats: empty domain", f, domain=(0, 4, 2))
    refused(INV, b"invalid domain size -1", f, domain=(4, 4, -1))
    refused(INV, b"line_stats: unknown bits in flags", f, flags=6)
    refused(OOB, b"line_stats: field 0: origin 1 + domain 6 along axis 0 is outside the array", f, domain=(6, 4, 2))
    refused(OOB, b"line_stats: field 0: negative origin", ctypes.byref(_field(origin=(1, -1, 0))))
    refused(UNS, b"line_stats: field 0 is not aligned to its item size", ctypes.byref(_field(ptr=0x10004)))
    refused(UNS, b"byte stride 52 along axis 1 is not a multiple of the item size", ctypes.byref(_field(strides=(8, 52, 312))))
    refused(INV, b"line_stats: field 0 has stride 0 along axis 0", ctypes.byref(_field(strides=(0, 8, 48))))
    other = ctypes.byref(_field(ptr=0x20000))
    refused(UNS, b"line_stats: other 0 is not aligned", f, ctypes.byref(_field(ptr=0x20002)))
    refused(OOB, b"line_stats: other 0: origin 1 + domain 4 along axis 1", f, ctypes.byref(_field(ptr=0x20000, shape=(6, 4, 2))))
    weight = ctypes.byref(_field(ptr=0x20000, shape=(6, 6, 1), strides=(8, 48, 0)))  # IJ against IJK
    for axis in range(3):
        rc, msg, launches, needed, _ = _call(f, weight, axis=axis)
        assert rc == 0 and launches == 1 and needed == 32 // (4, 4, 2)[axis] * 64, msg
    assert _call(f, other)[0] == 0
    # workspace and result
    refused(INV, b"line_stats: workspace is null", f, workspace=None)
    refused(INV, b"line_stats: result is null", f, result=None)
    refused(INV, b"line_stats: workspace of 511 bytes is too small, 512 are needed", f, workspace_bytes=NEEDED - 1)
    refused(INV, b"line_stats: workspace is not aligned to 8 bytes", f, workspace=WORK + 4)
    refused(INV, b"line_stats: result is not aligned to 8 bytes", f, result=RESULT + 4)
    # the domain of FIELD spans bytes [56, 520) of it; the result of one entry and 8 lines is 9 * 8 * 8 = 576 bytes
    refused(INV, b"line_stats: result overlaps field 0", f, result=FIELD[0] + 512)
    refused(INV, b"line_stats: result overlaps field 0", f, result=FIELD[0] + 56 - 568)  # its last double only
    refused(INV, b"line_stats: workspace overlaps field 0", f, workspace=FIELD[0] - NEEDED + 64)
    refused(INV, b"line_stats: workspace overlaps other 0", f, other, workspace=0x20000 + 512)
    refused(INV, b"line_stats: workspace overlaps result", f, result=WORK + 8)
    assert _call(f, result=FIELD[0] + 520)[0] == 0 and _call(f, result=FIELD[0] + 56 - 576)[0] == 0  # next to the domain: fine
    rc, msg, launches, _, _ = _call(f, workspace_bytes=8)  # the dry run refuses a buffer that is passed and too small as well
    assert rc == INV and b"too small" in msg and launches == 0
    # more (line, segment) pairs than the grids count: the limit is named
    big = (2 ** 16, 2 ** 15, 1)
    huge = ctypes.byref(_field(shape=big, strides=(8, 2 ** 19, 2 ** 34), origin=(0, 0, 0)))
    refused(UNS, b"line_stats: 2147483648 lines of 1 segments are more than 2^30 (line, segment) pairs", huge, domain=big, axis=2,
            workspace=None, result=None)
    rc, msg, launches, needed, _ = _call(huge, domain=(2 ** 15, 2 ** 15, 1), axis=2, workspace=None, result=None)
    assert rc == 0 and launches == 1 and needed == 2 ** 30 * 64, msg


def test_dry_run_reports_workspace_and_launches():
    many = E.table(_field(ptr=0x10000 * (n + 1)) for n in range(17))
    for n, want in ((1, 1), (8, 1), (9, 2), (16, 2), (17, 3)):
        rc, msg, launches, needed, _ = _call(many, nfields=n, workspace=None, result=None)  # asking for the size
        assert rc == 0 and launches == want and needed == n * NEEDED, (n, msg)
    for domain in ((1024, 1024, 80), (512, 512, 512), (17, 33, 5), (3, 5 * G + 1, 3), (2 * G + 3, 1, 40), (1, 1, 1)):
        big = ctypes.byref(_field(shape=domain, strides=(8, 8 * domain[0], 8 * domain[0] * domain[1]), origin=(0, 0, 0)))
        for axis in range(3):
            for nfields, passes in ((1, 1), (9, 2)):
                fields = E.table(_field(0x10000 + 0x1000000000 * n, domain, (8, 8 * domain[0], 8 * domain[0] * domain[1]), (0, 0, 0))
                                 for n in range(nfields))
                rc, msg, launches, needed, _ = _call(fields, nfields=nfields, domain=domain, axis=axis, workspace=None, result=None)
                lines, segments = math.prod(domain) // domain[axis], R.segments(domain[axis], G)
                assert rc == 0 and needed == nfields * lines * segments * 8 * 8 and launches == passes + (segments > 1), (domain, axis, msg)


def test_the_path_follows_the_strides():
    L, T, X = _lib.LINE_STATS_PATH_LANES, _lib.LINE_STATS_PATH_TILES, _lib.LINE_STATS_PATH_ITEMS
    assert (L, T, X) == (R.LANES, R.TILES, R.ITEMS)  # the restatement of the rule keeps its own copy
    ni, nj, nk = domain = (8, 6, 5)
    for size in (4, 8):
        layouts = {"I-contiguous": (size, size * ni, size * ni * nj), "J-contiguous": (size * nj, size, size * ni * nj),
                   "K-contiguous": (size * nj * nk, size * nk, size), "padded": (size, size * 64, size * 64 * nj),
                   "every other item": (2 * size, 2 * size * ni, 2 * size * ni * nj)}
        shape = (2 * ni, 64, 2 * nk)
        want = {"I-contiguous": (T, L, L), "J-contiguous": (L, T, L), "K-contiguous": (L, L, T), "padded": (T, L, L), "every other item": (X, X, X)}
        for name, strides in layouts.items():
            for axis in range(3):
                f = ctypes.byref(_field(shape=shape, strides=strides, origin=(0, 0, 0)))
                rc, msg, _, _, path = _call(f, domain=domain, axis=axis, elem_size=size, workspace=None, result=None)
                assert rc == 0 and path == want[name][axis] == R.expected_path([strides], [], domain, axis, size), (name, axis, msg, path)
        # mixed: an I-contiguous and a K-contiguous field share no unit-stride axis
        mixed = E.table((_field(0x10000, shape, layouts["I-contiguous"], (0, 0, 0)), _field(0x4000000, shape, layouts["K-contiguous"], (0, 0, 0))))
        for axis in range(3):
            assert _call(mixed, nfields=2, domain=domain, axis=axis, elem_size=size, workspace=None, result=None)[::4] == (0, X)
        # an IJ weight (K stride 0) beside an I-contiguous field: along K it is broadcast along the line, lanes still run along I
        weight = (size, size * ni, 0)
        pair = ctypes.byref(_field(shape=shape, strides=layouts["I-contiguous"], origin=(0, 0, 0)))
        w = ctypes.byref(_field(ptr=0x4000000, shape=(2 * ni, 64, 1), strides=weight, origin=(0, 0, 0)))
        for axis, path in enumerate((T, L, L)):
            got = _call(pair, w, domain=domain, axis=axis, elem_size=size, workspace=None, result=None)
            assert got[::4] == (0, path) and path == R.expected_path([layouts["I-contiguous"]], [weight], domain, axis, size), (axis, got)
        # nine entries are two launches: only the NINTH has a second field, and that alone breaks unit stride -- the rule looks at
        # every entry of the call, not at the eight of the first launch
        nine = E.table(_field(0x10000 + 0x1000000 * n, shape, layouts["I-contiguous"], (0, 0, 0)) for n in range(9))
        others = (_lib.Field * 9)()  # (data == NULL: no second field)
        others[8] = _field(0x40000000, shape, layouts["every other item"], (0, 0, 0))
        for axis, alone in enumerate((T, L, L)):
            assert _call(nine, nfields=9, domain=domain, axis=axis, elem_size=size, workspace=None, result=None)[::4] == (0, alone)
            got = _call(nine, others, nfields=9, domain=domain, axis=axis, elem_size=size, workspace=None, result=None)
            assert got[::4] == (0, X) and X == R.expected_path([layouts["I-contiguous"]] * 9, [layouts["every other item"]], domain, axis, size), (axis, got)
        # lines of one item, and one lane: extents of 1 select nothing
        one = ctypes.byref(_field(shape=shape, strides=layouts["I-contiguous"], origin=(0, 0, 0)))
        assert _call(one, domain=(1, nj, nk), axis=0, elem_size=size, workspace=None, result=None)[4] == X
        assert _call(one, domain=(1, nj, nk), axis=1, elem_size=size, workspace=None, result=None)[4] == X
        assert _call(one, domain=(ni, 1, 1), axis=0, elem_size=size, workspace=None, result=None)[4] == T


def test_the_kernels_are_in_the_resource_log_and_use_no_scratch():
    """As test_no_shipped_hot_kernel_spills reads the log: every line_stats kernel -- the march kernel and the tile kernels of both
    item types, the finish kernel -- has ScratchSize 0; only the tile kernels use LDS."""
    kernels = {name: (scratch, lds) for name, scratch, _, lds in E.kernel_resources(r"line_stats\S*kernel")}
    kinds = sorted(re.search(r"line_stats_(march|tile|finish)_kernel", name).group(1) for name in kernels)
    assert kinds == ["finish"] + ["march"] * 2 + ["tile"] * 4, sorted(kernels)
    assert all(scratch == 0 for scratch, _ in kernels.values()), kernels
    assert all((lds > 0) == ("tile" in name) for name, (_, lds) in kernels.items()), kernels


# ---- Lines and merge_lines -------------------------------------------------------------------------------------------------------
def _lines_of(a, b=None, axis=0):
    return diagnostics.Lines.from_rows(R.lines(a, b, axis, G))


def test_lines_record():
    rng = np.random.default_rng(14)
    a = _seeded(rng, (9, 3, 2), np.float64, False)
    a[4, 1, 1], a[2, 2, 0] = np.nan, np.inf
    p = _lines_of(a)
    assert p.shape == (3, 2) and p.count.dtype == np.int64 and p.nonfinite.dtype == np.int64 and p.sum.dtype == np.float64
    assert p.count.tolist() == [[9, 9]] * 3 and p.nonfinite.tolist() == [[0, 0], [0, 1], [1, 0]]
    assert p.all_finite.tolist() == [[True, True], [True, False], [False, True]] and p.first_nonfinite == (2, 0)
    assert math.isnan(p.max_abs[1, 1]) and p.max_abs[2, 0] == math.inf and p.max_abs[0, 0] == np.abs(a[:, 0, 0]).max()
    assert p.norm2[0, 1] == math.sqrt(p.sum_sq[0, 1]) and p.mean[0, 0] == p.sum[0, 0] / 9
    s = p[0, 1]
    assert isinstance(s, diagnostics.Stats) and isinstance(s.count, int) and (s.sum, s.min, s.max) == (p.sum[0, 1], a[:, 0, 1].min(), a[:, 0, 1].max())
    assert s.mean == p.mean[0, 1] and math.isnan(p[1, 1].min)
    with pytest.raises(IndexError):
        p[3, 0]
    assert _lines_of(a[:, :1]).first_nonfinite is None and p == _lines_of(a) and p != _lines_of(a[:, ::-1])
    assert "first_nonfinite=(2, 0)" in repr(p)
    with pytest.raises(ValueError, match=r"\(9, nB, nA\)"):
        diagnostics.Lines.from_rows(np.zeros((8, 3, 2)))
    with pytest.raises(ValueError, match="one shape"):
        diagnostics.Lines([[1, 1]], [[0, 0]], [[1.0]], [[1.0]], [[1.0]], [[1.0]], [[1.0]], [[1.0]])


def test_merge_lines_joins_line_by_line_in_the_order_given():
    """Three ranks split the line axis: counts and extremes of the joined parts are those of the whole line, the sums are
    `merge` of the parts' Stats, left to right."""
    rng = np.random.default_rng(15)
    a, b = _seeded(rng, (3 * G + 7, 4, 3), np.float64), _seeded(rng, (3 * G + 7, 4, 3), np.float64, False)
    a[:, 1, 1] = 0.0
    a[5, 1, 1] = -0.0  # a line of zeros whose only -0.0 is in the first part
    cuts = [0, G - 3, 2 * G + 1, 3 * G + 7]
    for other in (None, b):
        whole = _lines_of(a, other)
        parts = [_lines_of(a[lo:hi], None if other is None else other[lo:hi]) for lo, hi in zip(cuts, cuts[1:])]
        merged = diagnostics.merge_lines(parts)
        assert merged.shape == whole.shape == (4, 3)
        for name in ("count", "nonfinite", "min", "max"):
            assert R.same_bits(getattr(merged, name), getattr(whole, name)), name
        assert np.signbit(merged.min[1, 1]) and not np.signbit(merged.max[1, 1])
        for index in np.ndindex(4, 3):
            want = diagnostics.merge([p[index] for p in parts])
            assert R.same_bits(tuple(merged[index]), tuple(want)), index
            with np.errstate(all="ignore"):
                assert R.same_bits(merged.mean[index], np.float64(want.sum) / want.count)
        back = diagnostics.merge_lines(parts[::-1])
        assert R.same_bits(back.min, merged.min) and R.same_bits(back.count, merged.count)
    assert diagnostics.merge_lines(parts[:1]) == parts[0]
    with pytest.raises(ValueError, match="at least one"):
        diagnostics.merge_lines([])
    with pytest.raises(TypeError, match="Lines records"):
        diagnostics.merge_lines([parts[0], parts[0][0, 0]])
    with pytest.raises(ValueError, match=r"shapes \(4, 3\) and \(3, 3\) differ"):
        diagnostics.merge_lines([parts[0], _lines_of(a[:5, :3])])


# ---- the Python interface: every refusal before any GPU work ---------------------------------------------------------------
def test_python_refusals_need_no_gpu():
    D = diagnostics
    with pytest.raises(TypeError, match="axis"):
        D.line_stats(E.host_field(HOST))  # axis has no default
    for axis in ("L", 3, -1, None, True, 1.0):
        with pytest.raises(ValueError, match="axis must be 'I', 'J', 'K' or 0, 1, 2"):
            D.line_stats(E.host_field(HOST), axis=axis)
    with pytest.raises(ValueError, match="at least one field"):
        D.line_stats(axis="I")
    with pytest.raises(TypeError, match="float32 or float64 fields, not int32"):
        D.line_stats(E.host_field(HOST, dtype="int32"), axis="I")
    with pytest.raises(TypeError, match="share a dtype"):
        D.line_stats(E.host_field(HOST), axis="J", other=E.host_field(HOST, dtype="float32"))
    with pytest.raises(ValueError, match="one entry .* per field: 1 for 2 fields"):
        D.LineStats([E.host_field(HOST), E.host_field(HOST)], axis=0, others=[E.host_field(HOST)])
    with pytest.raises(ValueError, match="IJ or IJK fields"):
        D.line_stats(E.host_field((8,)), axis="I")
    with pytest.raises(ValueError, match="leave no domain"):
        D.line_stats(E.host_field(HOST), axis="K", halo=4)
    with pytest.raises(ValueError, match="line_stats: field 0: origin 0 \\+ domain 4 along axis 2 is outside the array"):
        D.line_stats(E.host_field(HOST), axis="I", origin=(0, 0, 0), domain=(8, 9, 4))
    with pytest.raises(ValueError, match="line_stats: empty domain"):
        D.line_stats(E.host_field(HOST), axis=2, domain=(3, 3, 0))
    # all checks passed (an IJ weight against an IJK field, a sub-box, every spelling of the axis): refused for being host memory
    for kwargs in (dict(axis="I"), dict(axis="j", halo=2), dict(axis="K", other=E.host_field((8, 9))), dict(axis=np.int64(1), origin=(1, 1, 1), domain=(2, 2, 2))):
        with pytest.raises(TypeError, match="device fields"):
            D.line_stats(E.host_field(HOST), **kwargs)
    with pytest.raises(TypeError, match="device fields"):
        D.LineStats([E.host_field((8, 9), "float32")], axis="I", halo=((1, 2), (0, 3)))  # Field[IJ]: nk = 1


# ---- what consumes a section: a stencil with a two-dimensional field of each kind ------------------------------------------------
def test_stencils_that_take_a_section_are_generated_and_compiled():
    """out = u - m with m a Field[JK], Field[IK] or Field[IJ] of float64: generated for hip:mi300 and compiled for gfx950 (no GPU
    needed).  The Field[IK] one has no J row of its own in the vector kernel's strips."""
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.gtscript import IJ, IK, JK, PARALLEL, Field, computation, interval  # noqa: F401

    def anomaly_jk(u: Field[np.float64], m: Field[JK, np.float64], out: Field[np.float64]):
        with computation(PARALLEL), interval(...):
            out = u - m

    def anomaly_ik(u: Field[np.float64], m: Field[IK, np.float64], out: Field[np.float64]):
        with computation(PARALLEL), interval(...):
            out = u - m

    def anomaly_ij(u: Field[np.float64], m: Field[IJ, np.float64], out: Field[np.float64]):
        with computation(PARALLEL), interval(...):
            out = u - m

    for definition in (anomaly_jk, anomaly_ik, anomaly_ij):
        program = type(gtscript.stencil(backend="hip:mi300", definition=definition))._gt_program_
        code = _lib.rtc_compile(program.source, f"{definition.__name__}.hip", [])
        assert code[:4] == b"\x7fELF" and all(k.name.encode() in code for k in program.kernels), definition.__name__
