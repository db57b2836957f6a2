"""``gt4py_amd.linefilter`` without a GPU: the contract's restatement (tests/line_filter_ref.py), plain Python against vectorised
numpy and both against ``numpy.fft``, the properties a filter must have, every refusal of the C entry through the dry run (made-up
addresses that are never dereferenced), the declaration, the path rule, the kernels' resources and the Python interface's argument
checks."""

import ctypes
import re

import numpy as np
import pytest

import device_layouts as DL
import entry_checks as E
import line_filter_ref as R
from entry_checks import INV, OOB, UNS, as_arg, int64s
from gt4py_amd import _lib, linefilter

HOST = (8, 9, 5)  # the shape of a host field where a test states none
EPS = 2.0 ** -52
LENGTHS = [2 ** k for k in range(1, 13)]
#: The largest deviation of the restatement from numpy.fft over `_lines` for n = 2 .. 4096, in units of EPS times the scale of the
#: line (max |x| for the filter, max |X| for the spectrum), as measured with this file (every test prints its own): 1.28 (filter),
#: 2.74 (spectrum); against the same bound 2.05 (a response of ones against x itself) and 3.99 (a removed wave, which also holds what
#: the rounding of the wave's own samples puts on other wavenumbers).  The bounds are 4 x the first two: the deviation grows with
#: log n and with the data, a wrong twiddle or stage shows at 1e-1 of the scale and more.
FILTER_BOUND, SPECTRUM_BOUND = 4 * 1.28 * EPS, 4 * 2.74 * EPS


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _lines(rng, n, lines=4, dtype=np.float64):
    """Mixed signs and magnitudes, so that almost every operation rounds."""
    return (rng.uniform(-1, 1, (n, lines)) * 10.0 ** rng.integers(-3, 4, (n, lines))).astype(dtype)


def _response(rng, n, lines=4):
    r = rng.uniform(0, 1, (n // 2 + 1, lines))
    r[rng.uniform(0, 1, r.shape) < 0.2] = 0.0
    return r


def test_the_two_restatements_agree_bit_for_bit():
    rng = np.random.default_rng(1)
    for dtype in (np.float32, np.float64):
        for n in (2, 4, 8, 16, 32, 64):
            x, r = _lines(rng, n, 5, dtype), _response(rng, n, 5)
            x[rng.integers(0, n), 3] = np.nan
            x[rng.integers(0, n), 4] = np.inf
            x[0, 0], x[1, 0] = -0.0, 0.0
            whole = R.filter(x, r)
            re, im = R.spectrum(x)
            assert whole.dtype == dtype and whole.shape == x.shape and re.shape == (n // 2 + 1, 5)
            for l in range(x.shape[1]):
                assert R.same_bits(whole[:, l], R.filter_line(x[:, l], r[:, l])).all(), (dtype, n, l)
                one_re, one_im = R.spectrum_line(x[:, l])
                assert R.same_bits(re[:, l], one_re).all() and R.same_bits(im[:, l], one_im).all(), (dtype, n, l)
            # a NaN or an infinity stays in its line
            assert np.isfinite(whole[:, :3]).all() and np.isnan(whole[:, 3]).all() and not np.isfinite(whole[:, 4]).any()
            # a shared response is the same response on every line
            assert R.same_bits(R.filter(x, r[:, 0]), R.filter(x, np.repeat(r[:, :1], 5, 1))).all()


def test_the_twiddle_table_is_numpys_with_two_entries_set_exactly_and_the_modules_own_is_the_same():
    for n in LENGTHS:
        wr, wi = R.twiddles(n)
        j = np.arange(n // 2)
        assert wr.dtype == np.float64 and len(wr) == len(wi) == n // 2
        assert (wr[0], wi[0]) == (1.0, 0.0) and not np.signbit(wi[0])
        if n >= 4:
            assert (wr[n // 4], wi[n // 4]) == (0.0, -1.0) and not np.signbit(wr[n // 4])
        rest = (j != 0) & (j != n // 4)
        assert np.array_equal(wr[rest], np.cos(2 * np.pi * j / n)[rest]) and np.array_equal(wi[rest], -np.sin(2 * np.pi * j / n)[rest])
        assert np.array_equal(linefilter.twiddles(n).view(np.uint64), np.concatenate([wr, wi]).view(np.uint64))


def test_the_restatement_against_numpy_fft():
    """Filter: irfft(rfft(x) * r, n), the deviation scaled by max |x| of the line; spectrum: rfft(x), scaled by max |X|."""
    rng = np.random.default_rng(2)
    worst_filter = worst_spectrum = 0.0
    for n in LENGTHS:
        x, r = _lines(rng, n), _response(rng, n)
        want = np.fft.irfft(np.fft.rfft(x, axis=0) * r, n, axis=0)
        dev = (np.abs(R.filter(x, r) - want) / np.abs(x).max(axis=0)).max()
        worst_filter = max(worst_filter, dev)
        X = np.fft.rfft(x, axis=0)
        re, im = R.spectrum(x)
        dev_s = (np.abs((re + 1j * im) - X) / np.abs(X).max(axis=0)).max()
        worst_spectrum = max(worst_spectrum, dev_s)
        print(f"n {n}: filter {dev / EPS:.2f} eps, spectrum {dev_s / EPS:.2f} eps")
        assert dev <= FILTER_BOUND and dev_s <= SPECTRUM_BOUND, (n, dev / EPS, dev_s / EPS)
    print(f"worst: filter {worst_filter / EPS:.2f} eps, spectrum {worst_spectrum / EPS:.2f} eps")


def test_a_response_that_keeps_the_mean_alone_gives_one_value_with_the_same_bits():
    rng = np.random.default_rng(3)
    for n in LENGTHS:
        x = _lines(rng, n) + 10.0 ** rng.integers(-1, 3, 4)  # (a mean that is not zero)
        r = np.zeros(n // 2 + 1)
        r[0] = 1.0
        got = R.filter(x, r)
        assert (R.bits(got) == R.bits(got[:1])).all(), n
        assert (np.abs(got[0] - x.mean(axis=0)) <= FILTER_BOUND * np.abs(x).max(axis=0)).all(), n


def test_a_response_of_ones_returns_the_line_within_the_bound_not_bit_for_bit():
    """Every item goes through 2 log2 n roundings: the identity holds to the bound of the filter, and is not exact."""
    rng = np.random.default_rng(4)
    exact = 0
    for n in LENGTHS:
        x = _lines(rng, n)
        got = R.filter(x, np.ones(n // 2 + 1))
        dev = (np.abs(got - x) / np.abs(x).max(axis=0)).max()
        print(f"n {n}: identity {dev / EPS:.2f} eps")
        assert dev <= FILTER_BOUND, (n, dev / EPS)
        exact += int(np.array_equal(got, x))
    assert exact < len(LENGTHS)
    # float32 items of ONE magnitude: the one rounding of the store takes the float64 deviation away
    x = rng.uniform(1, 2, (256, 4)).astype(np.float32)
    assert np.array_equal(R.filter(x, np.ones(129)), x)


def test_a_wave_whose_wavenumber_has_response_zero_is_removed():
    worst = 0.0
    for n in LENGTHS:
        i = np.arange(n)
        for m0 in sorted({0, 1, n // 4, n // 2 - 1, n // 2}):
            # (the phase reduced exactly in integers: 2 pi m0 i / n as one float64 product is off by up to n eps, and what
            # that adds to the line is not at wavenumber m0)
            x = np.cos(2 * np.pi * ((m0 * i) % n) / n)[:, None]
            r = np.ones(n // 2 + 1)
            r[m0] = 0.0
            dev = np.abs(R.filter(x, r)).max()
            worst = max(worst, dev)
            assert dev <= FILTER_BOUND, (n, m0, dev / EPS)
            r = np.zeros(n // 2 + 1)
            r[m0] = 1.0
            assert np.abs(R.filter(x, r) - x).max() <= FILTER_BOUND, (n, m0)
    print(f"worst: a removed wave {worst / EPS:.2f} eps")


def test_power_sums_to_the_mean_square():
    rng = np.random.default_rng(5)
    x = _lines(rng, 64)
    re, im = R.spectrum(x)
    p = R.power((re + 1j * im).T, 64)
    assert np.allclose(p.sum(axis=-1), (x * x).mean(axis=0), rtol=1e-12)


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
PARAMS = ["const gt4mi_field* dst", "const gt4mi_field* src", "int nfields", "const double* response", "const int64_t* response_extent",
          "const double* twiddles", "double* result", "const int64_t extent[3]", "int axis", "int elem_size", "int mode", "int flags",
          "void* stream", "int* path", "int* launches"]


def test_binding_declares_the_header_signature_and_the_abi_is_still_8():
    fp, i64p, c_int, ip, vp = ctypes.POINTER(_lib.Field), ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_void_p
    E.check_binding("gt4mi_line_filter", PARAMS, argtypes=[fp, fp, c_int, vp, i64p, vp, vp, i64p, c_int, c_int, c_int, c_int, vp, ip, ip],
                    prefix="FILTER", constants=("APPLY", "SPECTRUM", "DRY_RUN"),
                    phrases=("u = a - b", "a' = a + b", "b'.re = wr * u.re - wi * u.im", "b'.im = wr * u.im + wi * u.re",
                             "t.re = wr * b.re + wi * b.im", "t.im = wr * b.im - wi * b.re", "response[min(m, n - m)]", "no FMA", "bitrev_L(p)",
                             "w[n/4] = (0, -1)", "1.0 / n", "never evaluates a sine", "mixed radix"))


DST, SRC, RSP, TWD, RES = 0x10_0000, 0x4000_0000, 0x8000_0000, 0x9000_0000, 0xA000_0000  # made-up addresses, far apart
SHAPE = (10, 7, 5)
EXTENT = (8, 5, 5)
APPLY, SPECTRUM = _lib.FILTER_APPLY, _lib.FILTER_SPECTRUM


def _field(ptr, shape=SHAPE, *rest, **kwargs):  # (this file's shape)
    return E.field(ptr, shape, *rest, **kwargs)


def _call(dst, src, nfields=1, extent=EXTENT, axis=0, size=8, mode=APPLY, flags=0, response=RSP, rext=(1, 1), twiddles=TWD, result=None):
    rc, msg, path, launches = E.call("gt4mi_line_filter", as_arg(dst), as_arg(src), nfields, response, int64s(rext), twiddles, result,
                                     int64s(extent), axis, size, mode, flags | _lib.FILTER_DRY_RUN, None, outs=(77, 77))
    return rc, msg, launches, path


def _spectrum(src, **kwargs):
    kwargs.setdefault("result", RES)
    return _call(None, src, mode=SPECTRUM, response=None, rext=None, **kwargs)


def test_every_refusal_of_the_c_entry_without_a_gpu():
    """Every check runs before the first launch: these calls carry made-up device addresses and the dry-run flag."""
    T, LN = _lib.LINE_PATH_TILES, _lib.LINE_PATH_LANES
    rc, msg, launches, path = _call(_field(DST), _field(SRC))
    assert rc == 0 and launches == 1 and path == T, msg
    rc, msg, launches, path = _spectrum(_field(SRC))
    assert rc == 0 and launches == 1 and path == T, msg
    for rext in ((1, 1), (5, 1), (1, 5), (5, 5)):
        rc, msg, *_ = _call(_field(DST), _field(SRC), rext=rext)
        assert rc == 0, msg
    for size in (4, 8):
        rc, msg, *_ = _call(_field(DST, itemsize=size), _field(SRC, itemsize=size), size=size)
        assert rc == 0, msg
    # in a dry run the tables may be missing
    assert _call(_field(DST), _field(SRC), response=None, twiddles=None)[0] == 0
    assert _spectrum(_field(SRC), twiddles=None, result=None)[0] == 0
    # the line length: a power of two from 2 to 4096, and the message names it
    big = (8200, 3, 2)
    for n in (1, 3, 24, 8192):
        rc, msg, launches, path = _call(_field(DST, big, origin=(0, 0, 0)), _field(SRC, big, origin=(0, 0, 0)), extent=(n, 3, 2))
        assert rc == UNS and launches == 0 and path == -1, (n, msg)
        assert b"line_filter: a line of %d points along axis 0: the length must be a power of two from 2 to 4096 (mixed radix is not offered)" % n in msg
        rc, msg, *_ = _spectrum(_field(SRC, big, origin=(0, 0, 0)), extent=(n, 3, 2))
        assert rc == UNS and b"a line of %d points" % n in msg
    rc, msg, *_ = _call(_field(DST), _field(SRC), extent=(8, 5, 3), axis=2)
    assert rc == UNS and b"a line of 3 points along axis 2" in msg
    for n in (2, 4096):
        rc, msg, *_ = _call(_field(DST, big, origin=(0, 0, 0)), _field(SRC, big, origin=(0, 0, 0)), extent=(n, 3, 2))
        assert rc == 0, msg
    # null pointers
    rc, msg, launches, path = _call(None, _field(SRC))
    assert rc == INV and b"line_filter: dst is null" in msg and launches == 0 and path == -1
    rc, msg, *_ = _call(_field(DST), None)
    assert rc == INV and b"line_filter: src is null" in msg
    rc, msg, *_ = _spectrum(None)
    assert rc == INV and b"line_filter: field is null" in msg
    rc, msg, *_ = _call(_field(DST), _field(SRC), extent=None)
    assert rc == INV and b"extent is null" in msg
    rc, msg, *_ = _call(_field(DST), _field(SRC), rext=None)
    assert rc == INV and b"response_extent is null" in msg
    rc, msg, *_ = _call(_field(DST), _field(0))
    assert rc == INV and b"src 0 is null" in msg
    # counts, extents, axis, mode, flags, item size
    for n in (0, -2):
        rc, msg, launches, _ = _call(_field(DST), _field(SRC), nfields=n)
        assert rc == INV and b"nfields" in msg and launches == 0
    rc, msg, *_ = _call(_field(DST), _field(SRC), extent=(8, -1, 5))
    assert rc == INV and b"invalid extent -1 along axis 1" in msg
    for axis in (-1, 3):
        rc, msg, *_ = _call(_field(DST), _field(SRC), axis=axis)
        assert rc == INV and b"axis %d is not 0 (I), 1 (J) or 2 (K)" % axis in msg
    for mode in (-1, 2):
        rc, msg, *_ = _call(_field(DST), _field(SRC), mode=mode)
        assert rc == INV and b"mode %d is not GT4MI_FILTER_APPLY or GT4MI_FILTER_SPECTRUM" % mode in msg
    for flags in (1, 128, 512):
        rc, msg, *_ = _call(_field(DST), _field(SRC), flags=flags)
        assert rc == INV and b"unknown bits in flags" in msg
    for size in (2, 16):
        rc, msg, *_ = _call(_field(DST), _field(SRC), size=size)
        assert rc == UNS and b"item size %d is not supported" % size in msg
    # what goes with which mode
    rc, msg, *_ = _call(_field(DST), _field(SRC), result=RES)
    assert rc == INV and b"a result goes with GT4MI_FILTER_SPECTRUM only" in msg
    rc, msg, *_ = _call(_field(DST), _field(SRC), mode=SPECTRUM, response=None, rext=None, result=RES)
    assert rc == INV and b"a dst goes with GT4MI_FILTER_APPLY only" in msg
    rc, msg, *_ = _call(None, _field(SRC), mode=SPECTRUM, result=RES)
    assert rc == INV and b"a response goes with GT4MI_FILTER_APPLY only" in msg
    # the response's extents: 1 or the box's, along the two other axes in IJK order
    shape = (10, 7, 8)
    for axis, extent, rext, value, bad, box in ((0, EXTENT, (4, 1), 4, 1, 5), (0, EXTENT, (5, 8), 8, 2, 5), (2, (8, 5, 8), (8, 4), 4, 1, 5),
                                                (2, (8, 5, 8), (2, 5), 2, 0, 8), (0, EXTENT, (0, 1), 0, 1, 5)):
        rc, msg, launches, _ = _call(_field(DST, shape), _field(SRC, shape), extent=extent, axis=axis, rext=rext)
        assert rc == INV and b"response extent %d along axis %d is neither 1 nor the box's %d" % (value, bad, box) in msg and launches == 0, msg
    # alignment of the tables
    for kwargs, name in ((dict(response=RSP + 4), b"response"), (dict(twiddles=TWD + 4), b"twiddles")):
        rc, msg, *_ = _call(_field(DST), _field(SRC), **kwargs)
        assert rc == INV and b"line_filter: %s is not aligned to 8 bytes" % name in msg
    rc, msg, *_ = _spectrum(_field(SRC), result=RES + 4)
    assert rc == INV and b"result is not aligned to 8 bytes" in msg
    # a box that does not fit its field; strides and alignment of the fields
    rc, msg, *_ = _call(_field(DST, (8, 7, 5)), _field(SRC))
    assert rc == OOB and b"dst 0: origin 1 + extent 8 along axis 0 is outside the array (shape 8)" in msg
    rc, msg, *_ = _spectrum(_field(SRC, origin=(1, -1, 0)))
    assert rc == OOB and b"field 0: negative origin -1 along axis 1" in msg
    rc, msg, *_ = _call(_field(DST + 4), _field(SRC))
    assert rc == UNS and b"dst 0 is not aligned to its item size" in msg
    rc, msg, *_ = _call(_field(DST, strides=(0, 80, 560)), _field(SRC))
    assert rc == INV and b"dst 0 has stride 0 along axis 0" in msg
    # overlap in memory: a dst against a shifted src, another pair's src, the response, the twiddles, another dst
    rc, msg, launches, _ = _call(_field(DST), _field(DST + 8))
    assert rc == UNS and b"line_filter: dst 0 and src 0 overlap in memory" in msg and launches == 0
    rc, msg, *_ = _call(_field(DST), _field(SRC), response=DST + 160)
    assert rc == UNS and b"dst 0 and response overlap in memory" in msg
    box_lo = DST + 8 + 80  # (the first item of the dst box)
    rc, msg, *_ = _call(_field(DST), _field(SRC), response=box_lo - 5 * 5 * 5 * 8 + 8, rext=(5, 5))  # (a full response ends inside dst)
    assert rc == UNS and b"dst 0 and response overlap in memory" in msg
    rc, msg, *_ = _call(_field(DST), _field(SRC), response=box_lo - 5 * 5 * 5 * 8 + 8)  # (a shared one of 5 items does not reach it)
    assert rc == 0, msg
    rc, msg, *_ = _call(_field(DST), _field(SRC), twiddles=DST + 160)
    assert rc == UNS and b"dst 0 and twiddles overlap in memory" in msg
    two = lambda a, b: E.table((a, b))  # noqa: E731
    rc, msg, *_ = _call(two(_field(DST), _field(DST + 0x10000)), two(_field(SRC), _field(DST)), nfields=2)
    assert rc == UNS and b"dst 0 and src 1 overlap in memory" in msg
    rc, msg, *_ = _call(two(_field(DST), _field(DST + 64)), two(_field(SRC), _field(SRC + 0x10000)), nfields=2)
    assert rc == UNS and b"dst 0 and dst 1 overlap in memory" in msg
    rc, msg, *_ = _spectrum(_field(SRC), result=SRC + 160)
    assert rc == INV and b"result overlaps field 0" in msg
    rc, msg, *_ = _spectrum(_field(SRC), result=TWD + 8)
    assert rc == INV and b"result overlaps twiddles" in msg
    # THE allowed overlap: dst[n] is src[n], the same box; one src for two dsts is fine as well
    rc, msg, launches, _ = _call(_field(DST), _field(DST))
    assert rc == 0 and launches == 1, msg
    rc, msg, *_ = _call(two(_field(DST), _field(DST + 0x10000)), two(_field(SRC), _field(SRC)), nfields=2)
    assert rc == 0, msg
    # an extent with a zero entry along another axis: OK, nothing to launch
    rc, msg, launches, _ = _call(_field(DST), _field(SRC), extent=(8, 0, 5), rext=(1, 1))
    assert rc == 0 and launches == 0, msg


def _restated_path(strides, response_extent, extent, axis, itemsize=8):
    """include/gt4py_amd.h's rule: TILES where the line axis has unit stride in every field and is longer than 1; else LANES where
    another axis has and the response (None: a spectrum) is broadcast along it; else ITEMS."""
    others = [a for a in range(3) if a != axis]

    def unit(ax):
        if any(s[ax] != itemsize for s in strides):
            return False
        return ax == axis or response_extent is None or response_extent[others.index(ax)] == 1

    if unit(axis) and extent[axis] > 1:
        return _lib.LINE_PATH_TILES
    return _lib.LINE_PATH_LANES if any(unit(ax) and extent[ax] > 1 for ax in others) else _lib.LINE_PATH_ITEMS


def test_launches_are_one_per_eight_pairs_and_the_path_follows_the_strides():
    d = E.table(_field(DST + n * 0x10000) for n in range(9))
    s = E.table(_field(SRC + n * 0x10000) for n in range(9))
    assert [_call(d, s, nfields=n)[2] for n in (1, 3, 8, 9)] == [1, 1, 1, 2]
    assert [_spectrum(s, nfields=n)[2] for n in (1, 8, 9)] == [1, 1, 2]
    seen = set()
    for itemsize in (4, 8):
        for extent in ((8, 4, 2), (8, 1, 2), (8, 4, 1), (8, 1, 1), (2, 4, 2)):
            for axis in range(3):
                extent_ax = tuple(int(e) for e in np.roll(extent, axis))  # the line axis holds the power of two
                shape = tuple(e + 2 for e in extent_ax)
                layouts = [tuple(x * itemsize for x in DL.geometry(shape, name, itemsize, 1)[1]) for name in DL.LAYOUTS]
                others = [a for a in range(3) if a != axis]
                for sd in layouts:
                    for ss in layouts:
                        for rext in ((1, 1), (extent_ax[others[0]], 1), (1, extent_ax[others[1]]), (extent_ax[others[0]], extent_ax[others[1]])):
                            rc, msg, _, path = _call(_field(DST, shape, sd, itemsize=itemsize), _field(SRC, shape, ss, itemsize=itemsize),
                                                     extent=extent_ax, axis=axis, size=itemsize, rext=rext)
                            assert rc == 0 and path == _restated_path([sd, ss], rext, extent_ax, axis, itemsize), (extent_ax, axis, sd, ss, rext, path, msg)
                            seen.add((axis, path))
                    rc, msg, _, path = _spectrum(_field(SRC, shape, sd, itemsize=itemsize), extent=extent_ax, axis=axis, size=itemsize)
                    assert rc == 0 and path == _restated_path([sd], None, extent_ax, axis, itemsize), (extent_ax, axis, sd, path, msg)
    assert seen == {(axis, path) for axis in range(3) for path in (_lib.LINE_PATH_LANES, _lib.LINE_PATH_TILES, _lib.LINE_PATH_ITEMS)}
    # what the layouts are for: I-contiguous rows, C order, fields that disagree; the polar filter on K-contiguous fields keeps LANES
    T, LN, IT = _lib.LINE_PATH_TILES, _lib.LINE_PATH_LANES, _lib.LINE_PATH_ITEMS
    shape = (10, 10, 8)
    for axis, want in ((0, T), (1, LN), (2, LN)):
        assert _call(_field(DST, shape), _field(SRC, shape), extent=(8, 8, 8), axis=axis)[3] == want
    for axis, want in ((0, LN), (1, LN), (2, T)):
        assert _call(_field(DST, shape, layout="kfirst"), _field(SRC, shape, layout="kfirst"), extent=(8, 8, 8), axis=axis)[3] == want
        assert _call(_field(DST, shape), _field(SRC, shape, layout="kfirst"), extent=(8, 8, 8), axis=axis)[3] == IT
    assert _call(_field(DST, shape, layout="kfirst"), _field(SRC, shape, layout="kfirst"), extent=(8, 8, 8), axis=0, rext=(8, 1))[3] == LN  # lanes along K, one row per j
    assert _call(_field(DST, shape, layout="kfirst"), _field(SRC, shape, layout="kfirst"), extent=(8, 8, 8), axis=0, rext=(8, 8))[3] == IT
    assert _call(_field(DST, shape, layout="kfirst"), _field(SRC, shape, layout="kfirst"), extent=(8, 8, 8), axis=2, rext=(8, 8))[3] == T


def test_the_kernels_are_in_the_resource_log_without_scratch():
    kernels = E.kernel_resources(r"line_filter_kernel")
    # (float, double) x (a tile of 2048 points beside the twiddles, one line of 4096)
    assert len(kernels) == 4 and len({name for name, *_ in kernels}) == 4, kernels
    assert sorted(int(lds) for *_, lds in kernels) == [48 * 1024, 48 * 1024, 64 * 1024, 64 * 1024]
    for name, scratch, waves, lds in kernels:
        assert int(scratch) == 0 and int(waves) >= 2, (name, scratch, waves, lds)


# ---- the Python interface: every refusal before any GPU work ---------------------------------------------------------------
@pytest.mark.parametrize("kwargs, error, match", [
    (dict(halo=2.0), ValueError, "halo must be"),
    (dict(halo=-1), ValueError, "must not be negative"),
    (dict(axis="X"), ValueError, "axis must be one of"),
    (dict(axis=0), ValueError, "axis must be one of"),
    (dict(axis="J"), TypeError, "line_filter: a line of 9 points along axis 1: the length must be a power of two from 2 to 4096"),
    (dict(axis="K"), TypeError, "a line of 5 points along axis 2"),
    (dict(origin=(2, 0, 0)), TypeError, "a line of 6 points along axis 0"),
    (dict(origin=(0, 0, 0, 0)), ValueError, "at most three entries"),
    (dict(), TypeError, "device fields"),  # all checks passed: refused for being host memory
])
def test_python_refusals_need_no_gpu(kwargs, error, match):
    dst, src = E.host_field((8, 9, 5)), E.host_field((8, 9, 5))
    n = {"J": 9, "K": 5}.get(kwargs.get("axis"), 6 if "origin" in kwargs else 8)
    with pytest.raises(error, match=match):
        linefilter.filter_lines(dst, src, response=E.host_field((n // 2 + 1,)), **kwargs)
    with pytest.raises(error, match=match):
        linefilter.LineFilter([dst], [src], response=E.host_field((n // 2 + 1,)), **kwargs)
    with pytest.raises(error, match=match):
        linefilter.LineSpectrum([src], **kwargs)
    with pytest.raises(error, match=match):
        linefilter.spectrum_lines(src, **kwargs)


def test_python_refusals_about_the_fields_and_the_response():
    F = linefilter.filter_lines
    dst, src, r = E.host_field(HOST), E.host_field(HOST), E.host_field((5,))
    with pytest.raises(ValueError, match="at least one"):
        F([], [], response=r)
    with pytest.raises(ValueError, match="at least one"):
        linefilter.spectrum_lines([])
    with pytest.raises(ValueError, match="2 destination.s. and 1 source.s. were passed"):
        F([dst, E.host_field(HOST)], [src], response=r)
    with pytest.raises(ValueError, match="takes IJK fields"):
        F(E.host_field((8, 9)), src, response=r)
    # one dtype for the fields, float32 or float64
    with pytest.raises(TypeError, match="the fields of one call share a dtype: float64 and float32 differ"):
        F(dst, E.host_field(HOST, dtype="float32"), response=r)
    with pytest.raises(TypeError, match="float32 or float64 fields, not int64"):
        F(E.host_field(HOST, dtype="int64"), E.host_field(HOST, dtype="int64"), response=r)
    # the response: float64, (nh,) or (ea, eb, nh) C-ordered, nh = n // 2 + 1, an extent 1 or the box's
    with pytest.raises(TypeError, match="response must be float64, not float32"):
        F(dst, src, response=E.host_field((5,), "float32"))
    with pytest.raises(TypeError, match="response must be float64, not float32"):
        F(E.host_field(HOST, dtype="float32"), E.host_field(HOST, dtype="float32"), response=E.host_field((5,), "float32"))
    with pytest.raises(ValueError, match=r"response must have shape \(nh,\) or \(ea, eb, nh\), not \(9, 5\)"):
        F(dst, src, response=E.host_field((9, 5)))
    for shape in ((4,), (8,), (9, 5, 4)):
        with pytest.raises(ValueError, match=f"response holds {shape[-1]} wavenumbers, a line of 8 points along I needs n // 2 \\+ 1 = 5"):
            F(dst, src, response=E.host_field(shape))
    with pytest.raises(ValueError, match="response must be C-ordered and dense"):
        F(dst, src, response=E.host_field((9, 5, 10))[:, :, ::2])
    with pytest.raises(ValueError, match="line_filter: response extent 4 along axis 1 is neither 1 nor the box's 9"):
        F(dst, src, response=E.host_field((4, 5, 5)))
    with pytest.raises(ValueError, match="line_filter: response extent 9 along axis 2 is neither 1 nor the box's 5"):
        F(dst, src, response=E.host_field((9, 9, 5)))
    for shape in ((5,), (1, 1, 5), (9, 1, 5), (1, 5, 5), (9, 5, 5)):
        with pytest.raises(TypeError, match="device fields"):
            F(dst, src, response=E.host_field(shape))
    with pytest.raises(ValueError, match="share their length along I: 8 and 16 differ"):
        F(dst, E.host_field((16, 9, 5)), response=r)
    # overlaps come from the library; in place is fine up to the device check
    with pytest.raises(TypeError, match="line_filter: dst 0 and src 1 overlap in memory"):
        F([dst, E.host_field(HOST)], [src, dst], response=r)
    other = E.host_field(HOST)
    with pytest.raises(TypeError, match="line_filter: dst 0 and dst 1 overlap in memory"):
        F([dst, dst], [src, other], response=r)
    with pytest.raises(TypeError, match="line_filter: dst 0 and response overlap in memory"):
        F(dst, src, response=dst[0, 0])
    with pytest.raises(TypeError, match="device fields"):
        F(dst, dst, response=r)
    with pytest.raises(TypeError, match="device fields"):
        linefilter.spectrum_lines(src, other)


def test_frozen_objects_know_their_box_and_refuse_to_run_after_an_array_died(monkeypatch):
    """The weak references are taken last, behind the device check: what they guard is shown on objects whose device check is made
    to pass for host memory -- the call itself is never reached, the dead reference is found first."""
    E.on_device(monkeypatch)
    for count, launches in ((1, 1), (8, 1), (9, 2)):
        dsts, srcs = [E.host_field((10, 16, 5), "float32") for _ in range(count)], [E.host_field((12, 16, 5), "float32") for _ in range(count)]
        r = E.host_field((10, 1, 9))
        lf = linefilter.LineFilter(dsts, srcs, axis="J", response=r, halo=((1, 1), (0, 0)))
        assert (lf.n, lf.lines, lf.launches, lf.extent, lf.domain, lf.origin, lf.axis, lf.path) == \
            (16, 50, launches, (10, 16, 5), (8, 16, 5), (1, 0, 0), "J", "lanes")
        sp = linefilter.LineSpectrum(srcs, axis="J")
        assert (sp.n, sp.lines, sp.launches, sp.extent, sp.path) == (16, 60, launches, (12, 16, 5), "lanes")
        assert sp.result.shape == (count, 2, 12, 5, 9) and sp.coefficients() is sp.result
        with pytest.raises(RuntimeError, match="has not been called yet"):
            sp.get()
    a = E.host_field((8, 18, 5))
    assert linefilter.LineFilter(a, a, axis="I", response=E.host_field((18, 1, 5))).path == "lanes"  # torch's C order: K is contiguous
    assert linefilter.LineFilter(a, a, axis="I", response=E.host_field((18, 5, 5))).path == "items"  # (one response row per line: no lanes across lines)
    assert linefilter.LineFilter(a, a, axis="K", response=E.host_field((8, 18, 3)), origin=(0, 0, 1)).path == "tiles"
    del r
    E.refuses_a_dead_array(lf)
