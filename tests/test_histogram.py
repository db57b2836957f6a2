"""``gt4py_amd.histogram`` without a GPU: the contract's restatement (tests/histogram_ref.py), plain Python against vectorised
numpy and both against ``numpy.histogram``, directed items at every edge, the kernel's guess-and-correct search against the plain
search on adversarial edges, every refusal of the C entry through the dry run (made-up addresses that are never dereferenced), the
declaration, the kernels' resources, the arithmetic of ``Hist`` and the Python interface's argument checks."""

import ctypes
import re

import numpy as np
import pytest

import entry_checks as E
import histogram_ref as R
from entry_checks import INV, OOB, UNS, as_arg, int64s
from gt4py_amd import _lib, histogram

HOST = (8, 9, 5)  # the shape of a host field where a test states none


def _edge_sets():
    rng = np.random.default_rng(7)
    wobble = np.linspace(-3.0, 5.0, 65)
    inner = wobble[1:-1]
    wobble[1:-1] = np.where(rng.integers(0, 2, inner.size) == 0, np.nextafter(inner, -np.inf), np.nextafter(inner, np.inf))
    return {"one bin": np.array([0.0, 1.0]), "two bins": np.array([-1.0, 0.0, 2.5]), "uniform": np.linspace(-2.0, 2.0, 9),
            "log": np.concatenate([[0.0], np.logspace(-3, 2, 12)]), "wobble": wobble}


def _directed(e, dtype):
    """Every edge, its neighbours on both sides in ``dtype``, zeros, infinities, NaN and subnormals."""
    e = e.astype(dtype)
    tiny = np.finfo(dtype).smallest_subnormal
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, tiny, -tiny, np.finfo(dtype).tiny, np.finfo(dtype).max, -np.finfo(dtype).max], dtype=dtype)
    return np.concatenate([e, np.nextafter(e, dtype(-np.inf)), np.nextafter(e, dtype(np.inf)), special])


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def test_the_two_restatements_agree():
    rng = np.random.default_rng(1)
    for name, e in _edge_sets().items():
        for dtype in (np.float32, np.float64):
            x = np.concatenate([_directed(e, dtype), rng.uniform(e[0] - 1, e[-1] + 1, 300).astype(dtype)])
            whole = R.count(x, e)
            assert whole.dtype == np.int64 and whole.shape == (e.size + 2,) and whole.sum() == x.size
            assert np.array_equal(whole, R.count_items(x, e)), (name, dtype)
            assert np.array_equal(R.slots(x, e), [R.slot_of(v, e) for v in x]), (name, dtype)


def test_in_range_finite_items_are_numpy_histogram():
    rng = np.random.default_rng(2)
    for name, e in _edge_sets().items():
        for dtype in (np.float32, np.float64):
            x = rng.uniform(e[0], e[-1], 2000).astype(dtype).astype(np.float64)
            x = np.concatenate([x[(x >= e[0]) & (x <= e[-1])], e])  # (a float32 may round out of range; every edge is an item too)
            got = R.count(x, e)
            assert np.array_equal(got[:-3], np.histogram(x, bins=e)[0]) and not got[-3:].any(), (name, dtype)


def test_directed_items():
    e = np.array([-1.0, 0.0, 0.5, 2.0])
    nb = 3
    both = lambda x: (R.slot_of(x, e), int(R.slots(np.array([x]), e)[0]), R.slot_guess(x, e))  # noqa: E731
    same = lambda x, want: both(x) == (want,) * 3  # noqa: E731
    assert same(-1.0, 0) and same(np.nextafter(-1.0, -2), nb + R.BELOW) and same(np.nextafter(-1.0, 0), 0)
    assert same(0.0, 1) and same(-0.0, 1) and same(np.nextafter(0.0, -1), 0) and same(5e-324, 1) and same(-5e-324, 0)
    assert same(0.5, 2) and same(np.nextafter(0.5, 0), 1)
    assert same(2.0, 2) and same(np.nextafter(2.0, 0), 2) and same(np.nextafter(2.0, 3), nb + R.ABOVE)  # the last bin is closed
    assert same(np.inf, nb + R.ABOVE) and same(-np.inf, nb + R.BELOW) and same(np.nan, nb + R.NAN)
    # a float32 item that rounds ONTO an edge: 0.1 is no float32; the edge float64(float32(0.1)) holds the item, the edge 0.1 does not
    x32 = np.float32(0.1)
    assert float(x32) > 0.1
    assert R.slots(np.array([x32]), np.array([0.0, float(x32), 1.0]))[0] == 1
    assert R.slots(np.array([x32]), np.array([0.0, 0.1, 1.0]))[0] == 1 and R.slots(np.array([0.1]), np.array([0.0, float(x32), 1.0]))[0] == 0
    # the counters of any input sum to its size
    x = _directed(e, np.float32)
    assert R.count(x, e).sum() == x.size and R.count(x, e)[nb + R.NAN] == 1


def test_the_guess_and_correct_search_equals_the_plain_search_on_adversarial_edges():
    rng = np.random.default_rng(3)
    sets = dict(_edge_sets())
    for nb in (1, 2, 4096):
        base = np.linspace(-7.0, 13.0, nb + 1)
        wob = base.copy()
        k = rng.integers(0, 3, nb + 1) - 1
        wob = np.where(k < 0, np.nextafter(base, -np.inf), np.where(k > 0, np.nextafter(base, np.inf), base))
        sets[f"linspace {nb}"], sets[f"ulp {nb}"] = base, wob
        sets[f"log {nb}"] = np.logspace(-8, 8, nb + 1)
    sets["huge"] = np.array([-1.7e308, 0.0, 1.7e308])  # (e[nb] - e[0] overflows: the guess is worthless, the comparisons decide)
    sets["cluster"] = np.concatenate([[0.0], 1.0 + np.arange(30) * 2.0 ** -50, [1e6]])
    for name, e in sets.items():
        assert np.all(np.diff(e) > 0), name
        pick = np.unique(np.concatenate([[0, len(e) - 1], rng.integers(0, len(e), 40)]))
        x = np.concatenate([e[pick], np.nextafter(e[pick], -np.inf), np.nextafter(e[pick], np.inf),
                            (e[0] / 2 + e[-1] / 2) + rng.uniform(-1.0, 1.0, 200) * (e[-1] / 2 - e[0] / 2),
                            [np.nan, np.inf, -np.inf, 0.0, -0.0]])
        want = R.slots(x, e)
        got = np.array([R.slot_guess(v, e) for v in x])
        assert np.array_equal(got, want), (name, x[got != want][:4])
    # any content of the edges buffer terminates with a slot inside the counters
    for junk in (np.array([3.0, 1.0, 2.0, np.nan, -5.0]), np.full(9, np.nan), np.zeros(6), np.array([np.inf, -np.inf, np.inf])):
        for v in (-1.0, 0.0, 1.5, 2.0, np.inf, np.nan):
            assert 0 <= R.slot_guess(v, junk) < len(junk) - 1 + R.EXTRA


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_header_signature_and_the_abi_is_still_8():
    fp, i64p, c_int, ip = ctypes.POINTER(_lib.Field), ctypes.POINTER(ctypes.c_int64), ctypes.c_int, ctypes.POINTER(ctypes.c_int)
    shared = ("x != x", "x < e[0]", "-inf included", "+inf included", "the last bin is closed", "numpy.histogram", "-0.0 == 0.0",
              "weighted histograms", "rows along I or J", "joint")
    E.check_binding("gt4mi_field_histogram",
                    ["const gt4mi_field* fields", "int nfields", "const int64_t extent[3]", "int elem_size", "int nbins", "const double* edges",
                     "const double* edges_host", "int by", "int64_t* result", "int flags", "void* stream", "int* path", "int* launches"],
                    argtypes=[fp, c_int, i64p, c_int, c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), c_int, ctypes.c_void_p, c_int,
                              ctypes.c_void_p, ip, ip],
                    prefix="HISTOGRAM", constants=("MAX_FIELDS", "MAX_BINS", "EXTRA", "BELOW", "ABOVE", "NAN", "WHOLE", "BY_K", "PATH_ROWS",
                                                   "PATH_ITEMS", "ACCUMULATE", "EDGES_PER_FIELD", "DRY_RUN"),
                    phrases=shared + ("x > e[nbins]", "e[b] <= x < e[b+1]", "bounded by a constant", "hipMemsetAsync", "2^31 - 1 items", "49 184"))
    source = (E.ROOT / "gt4py_amd" / "csrc" / "field_histogram.hip.h").read_text()
    for phrase in shared:
        assert phrase in source, phrase
    assert (R.BELOW, R.ABOVE, R.NAN, R.EXTRA) == (_lib.HISTOGRAM_BELOW, _lib.HISTOGRAM_ABOVE, _lib.HISTOGRAM_NAN, _lib.HISTOGRAM_EXTRA)
    assert int(re.search(r"HIST_NUDGE = (\d+)", source).group(1)) == R.NUDGE and int(re.search(r"HIST_BISECT = (\d+)", source).group(1)) == R.BISECT


FLD, EDG, RES = 0x10_0000, 0x4000_0000, 0x8000_0000  # made-up addresses, far apart
SHAPE = (6, 7, 5)
EDGES = object()


def _field(ptr, shape=SHAPE, *rest, **kwargs):  # (this file's shape)
    return E.field(ptr, shape, *rest, **kwargs)


def _call(fields, nfields=1, extent=(4, 5, 5), size=8, nbins=4, edges=EDG, host=EDGES, by=0, result=RES, flags=0, dry=True):
    if host is EDGES:
        sets = max(nfields, 1) if flags & _lib.HISTOGRAM_EDGES_PER_FIELD else 1
        host = np.tile(np.linspace(0.0, 1.0, max(nbins, 1) + 1), sets)
    keep = None if host is None else np.ascontiguousarray(host, dtype=np.float64)
    rc, msg, path, launches = E.call("gt4mi_field_histogram", as_arg(fields), nfields, int64s(extent), size, nbins, edges,
                                     None if keep is None else keep.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), by, result,
                                     flags | (_lib.HISTOGRAM_DRY_RUN if dry else 0), None, outs=(77, 77))
    return rc, msg, launches, path


def test_every_refusal_of_the_c_entry_without_a_gpu():
    """Every check runs before anything is enqueued: these calls carry made-up device addresses and the dry-run flag."""
    ROWS, ITEMS = _lib.HISTOGRAM_PATH_ROWS, _lib.HISTOGRAM_PATH_ITEMS
    for by in (0, 1):
        for flags in (0, _lib.HISTOGRAM_ACCUMULATE, _lib.HISTOGRAM_EDGES_PER_FIELD, 3):
            for edges, result in ((EDG, RES), (None, None)):  # a dry run needs neither device buffer
                rc, msg, launches, path = _call(_field(FLD), by=by, flags=flags, edges=edges, result=result)
                assert rc == 0 and launches == 1 and path == ROWS, msg
    assert _call(_field(FLD, itemsize=4), size=4)[0] == 0
    assert _call(_field(FLD), nbins=_lib.HISTOGRAM_MAX_BINS)[0] == 0 and _call(_field(FLD), nbins=1)[0] == 0
    eight = E.table(_field(FLD + n * 0x10000) for n in range(9))
    assert _call(eight, nfields=8)[:1] == (0,) and _call(eight, nfields=8, flags=_lib.HISTOGRAM_EDGES_PER_FIELD)[0] == 0
    # the paths: ROWS where every field has a unit-stride axis inside a row's box, whichever it is
    kfirst, jfirst = (280, 40, 8), (56, 8, 336)
    assert _call(_field(FLD, strides=kfirst))[3] == ROWS and _call(_field(FLD, strides=jfirst))[3] == ROWS
    assert _call(_field(FLD, strides=kfirst), by=1)[3] == ITEMS and _call(_field(FLD, strides=jfirst), by=1)[3] == ROWS
    assert _call(_field(FLD, strides=(16, 96, 672)))[3] == ITEMS
    assert _call(_field(FLD), extent=(1, 5, 5))[3] == ITEMS and _call(_field(FLD, strides=kfirst), extent=(4, 5, 1))[3] == ITEMS
    pair = E.table((_field(FLD), _field(FLD + 0x10000, strides=(16, 96, 672))))
    assert _call(pair, nfields=2)[3] == ITEMS
    # null pointers
    rc, msg, launches, path = _call(None)
    assert rc == INV and b"field_histogram: fields is null" in msg and launches == 0 and path == -1
    rc, msg, *_ = _call(_field(FLD), extent=None)
    assert rc == INV and b"field_histogram: extent is null" in msg
    rc, msg, launches, _ = _call(_field(0))
    assert rc == INV and b"field_histogram: field 0 is null" in msg and launches == 0
    rc, msg, launches, _ = _call(_field(FLD), host=None)
    assert rc == INV and b"field_histogram: edges_host is null" in msg and launches == 0
    rc, msg, launches, _ = _call(_field(FLD), edges=None, dry=False)  # a real call without its buffers: refused in front of any launch
    assert rc == INV and b"field_histogram: edges is null" in msg and launches == 0
    rc, msg, launches, _ = _call(_field(FLD), result=None, dry=False)
    assert rc == INV and b"field_histogram: result is null" in msg and launches == 0
    # counts, the box, the item size, by, flags
    for n in (0, -2, 9):
        rc, msg, launches, _ = _call(eight, nfields=n)
        assert rc == INV and b"nfields = %d is outside 1 .. 8" % n in msg and launches == 0
    for nb in (0, -1, 4097):
        rc, msg, launches, _ = _call(_field(FLD), nbins=nb)
        assert rc == INV and b"nbins = %d is outside 1 .. 4096" % nb in msg and launches == 0
    for axis in range(3):
        extent = [4, 5, 5]
        extent[axis] = 0
        rc, msg, launches, _ = _call(_field(FLD), extent=extent)
        assert rc == INV and b"empty box (0 along axis %d)" % axis in msg and launches == 0
    rc, msg, *_ = _call(_field(FLD), extent=(4, -1, 5))
    assert rc == INV and b"invalid extent -1 along axis 1" in msg
    rc, msg, *_ = _call(_field(FLD), extent=(4, 2 ** 31, 5))
    assert rc == INV and b"invalid extent 2147483648 along axis 1" in msg
    for size in (2, 16):
        rc, msg, *_ = _call(_field(FLD), size=size)
        assert rc == UNS and b"item size %d is not supported" % size in msg
    for by in (-1, 2):
        rc, msg, *_ = _call(_field(FLD), by=by)
        assert rc == INV and b"by %d is not GT4MI_HISTOGRAM_WHOLE or GT4MI_HISTOGRAM_BY_K" % by in msg
    for flags in (4, 128, 512):
        rc, msg, *_ = _call(_field(FLD), flags=flags)
        assert rc == INV and b"unknown bits in flags" in msg
    # the edges: finite and strictly increasing, the first offending index named, in every set
    good = np.linspace(0.0, 1.0, 5)
    for at, value, what in ((0, np.nan, b"edge 0 of set 0 is not finite"), (4, np.inf, b"edge 4 of set 0 is not finite"),
                            (2, -np.inf, b"edge 2 of set 0 is not finite"), (2, 0.25, b"not strictly increasing at index 2"),
                            (3, 0.1, b"not strictly increasing at index 3"), (1, 0.0, b"not strictly increasing at index 1")):
        bad = good.copy()
        bad[at] = value
        rc, msg, launches, _ = _call(_field(FLD), host=bad)
        assert rc == INV and what in msg and launches == 0, msg
        rc, msg, *_ = _call(pair, nfields=2, host=np.concatenate([good, bad]), flags=_lib.HISTOGRAM_EDGES_PER_FIELD)
        assert rc == INV and what.replace(b"set 0", b"set 1") in msg and b"set 1" in msg, msg
    assert _call(pair, nfields=2, host=np.concatenate([good, good[::-1]]))[0] == 0  # shared edges: the second set is not there
    # a box that does not fit its field; strides and alignment
    for axis, extent in ((0, (6, 5, 5)), (1, (4, 7, 5)), (2, (4, 5, 6))):
        rc, msg, launches, _ = _call(_field(FLD), extent=extent)
        assert rc == OOB and b"field 0" in msg and b"axis %d is outside the array" % axis in msg and launches == 0, msg
    rc, msg, *_ = _call(_field(FLD, origin=(1, -1, 0)))
    assert rc == OOB and b"field 0: negative origin -1 along axis 1" in msg
    rc, msg, *_ = _call(E.table((_field(FLD), _field(FLD + 0x10000, origin=(3, 1, 0)))), nfields=2)
    assert rc == OOB and b"field 1: origin 3 + extent 4 along axis 0 is outside the array (shape 6)" in msg
    rc, msg, *_ = _call(_field(FLD, strides=(8, 52, 336)))
    assert rc == UNS and b"multiple of the item size" in msg
    rc, msg, *_ = _call(_field(FLD + 4))
    assert rc == UNS and b"field 0 is not aligned to its item size" in msg
    rc, msg, launches, _ = _call(_field(FLD, strides=(0, 8, 56)))
    assert rc == INV and b"field 0 has stride 0 along axis 0" in msg and launches == 0
    # edges and result: aligned to 8 bytes; the result clear of every field and of the edges (4 bins: 7 counters per row)
    rc, msg, *_ = _call(_field(FLD), edges=EDG + 4)
    assert rc == INV and b"edges is not aligned to 8 bytes" in msg
    rc, msg, launches, _ = _call(_field(FLD), result=RES + 4)
    assert rc == INV and b"result is not aligned to 8 bytes" in msg and launches == 0
    first = FLD + 8 * (1 + 6)  # the first item of the box
    rc, msg, launches, _ = _call(_field(FLD), result=first)
    assert rc == INV and b"field_histogram: result overlaps field 0" in msg and launches == 0
    assert _call(_field(FLD), result=first - 7 * 8)[0] == 0  # ends in front of it
    rc, msg, *_ = _call(_field(FLD), result=first - 7 * 8 + 8)
    assert rc == INV and b"result overlaps field 0" in msg
    assert _call(_field(FLD), result=first - 5 * 7 * 8)[0] == 0
    rc, msg, *_ = _call(_field(FLD), result=first - 5 * 7 * 8, by=1)  # five rows per level reach into the box
    assert rc == 0 and _call(_field(FLD), result=first - 5 * 7 * 8 + 8, by=1)[0] == INV
    rc, msg, *_ = _call(E.table((_field(FLD), _field(RES))), nfields=2)
    assert rc == INV and b"result overlaps field 1" in msg
    rc, msg, *_ = _call(_field(FLD), edges=RES + 8)
    assert rc == INV and b"result overlaps edges" in msg
    assert _call(_field(FLD), edges=RES + 7 * 8)[0] == 0 and _call(_field(FLD), edges=RES - 5 * 8)[0] == 0
    # more items than an on-chip counter holds
    huge = _lib.Field.make(FLD, (2 ** 11, 2 ** 10, 2 ** 10), (8, 2 ** 14, 2 ** 24), (0, 0, 0))
    rc, msg, launches, _ = _call(huge, extent=(2 ** 11, 2 ** 10, 2 ** 10), result=None)
    assert rc == UNS and b"more than 2^31 - 1 items in the box" in msg and launches == 0


def test_the_kernels_are_in_the_resource_log_without_scratch():
    kernels = E.kernel_resources(r"field_histogram\S*kernel")
    # (float, float64) x (a counter copy per wave up to 1024 bins, one copy up to 4096)
    assert len(kernels) == 4 and len({name for name, *_ in kernels}) == 4, kernels
    source = (E.ROOT / "gt4py_amd" / "csrc" / "field_histogram.hip.h").read_text()
    stated = [int(v.replace(" ", "")) for v in re.findall(r"= (\d\d \d\d\d) bytes", source)]
    assert stated == [24640, 49184]
    for name, scratch, waves, lds in kernels:
        assert int(scratch) == 0 and int(waves) >= 2, (name, scratch, waves, lds)
        limit = stated[0] if "Li1024E" in name else stated[1]
        assert 0 < int(lds) <= limit, (name, lds)
        assert 2 * int(lds) <= 160 * 1024


# ---- Hist ----------------------------------------------------------------------------------------------------------------------
def test_hist_arithmetic_on_hand_made_counts():
    H = histogram.Hist
    h = H([0.0, 1.0, 2.0, 4.0], [2, 0, 2], below=1, above=3, nan=4)
    assert (h.inside, h.total, h.below, h.above, h.nan) == (4, 12, 1, 3, 4)
    assert h.cdf().tolist() == [0.5, 0.5, 1.0]
    assert h.quantile(0.0) == 0.0 and h.quantile(0.25) == 0.5 and h.quantile(0.5) == 1.0 and h.quantile(0.75) == 3.0 and h.quantile(1.0) == 4.0
    assert H([0.0, 1.0, 2.0], [0, 4]).quantile(0.0) == 1.0  # the first bin that holds an item
    assert h.fraction_above(0.0) == 7 / 8 and h.fraction_above(2.0) == 5 / 8 and h.fraction_above(4.0) == 3 / 8
    with pytest.raises(ValueError, match="on an edge"):
        h.fraction_above(3.0)
    with pytest.raises(ValueError, match="between 0 and 1"):
        h.quantile(1.5)
    # empty rows: NaN, not an error
    empty = H([0.0, 1.0, 2.0], [0, 0], nan=2)
    assert empty.inside == 0 and np.isnan(empty.quantile(0.5)) and np.isnan(empty.cdf()).all() and np.isnan(empty.fraction_above(1.0))
    # per level
    p = H([0.0, 1.0, 2.0], [[1, 3], [0, 0], [4, 0]], below=[0, 1, 0], above=[0, 0, 4], nan=[0, 2, 0])
    assert p.inside.tolist() == [4, 0, 4] and p.total.tolist() == [4, 3, 8]
    q = p.quantile(0.5)
    assert q[0] == 1.0 + 1 / 3 and np.isnan(q[1]) and q[2] == 0.5
    assert p.cdf()[0].tolist() == [0.25, 1.0] and np.isnan(p.cdf()[1]).all()
    assert p.fraction_above(1.0).tolist() == [0.75, 0.0, 0.5]
    with pytest.raises(ValueError, match="nb \\+ 1 edges"):
        H([0.0, 1.0], [1, 2])
    with pytest.raises(ValueError, match="one entry per level"):
        H([0.0, 1.0], [[1], [2]], below=[1])
    # from_rows: one block of a result
    block = np.arange(10).reshape(2, 5)
    whole, levels = H.from_rows([0.0, 1.0, 2.0], block[:1], False), H.from_rows([0.0, 1.0, 2.0], block, True)
    assert whole.counts.tolist() == [0, 1] and (whole.below, whole.above, whole.nan) == (2, 3, 4)
    assert levels.counts.tolist() == [[0, 1], [5, 6]] and levels.nan.tolist() == [4, 9]


def test_merge_histograms_is_the_histogram_of_the_concatenation():
    rng = np.random.default_rng(5)
    e = np.linspace(-2.0, 2.0, 17)
    parts = [np.concatenate([rng.standard_normal(n) * 1.5, [np.nan, np.inf, -np.inf, 2.0, -2.0]]) for n in (10, 200, 1, 77)]
    record = lambda x: histogram.Hist.from_rows(e, R.count(x, e)[None], False)  # noqa: E731
    merged, whole = histogram.merge_histograms([record(x) for x in parts]), record(np.concatenate(parts))
    for name in ("counts", "below", "above", "nan", "total"):
        assert np.array_equal(getattr(merged, name), getattr(whole, name)), name
    boxes = [rng.standard_normal((3, 4, 5)) for _ in range(3)]
    level = lambda b: histogram.Hist.from_rows(e, R.count_box(b, e, True), True)  # noqa: E731
    merged = histogram.merge_histograms(level(b) for b in boxes)
    assert np.array_equal(merged.counts, level(np.concatenate(boxes, axis=0)).counts) and merged.counts.shape == (5, 16)
    with pytest.raises(ValueError, match="identical edges"):
        histogram.merge_histograms([record(parts[0]), histogram.Hist(np.nextafter(e, 9), np.zeros(16))])
    with pytest.raises(ValueError, match="identical edges"):
        histogram.merge_histograms([record(parts[0]), histogram.Hist(e[:-1], np.zeros(15))])
    with pytest.raises(ValueError, match="one shape"):
        histogram.merge_histograms([record(parts[0]), level(boxes[0])])
    with pytest.raises(TypeError, match="Hist records"):
        histogram.merge_histograms([record(parts[0]), (1, 2)])
    with pytest.raises(ValueError, match="at least one"):
        histogram.merge_histograms([])


# ---- the Python interface: every refusal before any GPU work ---------------------------------------------------------------
E5 = [0.0, 1.0, 2.0, 3.0, 4.0]


@pytest.mark.parametrize("kwargs, error, match", [
    (dict(edges=E5, halo=2.0), ValueError, "halo must be"),
    (dict(edges=E5, halo=(1, 2.0)), TypeError, "halo widths must be ints"),
    (dict(edges=E5, halo=(1, 2, 3)), ValueError, "halo must be"),
    (dict(edges=E5, halo=-1), ValueError, "must not be negative"),
    (dict(edges=E5, halo=5), ValueError, "leave no domain"),
    (dict(edges=E5, origin=(0, 0, 0, 0)), ValueError, "at most three entries"),
    (dict(edges=E5, origin=(7, 0, 0), domain=(2, 2, 2)), ValueError, "field_histogram: field 0: origin 7 \\+ extent 2 along axis 0 is outside"),
    (dict(edges=E5, by="J"), ValueError, "by must be None \\(the whole box\\) or 'K' \\(per level\\), not 'J'"),
    (dict(edges=E5, by=2), ValueError, "by must be None"),
    (dict(edges=[0.0]), ValueError, "nb \\+ 1 >= 2 numbers"),
    (dict(edges=[[0.0, 1.0], [0.0, 1.0, 2.0]]), ValueError, "all of one length"),
    (dict(edges=[[0.0, 1.0], [0.0, 2.0]]), ValueError, "2 sets for 1 field"),
    (dict(edges="wide"), ValueError, "edges must be"),
    (dict(edges=[0.0, 1.0, 1.0]), ValueError, "field_histogram: the edges of set 0 are not strictly increasing at index 2"),
    (dict(edges=[0.0, np.nan, 1.0]), ValueError, "field_histogram: edge 1 of set 0 is not finite"),
    (dict(edges=np.linspace(0, 1, 4098)), ValueError, "nbins = 4097 is outside 1 .. 4096"),
    (dict(edges=E5, by="K", halo=1), TypeError, "device fields"),  # all checks passed: refused for being host memory
    (dict(edges=[E5], domain=(2, 3, 1), origin=(3, 3, 2)), TypeError, "device fields"),
])
def test_python_refusals_need_no_gpu(kwargs, error, match):
    field = E.host_field(HOST)
    with pytest.raises(error, match=match):
        histogram.histogram(field, **kwargs)
    with pytest.raises(error, match=match):
        histogram.Histogram([field], accumulate=True, **kwargs)


def test_python_refusals_about_the_fields_themselves():
    import torch

    F = histogram.histogram
    field = E.host_field(HOST)
    with pytest.raises(ValueError, match="at least one field"):
        F(edges=E5)
    with pytest.raises(ValueError, match="at least one field"):
        histogram.Histogram([], edges=E5)
    with pytest.raises(TypeError, match="host"):
        F(torch.zeros(8, 9, 5, dtype=torch.float64), edges=E5)  # as_device_array's own refusal
    with pytest.raises(ValueError, match="takes IJ or IJK fields, not a field of 1 dimension"):
        F(E.host_field((8,)), edges=E5)
    with pytest.raises(TypeError, match="share a dtype: float64 and float32 differ"):
        F(field, E.host_field(HOST, dtype="float32"), edges=E5)
    with pytest.raises(TypeError, match="float32 or float64 fields, not int64"):
        F(E.host_field(HOST, dtype="int64"), edges=E5)
    with pytest.raises(ValueError, match="nfields = 9 is outside 1 .. 8"):
        F(*[E.host_field(HOST) for _ in range(9)], edges=E5)
    with pytest.raises(ValueError, match="field 1: origin 0 \\+ extent 9 along axis 1 is outside the array \\(shape 8\\)"):
        F(field, E.host_field((8, 8, 5)), edges=E5)  # the first field sets the box
    with pytest.raises(TypeError, match="device fields"):
        F(E.host_field((8, 9)), edges=E5, by="K")  # IJ: one level
    with pytest.raises(ValueError, match="bins must be a positive int"):
        histogram.Histogram.uniform([field], 0.0, 1.0, 0)
    with pytest.raises(ValueError, match="not strictly increasing"):
        histogram.Histogram.uniform([field], 1.0, 1.0, 4)
    with pytest.raises(TypeError, match="device fields"):
        histogram.Histogram.uniform([field], 0.0, 1.0, 4096, by="K")


def test_a_frozen_histogram_knows_its_box_its_edges_and_its_views(monkeypatch):
    """The device check is made to pass for host memory: the call itself is never reached."""
    import torch

    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    fields = [E.host_field((10, 9, 5), "float32") for _ in range(3)]
    h = histogram.Histogram.uniform(fields, -1.0, 1.0, 8, by="K", accumulate=True, halo=((1, 2), (0, 1)))
    assert (h.bins, h.by, h.accumulate, h.rows, h.origin, h.domain, h.launches, h.path) == (8, "K", True, 5, (1, 0, 0), (7, 8, 5), 1, "items")
    assert np.array_equal(h.edges, np.linspace(-1.0, 1.0, 9)) and h.edges.dtype == np.float64
    assert h.result.shape == (3, 5, 11) and h.result.dtype == np.int64
    assert h._flags == _lib.HISTOGRAM_ACCUMULATE and h._edges_device.dtype == torch.float64 and tuple(h._edges_device.shape) == (9,)
    c = h.counts(2)
    assert c.shape == (5, 8) and c.ptr == h.result.ptr + 8 * 2 * 5 * 11 and c.strides == (88, 8)
    with pytest.raises(IndexError, match="entry 3 of 3"):
        h.counts(3)
    h.result.tensor[:] = 7
    h.reset()
    assert not h.result.tensor.any()
    per = histogram.Histogram(fields[:2], edges=[[0.0, 1.0, 2.0], [0.0, 10.0, 20.0]])
    assert per._flags == _lib.HISTOGRAM_EDGES_PER_FIELD and per.rows == 1 and per.result.shape == (2, 1, 5) and per.counts(1).shape == (2,)
    assert per.counts(1).ptr == per.result.ptr + 8 * 5 and per.path == "rows" and tuple(per._edges_device.shape) == (2, 3)
    # torch's C order is K-contiguous: whole-box calls walk K, per-level calls go item by item
    assert histogram.Histogram(fields[0], edges=E5).path == "rows" and histogram.Histogram(fields[0], edges=E5, by="K").path == "items"
    del fields[1]
    E.refuses_a_dead_array(h)
