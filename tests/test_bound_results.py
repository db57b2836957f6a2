"""What the frozen utility calls WITH RESULTS promise beside their results, class by class, on the CPU: ``get()`` before the first
call, the refusal of an entry index, the order "the library's checks, then the host-array refusal, then the allocations" of the
classes that own buffers, and the two spellings of the one-shot forms.  Every message is pinned whole; none of this needs a device.

The one-shot forms of ``linefind``, ``histogram`` and ``linefilter`` take ``f(a, b)`` or ``f([a, b])``.  Those of ``diagnostics``
take their fields positionally only: to them a list is ONE argument that is no field, refused by ``as_device_array`` with a
``TypeError`` of its own wording -- the type of the host-array refusal, not its message -- and that is pinned as it is."""

import pytest

import entry_checks as E
from gt4py_amd import diagnostics, histogram, linefilter, linefind, linesolve, sampling

SHAPE, LINE = (6, 5, 4), (8, 5, 4)  # LINE: 8 points along I, what a transform takes


def _fields(count=2, shape=SHAPE):
    return [E.host_field(shape) for _ in range(count)]


# ---- get() before the first call; the stream of the last call -------------------------------------------------------------------
RESULT_CLASSES = {
    "FieldStats": lambda: diagnostics.FieldStats(_fields()),
    "LevelStats": lambda: diagnostics.LevelStats(_fields()),
    "LineStats": lambda: diagnostics.LineStats(_fields(), axis="I"),
    "LineFind": lambda: linefind.LineFind(_fields(), axis="K", what="argmax"),
    "LineSpectrum": lambda: linefilter.LineSpectrum(_fields(shape=LINE), axis="I"),
    "Sample": lambda: sampling.Sample(_fields(), pos_i=E.host_field((3,)), pos_j=E.host_field((3,))),
}


@pytest.mark.parametrize("name", sorted(RESULT_CLASSES))
def test_get_before_the_first_call_names_the_class_and_no_stream_is_kept(monkeypatch, name):
    E.on_device(monkeypatch)
    frozen = RESULT_CLASSES[name]()
    assert type(frozen).__name__ == name and frozen._stream is None
    with pytest.raises(RuntimeError) as refusal:
        frozen.get()
    assert str(refusal.value) == f"{name}.get: the object has not been called yet"
    assert frozen._stream is None


# ---- the entry index of a device view -------------------------------------------------------------------------------------------
VIEWS = {  # (the object over two fields, its view of one entry, the noun of the refusal)
    "LevelStats.profile": (lambda: diagnostics.LevelStats(_fields()), lambda o, n: o.profile("mean", n), "entry"),
    "LineStats.section": (lambda: diagnostics.LineStats(_fields(), axis="J"), lambda o, n: o.section("mean", n), "entry"),
    "LineFind.section": (lambda: linefind.LineFind(_fields(), axis="K", what="argmin"), lambda o, n: o.section("position", n), "entry"),
    "Histogram.counts": (lambda: histogram.Histogram(_fields(), edges=[0.0, 1.0, 2.0]), lambda o, n: o.counts(n), "entry"),
    "Sample.column": (lambda: sampling.Sample(_fields(), pos_i=E.host_field((3,)), pos_j=E.host_field((3,))), lambda o, n: o.column(n), "field"),
}


@pytest.mark.parametrize("name", sorted(VIEWS))
def test_an_entry_index_outside_the_call_is_refused_in_these_words(monkeypatch, name):
    E.on_device(monkeypatch)
    build, view, noun = VIEWS[name]
    frozen = build()
    for index in (-1, 2):
        with pytest.raises(IndexError) as refusal:
            view(frozen, index)
        assert str(refusal.value) == f"{noun} {index} of 2"
    assert view(frozen, 0).ptr != view(frozen, 1).ptr  # (the two indices of the call are served)


# ---- the classes that own buffers: the library's checks, the host-array refusal, only then an allocation ---------------------------
def _no_allocation(monkeypatch):
    """From here on ``torch.zeros`` and ``torch.empty`` raise: call it after the fields exist."""
    import torch

    def allocated(*args, **kwargs):
        raise AssertionError("a buffer was allocated for a call that is refused")

    monkeypatch.setattr(torch, "zeros", allocated)
    monkeypatch.setattr(torch, "empty", allocated)


def _line_solve(shape=SHAPE, **kwargs):
    out, rhs = _fields(shape=shape)
    lower, diag, upper = (E.host_field(shape[:1]) for _ in range(3))
    return lambda: linesolve.LineSolve(out, rhs, lower=lower, diag=diag, upper=upper, axis="I", **kwargs)


def _line_filter(shape=LINE, response=None, **kwargs):
    dst, src = _fields(shape=shape)
    r = E.host_field((shape[0] // 2 + 1,) if response is None else response)
    return lambda: linefilter.LineFilter(dst, src, axis="I", response=r, **kwargs)


def _with(fields, build):
    return lambda: build(fields)


OWNERS = {  # every builder makes its fields at once and returns the constructor call: fields first, then _no_allocation, then the call
    "FieldStats": lambda: _with(_fields(), lambda f: diagnostics.FieldStats(f)),
    "LevelStats": lambda: _with(_fields(), lambda f: diagnostics.LevelStats(f)),
    "LineStats": lambda: _with(_fields(), lambda f: diagnostics.LineStats(f, axis="K")),
    "LineFind": lambda: _with(_fields(), lambda f: linefind.LineFind(f, axis="K", level=1.0)),
    "Histogram": lambda: _with(_fields(), lambda f: histogram.Histogram(f, edges=[0.0, 1.0], by="K")),
    "LineSolve": lambda: _line_solve(),
    "LineFilter": lambda: _line_filter(),
    "LineSpectrum": lambda: _with(_fields(shape=LINE), lambda f: linefilter.LineSpectrum(f, axis="I")),
}


@pytest.mark.parametrize("name", sorted(OWNERS))
def test_host_fields_are_refused_before_anything_is_allocated(monkeypatch, name):
    construct = OWNERS[name]()
    _no_allocation(monkeypatch)
    with pytest.raises(TypeError, match="works on device fields"):
        construct()


SIX = (6, 5, 4)  # a line of 6 points along I: no power of two
LIBRARY_REFUSALS = {  # arguments that pass every check of the Python side: (the constructor call, the exception, words of the library's message)
    "FieldStats": (lambda: _with(_fields(), lambda f: diagnostics.FieldStats(f, domain=(7, 5, 4))), ValueError, "field_stats: field 0: origin 0 . domain 7 along axis 0 is outside the array"),
    "LevelStats": (lambda: _with(_fields(), lambda f: diagnostics.LevelStats(f, domain=(6, 5, 5))), ValueError, "level_stats: field 0: origin 0 . domain 5 along axis 2 is outside the array"),
    "LineStats": (lambda: _with(_fields(), lambda f: diagnostics.LineStats(f, axis="I", domain=(6, 6, 4))), ValueError, "line_stats: field 0: origin 0 . domain 6 along axis 1 is outside the array"),
    "LineFind": (lambda: _with(_fields(), lambda f: linefind.LineFind(f, axis="K", what="argmax", origin=(-1, 0, 0))), ValueError, "line_find: field 0: negative origin -1 along axis 0"),
    "Histogram": (lambda: _with(_fields(), lambda f: histogram.Histogram(f, edges=[1.0, 0.0])), ValueError, "field_histogram: the edges of set 0 are not strictly increasing"),
    "LineSolve": (lambda: _line_solve(shape=(2, 5, 4), periodic=True), ValueError, "a periodic line needs at least 3 points"),
    "LineFilter": (lambda: _line_filter(response=(3, 1, 5)), ValueError, "line_filter: response extent 3 along axis 1 is neither 1 nor the box's 5"),
    "LineSpectrum": (lambda: _with(_fields(shape=LINE), lambda f: linefilter.LineSpectrum(f, axis="I", origin=(0, -1, 0))), ValueError,
                     "line_filter: field 0: negative origin -1 along axis 1"),
    # the length of a line is refused as something no kernel handles, which is a TypeError on the Python side
    "LineFilter, 6 points": (lambda: _line_filter(shape=SIX), TypeError, "a line of 6 points along axis 0: the length must be a power of two"),
    "LineSpectrum, 6 points": (lambda: _with(_fields(shape=SIX), lambda f: linefilter.LineSpectrum(f, axis="I")), TypeError,
                               "a line of 6 points along axis 0: the length must be a power of two"),
}


@pytest.mark.parametrize("name", sorted(LIBRARY_REFUSALS))
def test_the_library_refuses_before_the_device_is_asked_for_and_before_anything_is_allocated(monkeypatch, name):
    build, error, words = LIBRARY_REFUSALS[name]
    construct = build()
    _no_allocation(monkeypatch)
    with pytest.raises(error, match=words):  # host memory, and no pretence that it is on the device: the library speaks first
        construct()
    E.on_device(monkeypatch)
    with pytest.raises(error, match=words):  # the same on "device" fields: still nothing was allocated
        construct()


# ---- the one-shot forms ---------------------------------------------------------------------------------------------------------
ONE_SHOTS = {  # (the function, its class, keyword arguments, the shape of its fields, the attribute that holds the native field table)
    "find_lines": (linefind.find_lines, linefind.LineFind, dict(axis="K", what="argmax"), SHAPE, "_fields"),
    "histogram": (histogram.histogram, histogram.Histogram, dict(edges=[0.0, 1.0, 2.0]), SHAPE, "_fields"),
    "spectrum_lines": (linefilter.spectrum_lines, linefilter.LineSpectrum, dict(axis="I"), LINE, "_src"),
    "field_stats": (diagnostics.field_stats, diagnostics.FieldStats, {}, SHAPE, "_fields"),
    "level_stats": (diagnostics.level_stats, diagnostics.LevelStats, {}, SHAPE, "_fields"),
    "line_stats": (diagnostics.line_stats, diagnostics.LineStats, dict(axis="J"), SHAPE, "_fields"),
}
TAKES_A_LIST = ("find_lines", "histogram", "spectrum_lines")


def _what_was_built(frozen, table):
    return (type(frozen), frozen._n, frozen.launches, frozen.origin, frozen.domain, bytes(getattr(frozen, table)), [r() for r in frozen._refs])


@pytest.mark.parametrize("name", sorted(ONE_SHOTS))
def test_both_spellings_of_a_one_shot_reach_the_host_array_refusal(name):
    function, _, kwargs, shape, _ = ONE_SHOTS[name]
    a, b = _fields(shape=shape)
    with pytest.raises(TypeError, match="works on device fields"):
        function(a, b, **kwargs)
    with pytest.raises(TypeError, match="works on device fields" if name in TAKES_A_LIST else "Cannot use list as a device array"):
        function([a, b], **kwargs)


@pytest.mark.parametrize("name", sorted(ONE_SHOTS))
def test_both_spellings_of_a_one_shot_build_the_call_of_the_frozen_class(monkeypatch, name):
    """The call and ``get()`` are replaced: what the one-shot form froze comes back instead of a result."""
    function, frozen_class, kwargs, shape, table = ONE_SHOTS[name]
    E.on_device(monkeypatch)
    called = []
    monkeypatch.setattr(frozen_class, "__call__", lambda self: called.append(self))
    monkeypatch.setattr(frozen_class, "get", lambda self: self)
    a, b = _fields(shape=shape)
    want = _what_was_built(frozen_class([a, b], **kwargs), table)
    assert want[1] == 2 and want[-1][0] is a and want[-1][1] is b
    spellings = [(a, b)] + ([([a, b],), ((a, b),)] if name in TAKES_A_LIST else [])
    for n, fields in enumerate(spellings):
        frozen = function(*fields, **kwargs)
        assert called[n:] == [frozen]  # (frozen, called once, then asked for its result)
        got = _what_was_built(frozen, table)
        assert got[:-1] == want[:-1] and all(x is y for x, y in zip(got[-1], want[-1])) and len(got[-1]) == 2


def test_a_statistics_one_shot_spreads_one_other_field_over_all_fields(monkeypatch):
    E.on_device(monkeypatch)
    monkeypatch.setattr(diagnostics.FieldStats, "__call__", lambda self: None)
    monkeypatch.setattr(diagnostics.FieldStats, "get", lambda self: self)
    a, b = _fields()
    w, v = E.host_field(SHAPE[:2]), E.host_field(SHAPE[:2])
    want = bytes(diagnostics.FieldStats([a, b], others=[w, w])._others)
    assert bytes(diagnostics.field_stats(a, b, other=w)._others) == want != bytes(diagnostics.FieldStats([a, b])._others)
    assert bytes(diagnostics.field_stats(a, b, other=[w, None])._others) == bytes(diagnostics.FieldStats([a, b], others=[w, None])._others)
    assert bytes(diagnostics.field_stats(a, b, other=(v, w))._others) == bytes(diagnostics.FieldStats([a, b], others=[v, w])._others)
