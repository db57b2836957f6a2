"""Every frozen utility call captured ONCE in a hipGraph (one stream, no parallel branches) and replayed, against the eager call:
the protocol of tests/graph_replay.py.  Per case: eager on image A against the class's numpy restatement, with the comparator of
the class's own GPU file (``Dev.assert_box`` over every byte of every written buffer, or that file's ``same_bits``; counters as
integers) -- no tolerance appears here because none of those files has one; a capture that enqueues nothing; a replay on image B
(NaN and infinities where the utility defines a result for them) against the restatement and, bit for bit over every written
byte, against an eager call on the same buffers; replays on C and on A again, the last one the bits of the first eager call;
``get()`` straight after a replay, on the default stream and on a side stream.  Shapes are those of the classes' own files: one
case per kernel path the object reports, and one that needs more than one launch per call (a graph of several nodes).

Then ONE composed model step -- halo fill, the kernel library's Laplacian, a line solve along K, a copy back into the state, field and
level statistics, a histogram by level, a first crossing along K and a stencil that reads the crossing's position as ``Field[IJ]`` --
captured once and replayed three times against three eager steps, bit for bit, and against the numpy chain of
tests/graph_step_ref.py (tests/test_graph_step_ref.py checks that chain on the CPU).

``LineFilter`` / ``LineSpectrum`` refuse a line that is not a power of two, so their cases are two powers of two along I and
along K.  ``Upload`` / ``Download`` stage through pinned host memory with events and are not meant for capture.

Wall time of this file on one MI355X: 5 s (122 tests)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import graph_replay as C  # noqa: E402
import graph_step_ref as S  # noqa: E402
import level_stats_ref  # noqa: E402
import stats_ref  # noqa: E402
import line_stats_ref  # noqa: E402
import transfer_ref  # noqa: E402
from gt4py_amd import _lib  # noqa: E402
from gt4py_amd.cartesian.gtscript import IJ, PARALLEL, Field, computation, interval  # noqa: E402, F401

LANES, TILES, ITEMS = "lanes", "tiles", "items"
I, J, K = 0, 1, 2
#: 8 entries, fields or pairs go into one launch (STATS_MAX_ENTRIES, HALO_FILL_MAX_FIELDS, FIELD_COPY_MAX_PAIRS, PAIR_MAX_FIELDS in csrc/)
MORE_THAN_ONE_LAUNCH = 9
G = _lib.LINE_STATS_SEGMENT  # a line of more items has a finishing launch

#: name -> (builder(dtype), the path or paths the object must report or None, whether a call is more than one launch)
CASES = {
    "halo_fill": (lambda t: C.halo_fill(t, "ifirst", 2), None, False),
    "halo_fill-kfirst-9": (lambda t: C.halo_fill(t, "kfirst", MORE_THAN_ONE_LAUNCH), None, True),
    "field_copy-rows": (lambda t: C.field_copy(t, "ifirst", "ifirst_unaligned", 1), [transfer_ref.ROWS], False),
    "field_copy-tiles": (lambda t: C.field_copy(t, "ifirst", "kfirst", 1, extent=(70, 35, 9)), [transfer_ref.TILES], False),
    "field_copy-items": (lambda t: C.field_copy(t, "kfirst", "ifirst", 1, strided=True), [transfer_ref.ITEMS], False),
    "field_copy-9": (lambda t: C.field_copy(t, "kfirst", "ifirst", MORE_THAN_ONE_LAUNCH), [transfer_ref.TILES] * 9, True),
    "field_stats": (lambda t: C.stats("field", t, 2), None, True),  # (a pass and a finishing launch, always)
    "field_stats-kfirst-9": (lambda t: C.stats("field", t, MORE_THAN_ONE_LAUNCH, layouts=("kfirst", "kfirst")), None, True),
    "level_stats": (lambda t: C.stats("level", t, 2), None, True),
    "level_stats-kfirst-9": (lambda t: C.stats("level", t, MORE_THAN_ONE_LAUNCH, layouts=("kfirst", "kfirst")), None, True),
    "line_stats-tiles": (lambda t: C.stats("line", t, 2, extent=(5, 65, 2), axis=I), line_stats_ref.TILES, False),
    "line_stats-lanes": (lambda t: C.stats("line", t, 2, extent=(5, 65, 2), axis=J), line_stats_ref.LANES, False),
    "line_stats-items": (lambda t: C.stats("line", t, 2, extent=(5, 65, 2), axis=I, layouts=("ifirst", "kfirst")), line_stats_ref.ITEMS, False),
    "line_stats-finish": (lambda t: C.stats("line", t, 2, extent=(G + 1, 63, 5), axis=I), line_stats_ref.TILES, True),  # (a line of two segments)
    "line_stats-finish-9": (lambda t: C.stats("line", t, MORE_THAN_ONE_LAUNCH, extent=(5, 63, G + 1), axis=K), line_stats_ref.LANES, True),
    "line_find-lanes": (lambda t: C.line_find(t, K, "ifirst", 1, (65, 2, 33)), LANES, False),
    "line_find-tiles": (lambda t: C.line_find(t, K, "kfirst", 2, (65, 2, 33)), TILES, False),
    "line_find-items": (lambda t: C.line_find(t, I, "kfirst", 1, (33, 1, 1), what="argmax"), ITEMS, False),
    "line_find-9": (lambda t: C.line_find(t, K, "ifirst", MORE_THAN_ONE_LAUNCH, (5, 3, 17)), LANES, True),
    "histogram-rows-small": (lambda t: C.histogram(t, "ifirst", 16, None), "rows", False),  # (nb <= 1024: a counter copy per wave)
    "histogram-rows-large-by-k": (lambda t: C.histogram(t, "ifirst", 2048, "K"), "rows", False),
    "histogram-items-by-k": (lambda t: C.histogram(t, "kfirst", 16, "K"), "items", False),  # (K is the only unit axis and a row has one level)
    "histogram-accumulate": (lambda t: C.histogram(t, "kfirst", 2048, None, accumulate=True), "rows", False),  # (cleared with reset())
    "line_scan-tiles": (lambda t: C.line_scan(t, I, "ifirst", None, 1, (33, 65, 2)), TILES, False),
    "line_scan-lanes": (lambda t: C.line_scan(t, I, "kfirst", None, 1, (33, 65, 2)), LANES, False),
    "line_scan-items": (lambda t: C.line_scan(t, I, "ifirst", "kfirst", 1, (33, 65, 2)), ITEMS, False),
    "line_scan-9": (lambda t: C.line_scan(t, K, "ifirst", None, MORE_THAN_ONE_LAUNCH, (5, 3, 17)), LANES, True),
    "line_solve-tiles": (lambda t: C.line_solve(t, I, "ifirst", None, 1, (33, 65, 2)), TILES, False),
    "line_solve-lanes": (lambda t: C.line_solve(t, K, "ifirst", None, 1, (65, 2, 33)), LANES, False),
    "line_solve-items": (lambda t: C.line_solve(t, I, "ifirst", "kfirst", 1, (33, 65, 2)), ITEMS, False),
    "line_solve-periodic-long": (lambda t: C.line_solve(t, K, "kfirst", None, 2, (3, 2, 130), periodic=True), TILES, False),
    "line_solve-9": (lambda t: C.line_solve(t, K, "ifirst", None, MORE_THAN_ONE_LAUNCH, (5, 3, 17)), LANES, True),
    "line_filter-I-16": (lambda t: C.line_filter(t, I, "ifirst", None, 1, (16, 63, 1)), TILES, False),
    "line_filter-I-64": (lambda t: C.line_filter(t, I, "kfirst", None, 1, (64, 3, 2)), LANES, False),
    "line_filter-K-16": (lambda t: C.line_filter(t, K, "kfirst", None, 1, (63, 1, 16)), TILES, False),
    "line_filter-K-64-items": (lambda t: C.line_filter(t, K, "jfirst", "ifirst", 1, (3, 2, 64)), ITEMS, False),
    "line_filter-9": (lambda t: C.line_filter(t, K, "ifirst", None, MORE_THAN_ONE_LAUNCH, (5, 3, 8)), LANES, True),
    "line_spectrum-I-16": (lambda t: C.line_spectrum(t, I, "ifirst", 2, (16, 63, 1)), TILES, False),
    "line_spectrum-I-64": (lambda t: C.line_spectrum(t, I, "kfirst", 1, (64, 3, 2)), LANES, False),
    "line_spectrum-K-16": (lambda t: C.line_spectrum(t, K, "kfirst", 1, (63, 1, 16)), TILES, False),
    "line_spectrum-K-64": (lambda t: C.line_spectrum(t, K, "ifirst", 1, (3, 2, 64)), LANES, False),
    "line_spectrum-9": (lambda t: C.line_spectrum(t, K, "ifirst", MORE_THAN_ONE_LAUNCH, (5, 3, 8)), LANES, True),
    "vertical_remap": (lambda t: C.vertical_remap(t, "ifirst", 2), None, False),
    "vertical_remap-kfirst-9": (lambda t: C.vertical_remap(t, "kfirst", MORE_THAN_ONE_LAUNCH), None, True),
    "vertical_interp": (lambda t: C.vertical_interp(t, "ifirst", 2), None, False),
    "vertical_interp-kfirst-9": (lambda t: C.vertical_interp(t, "kfirst", MORE_THAN_ONE_LAUNCH), None, True),
    "horizontal_interp": (lambda t: C.horizontal_interp(t, "ifirst", 2), None, False),
    "horizontal_interp-kfirst-9": (lambda t: C.horizontal_interp(t, "kfirst", MORE_THAN_ONE_LAUNCH), None, True),
    "horizontal_remap": (lambda t: C.horizontal_remap(t, "ifirst", 2), None, False),
    "horizontal_remap-kfirst-9": (lambda t: C.horizontal_remap(t, "kfirst", MORE_THAN_ONE_LAUNCH), None, True),
    "departure_interp": (lambda t: C.departure_interp(t, "ifirst", 2), None, False),
    "departure_interp-kfirst-9": (lambda t: C.departure_interp(t, "kfirst", MORE_THAN_ONE_LAUNCH), None, True),
    "sample-columns": (lambda t: C.sample(t, "ifirst", 2, False), None, False),
    "sample-points-kfirst-9": (lambda t: C.sample(t, "kfirst", MORE_THAN_ONE_LAUNCH, True), None, True),
}


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name", list(CASES))
def test_one_capture_replays_what_the_eager_call_computes(name, dtype):
    build, path, several = CASES[name]
    case = build(dtype)
    obj = case.obj
    if path is not None:
        reported = obj.paths if hasattr(obj, "paths") else obj.path
        assert reported == path, (name, reported, path)
    if hasattr(case, "expected_paths"):
        assert obj.paths == case.expected_paths
    assert (obj.launches > 1) == several, (name, obj.launches)
    C.protocol(case, f"{name} {np.dtype(dtype)}")


def test_every_frozen_class_has_a_case():
    """``Upload`` and ``Download`` are out of scope: they stage through pinned host memory with events."""
    classes = {"halo_fill", "field_stats", "level_stats", "line_stats", "field_copy", "vertical_remap", "vertical_interp", "horizontal_interp",
               "horizontal_remap", "departure_interp", "sample", "line_solve", "line_scan", "line_find", "line_filter", "line_spectrum",
               "histogram"}
    assert {name.split("-")[0] for name in CASES} == classes
    assert all(any(name.startswith(c) and CASES[name][2] for name in CASES) for c in classes - {"histogram"})  # (at most 8 fields, one launch)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("by", [None, "K"])
def test_the_zeroing_of_a_histogram_is_a_node_of_the_graph(by, dtype):
    """Two replays on the same input without clearing: exactly the counts of one without ``accumulate``, exactly twice with it."""
    import torch

    for accumulate in (False, True):
        case = C.histogram(dtype, "ifirst", 16, by, accumulate=accumulate)
        h = case.obj
        case.load(0)
        h.reset()
        h()
        torch.cuda.synchronize()
        case.check(0, f"accumulate {accumulate}: eager on A")
        h.reset()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            h()
        torch.cuda.synchronize()
        assert not h.result.tensor.any().item(), "the capture counted"
        case.load(1)
        graph.replay()
        torch.cuda.synchronize()
        case.check(1, f"accumulate {accumulate}: replay on B")
        one = h.result.tensor.cpu().numpy().copy()
        assert one.sum() == 2 * 65 * 7 * 5  # (two fields: every item in exactly one counter)
        if accumulate:
            h.reset()
        graph.replay()
        graph.replay()
        two, = (h.result.tensor.cpu().numpy(),)
        assert np.array_equal(two, 2 * one if accumulate else one), f"accumulate {accumulate}"
        got, = h.get()[:1]
        assert np.array_equal(np.atleast_2d(got.counts), two[0][:, :16])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_replay_searches_for_the_level_of_its_capture(dtype):
    """``LineFind.set_level`` after a capture: the levels are passed by value at each call, so the graph keeps the level it was
    captured with; the next eager call searches for the new one."""
    import torch

    case = C.line_find(dtype, K, "ifirst", 1, (65, 2, 33))
    lf = case.obj
    graph = C.protocol(case, f"line_find {np.dtype(dtype)}")
    lf.set_level(0.25)
    assert lf.level == (0.25,)
    case.load(1)
    graph.replay()
    torch.cuda.synchronize()
    case.check(1, "a replay after set_level")  # (the restatement for the level 0.0 of the capture)
    captured = lf.result.tensor.cpu().numpy().copy()
    lf()
    torch.cuda.synchronize()
    moved = lf.result.tensor.cpu().numpy()
    _, box, _ = C.boxed((65, 2, 33))
    want = case.want_with([0.25])([case.images[1][0][box]])
    assert C._same_or_both_nan(moved, want.reshape(moved.shape)) and not C._same_or_both_nan(moved, captured)


def test_line_filters_refuse_a_line_that_is_no_power_of_two():
    """Why the cases above have two powers of two and no other length."""
    import torch

    from gt4py_amd import linefilter

    src, dst = (torch.zeros(12, 5, 3, dtype=torch.float64, device="cuda") for _ in range(2))
    response = torch.ones(7, dtype=torch.float64, device="cuda")
    with pytest.raises(TypeError, match="the length must be a power of two"):
        linefilter.LineFilter(dst, src, axis="I", response=response)
    with pytest.raises(TypeError, match="the length must be a power of two"):
        linefilter.LineSpectrum([src], axis="I")


# ---- one composed step ---------------------------------------------------------------------------------------------------------------
def scale_by_position(state: Field["T"], position: Field[IJ, np.float64], out: Field[np.float64]):  # noqa: F821
    with computation(PARALLEL), interval(...):
        out = state * position  # noqa: F841


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("layout", ["ifirst", "kfirst"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_composed_step_captured_once_replays_three_eager_steps(dtype, layout):
    """A single stream, no parallel branches, nothing allocated inside the capture.  After every step the state (ghost cells
    included), the statistics, the profiles, the counters, what the search found and the last stencil's output are the bits of the
    eager run of that step; every step is also compared with the numpy chain, each part with its own file's comparator (bits; the
    statistics with ``same_bits``, the positions with NaN equal to NaN)."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import boundary, diagnostics, histogram, linefind, linesolve, transfer
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates
    from gt4py_amd.storage.device_array import DeviceArray

    backend = "hip:mi300"

    def field(host):
        if layout == "ifirst":
            return gt_storage.from_array(host, host.dtype, backend=backend, aligned_index=S.ORIGIN)
        return DeviceArray(torch.from_numpy(np.ascontiguousarray(host)).cuda())  # numpy's C order: K contiguous

    host_state, host_coefs = S.inputs(dtype)
    zeros = np.zeros(S.SHAPE, dtype=dtype)
    state, tmp, sol = field(host_state), field(zeros), field(zeros)
    out = field(np.zeros(S.SHAPE))
    coefs = [torch.from_numpy(c).cuda() for c in host_coefs]
    # literals of the fields' precision: what the oracle's numpy Laplacian restates (a float64 literal widens a float32 step)
    lap = gtscript.stencil(backend=backend, definition=hip_templates.lap_notebook, dtypes={"T": dtype}, device_sync=False,
                           literal_float_precision=8 * np.dtype(dtype).itemsize)
    scale = gtscript.stencil(backend=backend, definition=scale_by_position, dtypes={"T": dtype}, device_sync=False)
    fill = boundary.HaloFill([state], halo=S.HALO, mode=S.MODES)
    lap_f = lap.freeze(origin={"inp": S.ORIGIN, "out": S.ORIGIN}, domain=S.DOMAIN)
    solve = linesolve.LineSolve([sol], [tmp], lower=coefs[0], diag=coefs[1], upper=coefs[2], axis="K", halo=S.HALO)
    copy = transfer.FieldCopy([state], [sol], origin=S.ORIGIN, domain=S.DOMAIN)
    field_stats = diagnostics.FieldStats([state], halo=S.HALO)
    level_stats = diagnostics.LevelStats([state], halo=S.HALO)
    hist = histogram.Histogram([state], edges=S.EDGES, by="K", halo=S.HALO)
    find = linefind.LineFind([state], axis="K", what="crossing", level=S.LEVEL, missing=S.MISSING, halo=S.HALO)
    position = find.section("position")  # over the whole array, ghost cells included: the same origin as the state's
    assert position.shape == S.SHAPE[:2] and field_stats.domain == level_stats.domain == hist.domain == S.DOMAIN
    assert solve.extent == find.extent == S.SHAPE and copy.extent == S.DOMAIN
    scale_f = scale.freeze(origin={"state": S.ORIGIN, "position": S.ORIGIN[:2], "out": S.ORIGIN}, domain=S.DOMAIN)

    def step():
        fill()
        lap_f(inp=state, out=tmp)
        solve()
        copy()
        field_stats()
        level_stats()
        hist()
        find()
        scale_f(state=state, position=position, out=out)

    def reset():
        state.tensor.copy_(torch.from_numpy(host_state))
        for a in (tmp, sol, out):
            a.tensor.zero_()
        for r in (field_stats, level_stats, hist, find):
            r.result.tensor.fill_(-7)
        torch.cuda.synchronize()

    def collect():
        torch.cuda.synchronize()
        return {"state": state.get(), "laplacian": tmp.get()[S.BOX], "stats": field_stats.result.get()[0], "profile": level_stats.result.get()[0],
                "counts": hist.result.get()[0], "found": find.result.get()[0], "out": out.get()}

    reset()
    eager = []
    for _ in range(3):
        step()
        eager.append(collect())

    reset()
    before = collect()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    after = collect()
    assert all(_same_bits(after[k], before[k]) for k in before), "the capture wrote something"
    for n in range(3):
        graph.replay()
        got = collect()
        for name in got:
            assert _same_bits(got[name], eager[n][name]), f"step {n + 1}: {name} of the replay is not the eager run's"

    i, j = S.BOX[0], S.BOX[1]
    for n, want in enumerate(S.run(dtype)):
        got, about = eager[n], f"{np.dtype(dtype)} {layout} step {n + 1}"
        assert _same_bits(got["laplacian"], want["laplacian"]), f"{about}: the Laplacian"
        assert _same_bits(got["state"], want["state"]), f"{about}: the state (halo fill, solve and copy)"
        assert stats_ref.same_bits(got["stats"], want["stats"]), f"{about}: FieldStats"
        assert level_stats_ref.same_bits(got["profile"], want["profile"]), f"{about}: LevelStats"
        assert got["counts"].tobytes() == want["counts"].tobytes(), f"{about}: Histogram"
        found = np.ascontiguousarray(got["found"].transpose(0, 2, 1)[:, i, j])  # (3, nB, nA) of the whole array -> (3, ni, nj) of the box
        assert C._same_or_both_nan(found, want["found"]), f"{about}: LineFind"
        assert _same_bits(got["out"][S.BOX], want["out"]) and not got["out"][:S.HALO].any(), f"{about}: the stencil on the position"
