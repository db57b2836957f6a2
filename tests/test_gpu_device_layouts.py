"""``device_layouts.Dev`` itself: about ten GPU test files rest their byte-for-byte comparison on its ``assert_box`` and
``assert_unchanged``.  Every write here is a plain torch assignment into the buffer; no product code runs."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import device_layouts as L  # noqa: E402

SHAPE = (5, 4, 3)
BOX = (slice(1, 4), slice(1, 3))
OTHER_NAN = {4: 0x7FC1_2345, 8: 0x7FF8_0000_0BAD_F00D}  # quiet NaNs with a payload: neither np.nan's bits nor the sentinel's
ODD_BITS = 12345  # a subnormal in both dtypes: no value, sentinel or NaN of these tests

cases = pytest.mark.parametrize("layout, dtype", [(layout, dtype) for layout in L.LAYOUTS for dtype in (np.float32, np.float64)])


def _dev(layout, dtype, nan_at=None):
    """(a Dev of values in [1, 2) with the box of ``want`` already written to it, want)"""
    import torch

    rng = np.random.default_rng(11)
    values, want = rng.uniform(1, 2, SHAPE).astype(dtype), rng.uniform(1, 2, (3, 2, 3)).astype(dtype)
    if nan_at is not None:
        values[nan_at] = np.nan
    d = L.Dev(SHAPE, dtype, layout, values, align_i=1)
    d.lay.view[BOX] = torch.from_numpy(want.view(L.NP_INT[want.itemsize])).cuda()
    return d, want


def _places(d):
    """Flat indices outside the box: a ghost cell of the view; where the layout has them, a padding item between two rows and an
    item of the slack behind the view."""
    covered = np.zeros(d.lay.flat.numel(), dtype=bool)
    d.lay.host_view(covered)[...] = True
    last = int(np.flatnonzero(covered)[-1])
    free = np.flatnonzero(~covered)
    places = {"ghost cell": d.lay.offset}  # (the view's item [0, 0, 0])
    if d.lay.strides[0] == 1 and d.lay.strides[1] > SHAPE[0]:  # padded rows
        places["row padding"] = int(free[(free > d.lay.offset) & (free < last)][0])
        places["slack"] = int(free[free > last][-1])
    else:
        assert free.size == 0
    return places


def _inside(d):
    """The flat index of item [0, 0, 1] of the box."""
    return d.lay.offset + 1 * d.lay.strides[0] + 1 * d.lay.strides[1] + 1 * d.lay.strides[2]


@cases
def test_the_box_as_wanted_and_everything_else_untouched_passes_and_returns_the_box(layout, dtype):
    d, want = _dev(layout, dtype)
    got = d.assert_box(BOX, want, "case")
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes()


@cases
def test_one_item_inside_the_box_differs(layout, dtype):
    d, want = _dev(layout, dtype)
    d.lay.flat[_inside(d)] = ODD_BITS
    with pytest.raises(AssertionError, match=r"case: 1 items of the whole buffer differ \(1 of them in the box\)"):
        d.assert_box(BOX, want, "case")


@cases
def test_one_item_outside_the_box_differs(layout, dtype):
    names = ("ghost cell", "row padding", "slack") if layout.startswith("ifirst") else ("ghost cell",)
    for name in names:
        d, want = _dev(layout, dtype)
        index = _places(d)[name]
        d.lay.flat[index] = ODD_BITS
        with pytest.raises(AssertionError, match=rf"{name}: 1 items of the whole buffer differ \(0 of them in the box\), first at flat index \[{index}\]"):
            d.assert_box(BOX, want, name)


@cases
def test_nan_against_a_nan_of_another_payload_inside_the_box_passes(layout, dtype):
    d, want = _dev(layout, dtype)
    want[0, 0, 1] = np.nan
    d.lay.flat[_inside(d)] = OTHER_NAN[want.itemsize]
    got = d.assert_box(BOX, want, "case")
    ut = L.NP_UINT[want.itemsize]
    assert got.view(ut)[0, 0, 1] == OTHER_NAN[want.itemsize] != want.view(ut)[0, 0, 1]  # (the box as it is)


@cases
def test_nan_against_a_nan_of_another_payload_outside_the_box_fails(layout, dtype):
    """Outside the box the comparison is of integers: the ghost cell holds np.nan, the padding and the slack the sentinel NaN."""
    for name in ("ghost cell", "row padding", "slack"):
        d, want = _dev(layout, dtype, nan_at=(0, 0, 0))
        index = _places(d).get(name)
        if index is None:
            continue
        assert np.isnan(d.image.view(d.dtype)[index])
        d.lay.flat[index] = OTHER_NAN[want.itemsize]
        with pytest.raises(AssertionError, match=r"1 items of the whole buffer differ \(0 of them in the box\)"):
            d.assert_box(BOX, want, name)


@cases
def test_assert_unchanged_passes_before_and_fails_after_any_single_write(layout, dtype):
    import torch

    d = L.Dev(SHAPE, dtype, layout, np.random.default_rng(12).uniform(1, 2, SHAPE).astype(dtype), align_i=1)
    d.assert_unchanged("buffer")
    for index in [_inside(d), *_places(d).values()]:
        d.lay.flat[index] = ODD_BITS
        with pytest.raises(AssertionError, match="buffer changed"):
            d.assert_unchanged("buffer")
        d.lay.upload(d.image)
        d.assert_unchanged("buffer")
    line = L.Line(np.arange(7), dtype)
    assert line.values.dtype == dtype and line.given.dtype == {4: torch.float32, 8: torch.float64}[line.values.itemsize]
    line.assert_unchanged("line")
    line.given[3] = -1.0
    with pytest.raises(AssertionError, match="line changed"):
        line.assert_unchanged("line")
