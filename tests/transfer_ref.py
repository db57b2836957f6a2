"""The field copy's contract restated with numpy slicing on host images of the FLAT buffers (``gt4mi_field_copy`` in
include/gt4py_amd.h; gt4py_amd/transfer.py), the rule that names the path a pair takes, and the inputs of the conversions.  The
buffers and their four layouts are tests/device_layouts.py's.  Test infrastructure; imports no product code and (at import) no
torch."""

from __future__ import annotations

import numpy as np

from device_layouts import NP_UINT

ITEMSIZES = [1, 2, 4, 8]
K_LONG = [(66, 3, 65), (7, 2, 200)]  # these cross a tile edge along K; device_layouts.DOMAINS never does
ROWS, TILES, ITEMS = 0, 1, 2


def box_slices(start, extent):
    return tuple(slice(s, s + e) for s, e in zip(start, extent))


def copy_box(dst_view: np.ndarray, src_view: np.ndarray, dst_start, src_start, extent) -> None:
    """THE CONTRACT: the box of src lands in the box of dst; nothing else changes."""
    dst_view[box_slices(dst_start, extent)] = src_view[box_slices(src_start, extent)]


def expected_path(dst_strides, src_strides, extent) -> int:
    """Strides in ITEMS.  ROWS: both sides have unit stride along the same axis; TILES: along different axes; ITEMS: a side has no
    unit stride on an axis of extent > 1, or a src stride is 0 there."""
    if any(e > 1 and s == 0 for s, e in zip(src_strides, extent)):
        return ITEMS
    unit_d = [ax for ax in range(3) if extent[ax] > 1 and dst_strides[ax] == 1]
    unit_s = [ax for ax in range(3) if extent[ax] > 1 and src_strides[ax] == 1]
    if not unit_d or not unit_s:
        return ITEMS
    return ROWS if set(unit_d) & set(unit_s) else TILES


# ---- conversion: a random field with IEEE edge values planted in it ------------------------------------------------------------
_F32_MAX = float(np.finfo(np.float32).max)
#: (float64 value, the float32 that ONE rounding to nearest even gives): ties, the subnormal boundary, overflow, signed zeros
NARROWING_EXPECTATIONS = [
    (1.0 + 2.0**-24, 1.0),                                  # a tie: to the even neighbour below
    (1.0 + 3 * 2.0**-24, 1.0 + 2.0**-22),                   # a tie: to the even neighbour above
    (1.0 + 2.0**-24 + 2.0**-52, 1.0 + 2.0**-23),            # just above a tie
    (-(1.0 + 2.0**-24), -1.0),
    (_F32_MAX + 2.0**103, np.inf),                          # max + half an ulp: the tie goes to infinity
    (-(_F32_MAX + 2.0**103), -np.inf),
    (_F32_MAX + 2.0**103 - 2.0**75, _F32_MAX),              # just below it
    (1e300, np.inf), (-1e300, -np.inf),
    (2.0**-149, 2.0**-149),                                 # the smallest float32 subnormal
    (2.0**-150, 0.0),                                       # a tie between 0 and it: to 0 (even)
    (-(2.0**-150), -0.0),
    (2.0**-150 * (1.0 + 2.0**-52), 2.0**-149),              # just above that tie
    (3 * 2.0**-150, 2.0**-148),                             # a tie between two subnormals: to the even one
    (2.0**-126 - 2.0**-150, 2.0**-126),                     # rounds up INTO the normal range
    (-(2.0**-151), -0.0), (5e-324, 0.0),                    # underflow, sign kept
    (0.0, 0.0), (-0.0, -0.0),
]


def conversion_inputs(shape=(65, 63, 7)):
    """(a float64 field, a float32 field): random values over many magnitudes with the edge values of tests/edge_values.py and
    the ones above planted at random points, at most 1 % NaNs (both signs, with payloads)."""
    import edge_values as E

    rng = np.random.default_rng(E._seed("transfer", tuple(shape)))
    n = int(np.prod(shape))
    out = []
    for dt in (np.float64, np.float32):
        a = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 7, n)).astype(dt)
        planted = [np.asarray([v for v, _ in NARROWING_EXPECTATIONS], dtype=np.float64)] if dt is np.float64 else []
        planted += [E.palette(regime, dt)[0] for regime in E.REGIMES]
        planted += [E.palette(regime, np.float32)[0].astype(dt) for regime in E.REGIMES]
        planted.append(np.asarray([np.inf, -np.inf], dtype=dt))
        values = np.concatenate([np.asarray(p, dtype=dt) for p in planted])
        where = rng.choice(n, size=(values.size, 4), replace=False)  # every value at four points
        a[where] = values[:, None]
        ut = NP_UINT[np.dtype(dt).itemsize]
        quiet = {4: [0x7FC0_0000, 0xFFC0_0000, 0x7FC1_2345, 0xFFC5_4321],
                 8: [0x7FF8_0000_0000_0000, 0xFFF8_0000_0000_0000, 0x7FF8_0000_0BAD_F00D, 0xFFF8_0000_DEAD_BEEF]}[np.dtype(dt).itemsize]
        free = np.setdiff1d(np.arange(n), where.ravel())
        nan_at = rng.choice(free, size=n // 200, replace=False)  # 0.5 %
        a.view(ut)[nan_at] = np.asarray(quiet, dtype=ut)[rng.integers(0, 4, nan_at.size)]
        out.append(a.reshape(shape))
    return out[0], out[1]
