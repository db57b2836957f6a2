"""The contract of ``gt4mi_field_histogram`` (include/gt4py_amd.h, csrc/field_histogram.hip.h) restated twice: item by item in
plain Python (:func:`slot_of`, :func:`count_items`) and vectorised in numpy (:func:`count`), plus the kernel's guess-and-correct
search (:func:`slot_guess`) restated so that it can be compared with the plain search on adversarial edges.  Test infrastructure:
imports no product code.

For nb bins the caller gives nb + 1 float64 edges e[0] < ... < e[nb], all finite.  Every item x, converted exactly to float64,
lands in exactly one of nb + 3 counters: the bins 0 .. nb-1, then below, above, nan:
  nan    if x != x
  below  if x < e[0]   (-inf included)
  above  if x > e[nb]  (+inf included)
  bin nb - 1 if x == e[nb] (the last bin is closed, as in numpy.histogram)
  else the bin b with e[b] <= x < e[b+1]; -0.0 == 0.0 as IEEE compares them."""

import numpy as np

BELOW, ABOVE, NAN, EXTRA = 0, 1, 2, 3
NUDGE, BISECT = 2, 13  # the constants of csrc/field_histogram.hip.h


def slot_of(x, e) -> int:
    """The slot of one item, by comparisons in the order the contract states them; the bin by a linear walk."""
    x = float(x)
    nb = len(e) - 1
    if x != x:
        return nb + NAN
    if x < e[0]:
        return nb + BELOW
    if x > e[nb]:
        return nb + ABOVE
    if x == e[nb]:
        return nb - 1
    b = 0
    while not (e[b] <= x < e[b + 1]):
        b += 1
    return b


def count_items(items, e) -> np.ndarray:
    """The nb + 3 counters of a flat list of items, one at a time."""
    out = np.zeros(len(e) - 1 + EXTRA, dtype=np.int64)
    for x in np.asarray(items).ravel():
        out[slot_of(x, e)] += 1
    return out


def slots(x, e) -> np.ndarray:
    """The slot of every item of ``x``, vectorised: searchsorted(e, x, 'right') - 1 with the last-edge rule."""
    e = np.asarray(e, dtype=np.float64)
    x = np.asarray(x).astype(np.float64)  # (exact for float32)
    nb = e.size - 1
    b = np.searchsorted(e, x, side="right") - 1
    b = np.where(x == e[nb], nb - 1, b)
    b = np.where(x < e[0], nb + BELOW, b)
    b = np.where(x > e[nb], nb + ABOVE, b)
    return np.where(x != x, nb + NAN, b).astype(np.int64)


def count(x, e) -> np.ndarray:
    """The nb + 3 counters of all items of ``x``."""
    return np.bincount(slots(x, e).ravel(), minlength=len(e) - 1 + EXTRA).astype(np.int64)


def count_box(box, e, by_k: bool) -> np.ndarray:
    """The (nrows, nb + 3) block of one field's IJK box: one row, or one per level."""
    if not by_k:
        return count(box, e)[None]
    return np.stack([count(box[:, :, k], e) for k in range(box.shape[2])])


def slot_guess(x, e) -> int:
    """The kernel's search: the bin guessed with one multiply, moved by at most NUDGE bins, accepted only if the comparisons
    against e[] hold, else a bisection of at most BISECT halvings.  Every loop is bounded by a constant."""
    x = np.float64(x)
    nb = len(e) - 1
    e0, top = np.float64(e[0]), np.float64(e[nb])
    if x != x:
        return nb + NAN
    if x < e0:
        return nb + BELOW
    if x > top:
        return nb + ABOVE
    with np.errstate(all="ignore"):
        scale = np.float64(nb) / (top - e0)
        t = (x - e0) * scale
    t = t if t >= 0.0 else np.float64(0.0)
    t = t if t <= nb - 1 else np.float64(nb - 1)
    g = int(t)
    for _ in range(NUDGE):
        if g > 0 and x < e[g]:
            g -= 1
        elif g < nb - 1 and x >= e[g + 1]:
            g += 1
    if e[g] <= x and (x < e[g + 1] or g == nb - 1):
        return g
    lo, hi = 0, nb
    for _ in range(BISECT):
        if hi - lo <= 1:
            break
        mid = (lo + hi) >> 1
        if x >= e[mid]:
            lo = mid
        else:
            hi = mid
    return lo
