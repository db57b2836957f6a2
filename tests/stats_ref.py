"""numpy restatement of the order in which ``gt4mi_field_stats`` adds (csrc/field_stats.hip.h, header comment).

Imports no product code.  ``stats(a, b=None)`` takes the host copy of the compute-domain box (2-D or 3-D, float32 or float64;
``b`` may have extent 1 along an axis: a broadcast weight) and returns the eight slots as a float64 array, bit for bit what the
kernels produce; ``depth(domain)`` is the longest chain of additions any one element passes through in that order.

The order, a function of the domain (ni, nj, nk) alone:
  rows    r = j + nj * k;  RW = ceil(rows / (4 * 4096)) rows per wave, 4 waves per tile, tiles = ceil(rows / (4 * RW))
  lane    lane l of a wave owns the columns i with (i mod 256) div 4 == l and adds them, starting from +0.0, in the order
          (row, i) increasing over the wave's RW rows
  wave    balanced binary tree over the 64 lanes (neighbours first)
  tile    the four waves left to right
  finish  leaf q of 128 adds C = ceil(tiles / 128) consecutive tiles left to right starting from its first tile; the leaves are
          halved level by level, new[i] = old[2 i] + old[2 i + 1], an odd last one carried up unchanged
min / max do not depend on the order: NaN if any x is NaN, min(-0, +0) = -0, max(-0, +0) = +0.
"""

from __future__ import annotations

import numpy as np

COUNT, NONFINITE, SUM, SUM_ABS, SUM_SQ, MIN, MAX, DOT = range(8)
GROUP, LANES, WAVES, MAX_TILES, LEAVES = 4, 64, 4, 4096, 128
CHUNK = GROUP * LANES


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def geometry(domain):
    """(rows, rows per wave, tiles, chunks of 256 columns per row, tiles per finish leaf, finish leaves)"""
    ni, nj, nk = (int(d) for d in domain)
    rows = nj * nk
    rw = _cdiv(rows, WAVES * MAX_TILES)
    tiles = _cdiv(rows, WAVES * rw)
    per_leaf = _cdiv(tiles, LEAVES)
    return rows, rw, tiles, _cdiv(ni, CHUNK), per_leaf, _cdiv(tiles, per_leaf)


def depth(domain) -> int:
    """Additions on the longest path from an element to the result: a lane's chain (the one onto +0.0 included), six levels of
    the butterfly, three wave additions, the leaf's chain and the halving levels."""
    rows, rw, tiles, chunks, per_leaf, leaves = geometry(domain)
    levels = 0
    while leaves > 1:
        leaves = (leaves + 1) // 2
        levels += 1
    return rw * chunks * GROUP + 6 + (WAVES - 1) + (per_leaf - 1) + levels


def ordered_sum(term: np.ndarray) -> float:
    """Sum of a float64 (ni, nj, nk) array in the documented order."""
    ni, nj, nk = term.shape
    rows, rw, tiles, chunks, per_leaf, leaves = geometry(term.shape)
    nwaves = tiles * WAVES
    padded = np.zeros((nwaves * rw, chunks * CHUNK))
    valid = np.zeros(padded.shape, dtype=bool)
    padded[:rows, :ni] = term.transpose(2, 1, 0).reshape(rows, ni)
    valid[:rows, :ni] = True

    def per_lane(x):  # (wave, row, chunk, lane, item) -> (wave, lane, the lane's sequence)
        return x.reshape(nwaves, rw, chunks, LANES, GROUP).transpose(0, 3, 1, 2, 4).reshape(nwaves, LANES, rw * chunks * GROUP)

    seq, ok = per_lane(padded), per_lane(valid)
    with np.errstate(all="ignore"):
        acc = np.zeros((nwaves, LANES))
        for s in range(seq.shape[2]):
            acc = np.where(ok[:, :, s], acc + seq[:, :, s], acc)
        while acc.shape[1] > 1:  # the butterfly: neighbours first
            acc = acc[:, 0::2] + acc[:, 1::2]
        w = acc.reshape(tiles, WAVES)
        t = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
        level = []
        for q in range(leaves):
            part = t[q * per_leaf: (q + 1) * per_leaf]
            v = part[0]
            for x in part[1:]:
                v = v + x
            level.append(v)
        while len(level) > 1:
            nxt = [level[2 * i] + level[2 * i + 1] for i in range(len(level) // 2)]
            if len(level) % 2:
                nxt.append(level[-1])
            level = nxt
    return float(level[0])


def _box3(a):
    a = np.asarray(a)
    assert a.ndim in (2, 3) and a.dtype in (np.float32, np.float64), (a.ndim, a.dtype)
    return a.reshape(a.shape + (1,) * (3 - a.ndim))


def terms(a, b=None):
    """The float64 arrays that are summed: x, |x|, x * x and a * b (None without b), each product and difference rounded once."""
    a64 = _box3(a).astype(np.float64)
    with np.errstate(all="ignore"):
        if b is None:
            x, prod = a64, None
        else:
            b64 = np.broadcast_to(_box3(b).astype(np.float64), a64.shape)
            x, prod = a64 - b64, a64 * b64
        return x, np.abs(x), x * x, prod


def extremes(x):
    if np.isnan(x).any():
        return np.nan, np.nan
    lo, hi = float(x.min()), float(x.max())
    zeros = x == 0
    if lo == 0:
        lo = -0.0 if np.signbit(x[zeros]).any() else 0.0
    if hi == 0:
        hi = 0.0 if (~np.signbit(x[zeros])).any() else -0.0
    return lo, hi


def stats(a, b=None) -> np.ndarray:
    x, ax, sq, prod = terms(a, b)
    out = np.zeros(8)
    out[COUNT] = x.size
    out[NONFINITE] = np.count_nonzero(~np.isfinite(x))
    out[SUM], out[SUM_ABS], out[SUM_SQ] = ordered_sum(x), ordered_sum(ax), ordered_sum(sq)
    out[MIN], out[MAX] = extremes(x)
    out[DOT] = ordered_sum(prod) if prod is not None else 0.0
    return out


def same_bits(got, want) -> bool:
    """Bit for bit, NaN slots compared as NaN (their payload and sign are unspecified)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)))
