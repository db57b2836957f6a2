"""numpy restatement of the order in which ``gt4mi_level_stats`` adds (csrc/level_stats.hip.h, header comment).

Imports no product code.  ``profile(a, b=None)`` takes the host copy of the compute-domain box (2-D or 3-D, float32 or float64;
``b`` may have extent 1 along an axis: a broadcast weight) and returns the nine rows (the eight slots, then the mean) as a
``(9, nk)`` float64 array, bit for bit what the kernels produce; ``depth(ni, nj)`` is the longest chain of additions any one
element passes through in that order.

The order of level k, a function of (ni, nj) alone:
  rows    a row is one j;  RW = ceil(nj / (4 * MAX_TILES)) rows per wave, 4 waves per tile, TL = ceil(nj / (4 * RW)) tiles
  lane    lane l of a wave owns the columns i with (i mod 256) div 4 == l and adds them, starting from +0.0, in the order
          (row, i) increasing over the wave's RW rows
  wave    balanced binary tree over the 64 lanes (neighbours first)
  tile    the four waves left to right
  finish  the TL tiles are halved level by level, new[i] = old[2 i] + old[2 i + 1], an odd last one carried up unchanged;
          mean = sum / count, one division
min / max do not depend on the order: NaN if any x is NaN, min(-0, +0) = -0, max(-0, +0) = +0.
"""

from __future__ import annotations

import numpy as np

from stats_ref import extremes, same_bits, terms  # noqa: F401  (same_bits: for the tests that compare against this file)

COUNT, NONFINITE, SUM, SUM_ABS, SUM_SQ, MIN, MAX, DOT, MEAN = range(9)
ROWS = 9
GROUP, LANES, WAVES, MAX_TILES = 4, 64, 4, 32  # MAX_TILES: this file's own copy of LT (a CPU test compares it to the library's)
CHUNK = GROUP * LANES


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def geometry(ni: int, nj: int):
    """(rows per wave, tiles per level, chunks of 256 columns per row)"""
    rw = _cdiv(int(nj), WAVES * MAX_TILES)
    return rw, _cdiv(int(nj), WAVES * rw), _cdiv(int(ni), CHUNK)


def halvings(tiles: int):
    """The number of values at every stage of the finish, from `tiles` down to 1."""
    counts = [int(tiles)]
    while counts[-1] > 1:
        counts.append((counts[-1] + 1) // 2)
    return counts


def depth(ni: int, nj: int) -> int:
    """Additions on the longest path from an element to the level's result: a lane's chain (the one onto +0.0 included), six
    levels of the butterfly, three wave additions and the halving levels."""
    rw, tiles, chunks = geometry(ni, nj)
    return rw * chunks * GROUP + 6 + (WAVES - 1) + (len(halvings(tiles)) - 1)


def ordered_sums(term: np.ndarray) -> np.ndarray:
    """Per-level sums of a float64 (ni, nj, nk) array in the documented order; every level on its own, all at once."""
    ni, nj, nk = term.shape
    rw, tiles, chunks = geometry(ni, nj)
    nwaves = tiles * WAVES
    padded = np.zeros((nk, nwaves * rw, chunks * CHUNK))
    valid = np.zeros(padded.shape[1:], dtype=bool)
    padded[:, :nj, :ni] = term.transpose(2, 1, 0)
    valid[:nj, :ni] = True

    def per_lane(x):  # (..., wave, row, chunk, lane, item) -> (..., wave, lane, the lane's sequence)
        lead = x.shape[:-2]
        x = x.reshape(lead + (nwaves, rw, chunks, LANES, GROUP))
        x = np.moveaxis(x, -2, -4)  # (..., wave, lane, row, chunk, item)
        return x.reshape(lead + (nwaves, LANES, rw * chunks * GROUP))

    seq, ok = per_lane(padded), per_lane(valid)
    with np.errstate(all="ignore"):
        acc = np.zeros((nk, nwaves, LANES))
        for s in range(seq.shape[-1]):
            acc = np.where(ok[:, :, s], acc + seq[:, :, :, s], acc)
        while acc.shape[-1] > 1:  # the butterfly: neighbours first
            acc = acc[..., 0::2] + acc[..., 1::2]
        w = acc.reshape(nk, tiles, WAVES)
        level = ((w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3]
        while level.shape[1] > 1:
            n = level.shape[1]
            nxt = level[:, 0:n - 1:2] + level[:, 1::2]
            level = np.concatenate([nxt, level[:, -1:]], axis=1) if n % 2 else nxt
    return level[:, 0]


def profile(a, b=None) -> np.ndarray:
    x, ax, sq, prod = terms(a, b)
    nk = x.shape[2]
    out = np.zeros((ROWS, nk))
    out[COUNT] = x.shape[0] * x.shape[1]
    out[NONFINITE] = np.count_nonzero(~np.isfinite(x), axis=(0, 1))
    out[SUM], out[SUM_ABS], out[SUM_SQ] = ordered_sums(x), ordered_sums(ax), ordered_sums(sq)
    for k in range(nk):
        out[MIN, k], out[MAX, k] = extremes(x[:, :, k])
    if prod is not None:
        out[DOT] = ordered_sums(prod)
    with np.errstate(all="ignore"):
        out[MEAN] = out[SUM] / out[COUNT]
    return out
