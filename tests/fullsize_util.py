"""Whole-field, bit-for-bit comparison of full-size results with the oracle, slab by slab.

The full-size GPU cases in test_gpu_stencils.py compare EVERY element of an output array -- its halo and the padding at the
end of its rows included -- with a sentinel-filled copy into which the oracle wrote the compute domain.  Arrays of several GB
are compared in slabs along an axis on which the stencil's points are independent (K for lap5 / hdiff, J for the column
solvers), so host memory stays bounded.  Elements are compared as bit patterns (uint64 / uint32): ``np.array_equal`` holds
-0.0 equal to +0.0, and the flux limiter produces exact zeros of either sign on quantized inputs.

Works on device and on host torch tensors alike (tests/test_oracle.py checks the helper itself on the CPU).
"""

from __future__ import annotations

import os
from typing import Callable, Dict, Sequence

import numpy as np
import torch

from device_layouts import SENTINEL

_UINT = {np.dtype(np.float64): np.uint64, np.dtype(np.float32): np.uint32}
_TINT = {8: torch.int64, 4: torch.int32}
_NP = {torch.float64: np.float64, torch.float32: np.float32}
# what the elements a kernel must not write hold: NaNs with a payload no arithmetic produces
SENTINEL_BITS = {isz: SENTINEL[isz] for isz in (8, 4)}


def oracle_threads() -> int:
    """The CPUs this process may use (never more than 16): ``nproc`` counts the whole machine."""
    return min(16, len(os.sched_getaffinity(0)))


def padded(t: torch.Tensor) -> torch.Tensor:
    """``t`` widened to the whole row pitch of its storage (the padding after the last column of every row), when ``t`` is
    an I-contiguous IJK view whose storage holds it; else ``t`` itself."""
    si, sj, sk = t.stride()
    ni, nj, nk = t.shape
    if si != 1 or sj <= ni or sk % sj != 0 or sk // sj < nj:
        return t
    njp = sk // sj
    if (t.storage_offset() + sk * (nk - 1) + sj * njp) * t.element_size() > t.untyped_storage().nbytes():
        njp = nj
        if (t.storage_offset() + sk * (nk - 1) + sj * nj) * t.element_size() > t.untyped_storage().nbytes():
            return t
    return torch.as_strided(t, (sj, njp, nk), (1, sj, sk), t.storage_offset())


def fill_sentinel(t: torch.Tensor) -> None:
    """Every element of ``padded(t)`` := the sentinel."""
    padded(t).view(_TINT[t.element_size()]).fill_(SENTINEL_BITS[t.element_size()])


def fill_uniform(t: torch.Tensor, gen: torch.Generator, lo: float, hi: float, quantum: float = 0.0) -> None:
    """``t`` := U[lo, hi) drawn on ``t``'s device from ``gen``; rounded down to multiples of ``quantum`` when given (exact
    in both float types for quanta like 1/8: equal neighbours, exact zeros)."""
    r = torch.rand(t.shape, dtype=t.dtype, device=t.device, generator=gen) * (hi - lo) + lo
    if quantum:
        r = torch.floor(r / quantum) * quantum
    t.copy_(r)
    del r


def host(t: torch.Tensor, axis: int, lo: int, hi: int) -> np.ndarray:
    """Bit-exact, I-contiguous host copy of ``t`` restricted to [lo, hi) along ``axis`` (moved as integers: no float
    arithmetic touches a NaN payload on the way)."""
    s = t.view(_TINT[t.element_size()]).narrow(axis, lo, hi - lo).permute(2, 1, 0).contiguous().cpu().numpy()
    return s.view(_NP[t.dtype]).transpose(2, 1, 0)


def sentinel_slab(t: torch.Tensor, axis: int, lo: int, hi: int) -> np.ndarray:
    """An I-contiguous host array shaped like ``padded(t)`` restricted to [lo, hi) along ``axis``, every element the
    sentinel: the expected slab, before the oracle writes the compute domain into it."""
    shape = list(padded(t).shape)
    shape[axis] = hi - lo
    dt = _NP[t.dtype]
    a = np.empty(shape[::-1], dtype=dt).transpose(2, 1, 0)
    a.view(_UINT[np.dtype(dt)])[...] = SENTINEL_BITS[t.element_size()]
    return a


class Mismatches:
    """Running tally of bitwise mismatches over the slabs of one array."""

    def __init__(self, keep: int = 8):
        self.count, self.keep, self.first, self.max_abs, self.nan, self.all_signed_zero = 0, keep, [], 0.0, 0, True

    def add(self, got: np.ndarray, want: np.ndarray, offset: Sequence[int] = (0, 0, 0)) -> None:
        assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
        u = _UINT[got.dtype]
        bad = got.view(u) != want.view(u)
        levels = np.flatnonzero(bad.any(axis=(0, 1)))
        for k in levels:  # level by level: no temporary larger than one level
            b = bad[:, :, k]
            self.count += int(b.sum())
            with np.errstate(invalid="ignore", over="ignore"):  # (float32 signalling NaNs widen with a warning)
                g, w = got[:, :, k][b].astype(np.float64), want[:, :, k][b].astype(np.float64)
                d = np.abs(g - w)
            nan = np.isnan(d)
            self.nan += int(nan.sum())
            if not nan.all():
                self.max_abs = max(self.max_abs, float(d[~nan].max()))
            self.all_signed_zero &= bool(((g == 0) & (w == 0)).all())
            if len(self.first) < self.keep:
                ji = np.argwhere(b.T)[: self.keep - len(self.first)]  # (j, i) in memory order of an I-contiguous array
                self.first += [(int(i) + offset[0], int(j) + offset[1], int(k) + offset[2]) for j, i in ji]

    def report(self) -> str:
        if not self.count:
            return ""
        zero = "every one of them a sign-of-zero difference" if self.all_signed_zero else "not only sign-of-zero differences"
        nan = f" ({self.nan} of them against a NaN: a sentinel overwritten or left in place)" if self.nan else ""
        return (f"{self.count} mismatching point(s){nan}; first at (i, j, k) = {self.first}; largest absolute difference "
                f"{self.max_abs:.6g}; {zero}")


def bitwise_report(got: np.ndarray, want: np.ndarray) -> str:
    """'' when ``got`` and ``want`` are identical bit for bit, else what differs (see ``Mismatches``)."""
    m = Mismatches()
    m.add(got, want)
    return m.report()


def assert_bitwise(got: np.ndarray, want: np.ndarray, what: str = "") -> None:
    msg = bitwise_report(got, want)
    assert not msg, f"{what}: {msg}"


def check_slabs(what: str, outputs: Dict[str, torch.Tensor], expect: Callable[[int, int], Dict[str, np.ndarray]], axis: int,
                step: int, starts: Sequence[int] = None) -> None:
    """Compare every element of ``padded(outputs[name])`` with ``expect(lo, hi)[name]`` (a host array shaped like the padded
    slab, see ``sentinel_slab``) slab by slab: [lo, lo + step) along ``axis`` for every ``lo`` in ``starts`` (default: all
    slabs).  Fails with every mismatch of every array counted, the first ones located in array coordinates."""
    views = {n: padded(t) for n, t in outputs.items()}
    n = next(iter(views.values())).shape[axis]
    tally = {name: Mismatches() for name in views}
    for lo in (range(0, n, step) if starts is None else starts):
        hi = min(n, lo + step)
        want = expect(lo, hi)
        offset = [0, 0, 0]
        offset[axis] = lo
        for name, v in views.items():
            tally[name].add(host(v, axis, lo, hi), want[name], offset)
        del want
    bad = {name: m.report() for name, m in tally.items() if m.count}
    assert not bad, f"{what}: " + "; ".join(f"{name}: {msg}" for name, msg in bad.items())


def slab_step(t: torch.Tensor, axis: int, budget_bytes: int = 256 << 20) -> int:
    """Slab thickness along ``axis`` such that one padded slab of ``t`` holds at most ``budget_bytes``."""
    shape = padded(t).shape
    per = t.element_size() * int(np.prod(shape)) // shape[axis]
    return max(1, budget_bytes // per)


class StorageField:
    """What tests/gpu_util.py's C-ABI wrappers need of an array (``dtype``, ``field(origin)``) for a device storage -- the
    full-size cases allocate with gt4py_amd.storage instead of copying a host array in."""

    def __init__(self, array):
        self.array = array
        self.dtype = np.dtype(array.dtype)

    def field(self, origin):
        from gt4py_amd import _lib

        t = self.array.tensor
        return _lib.Field.make(self.array.ptr, tuple(t.shape), tuple(s * t.element_size() for s in t.stride()), origin)
