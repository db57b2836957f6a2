"""numpy restatement of the halo fill's contract (``gt4mi_halo_fill`` in include/gt4py_amd.h; gt4py_amd/boundary.py), as
SEQUENTIAL slice assignments: the I sides first, then the J sides over the whole padded I range, honouring ``sides``.

Written from the contract's text, not from the kernel: one assignment per ghost plane, each reading what the assignments
before it left.  tests/test_boundary.py pins it to ``numpy.pad``; tests/test_gpu_boundary.py compares the kernel with it."""

from __future__ import annotations

import itertools

import numpy as np

I_LO, I_HI, J_LO, J_HI, ALL = 1, 2, 4, 8, 15
COPY_MODES = ("periodic", "zero_gradient", "symmetric", "reflect")
MODES = COPY_MODES + ("constant",)
NUMPY_PAD = {"periodic": "wrap", "zero_gradient": "edge", "symmetric": "symmetric", "reflect": "reflect", "constant": "constant"}


def source_index(mode: str, low: bool, d: int, n: int) -> int:
    """Index in [0, n) that the cell at distance d >= 1 outside an axis of n cells takes its value from."""
    return {"periodic": (n - d, d - 1), "zero_gradient": (0, n - 1), "symmetric": (d - 1, n - d),
            "reflect": (d, n - 1 - d)}[mode][0 if low else 1]


def most_width(mode, n: int):
    """Largest admissible width for ``mode`` on an axis of n cells (None = whatever fits the array)."""
    return {"periodic": n, "symmetric": n, "reflect": n - 1}.get(mode)


def admissible(modes, widths, domain) -> bool:
    for axis, mode in enumerate(modes):
        most = most_width(mode, domain[axis])
        if most is not None and max(widths[2 * axis: 2 * axis + 2]) > most:
            return False
    return True


def fill(a: np.ndarray, origin, domain, widths, modes, value=0, sides: int = ALL) -> None:
    """In place on the host array ``a`` (I, J, K).  ``widths`` = (lo_i, hi_i, lo_j, hi_j); ``modes`` = (mode_i, mode_j)."""
    assert admissible(modes, widths, domain), (modes, widths, domain)
    (oi, oj, ok), (ni, nj, nk) = origin, domain
    lo_i, hi_i, lo_j, hi_j = widths
    mode_i, mode_j = modes
    ks = slice(ok, ok + nk)
    js = slice(oj, oj + nj)
    if mode_i is not None:  # the I sides, rows of the domain only
        for low, width, bit in ((True, lo_i, I_LO), (False, hi_i, I_HI)):
            if not sides & bit:
                continue
            for d in range(1, width + 1):
                i = oi - d if low else oi + ni - 1 + d
                if mode_i == "constant":
                    a[i, js, ks] = value
                else:
                    a[i, js, ks] = a[oi + source_index(mode_i, low, d, ni), js, ks]
    if mode_j is not None:  # the J sides, over the padded I range: the corners come from what the I step left there
        pi = slice(oi - lo_i, oi + ni + hi_i)
        for low, width, bit in ((True, lo_j, J_LO), (False, hi_j, J_HI)):
            if not sides & bit:
                continue
            for d in range(1, width + 1):
                j = oj - d if low else oj + nj - 1 + d
                if mode_j == "constant":
                    a[pi, j, ks] = value
                else:
                    a[pi, j, ks] = a[pi, oj + source_index(mode_j, low, d, nj), ks]


def mode_pairs(with_none: bool = True):
    modes = MODES + ((None,) if with_none else ())
    return list(itertools.product(modes, modes))
