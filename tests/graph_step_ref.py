"""The numpy chain of the composed model step of tests/test_gpu_graph_replay.py: nothing but a composition of the restatements the
suite already has (boundary_ref, the oracle's Laplacian, line_solve_ref, stats_ref, level_stats_ref, histogram_ref, line_find_ref).
tests/test_graph_step_ref.py checks on the CPU that it is no vacuous reference.  Test infrastructure; torch-free."""

from __future__ import annotations

import numpy as np

import boundary_ref
import histogram_ref
import level_stats_ref
import line_find_ref
import line_solve_ref
import stats_ref
from oracle import ref_numpy as ORACLE

HALO, DOMAIN = 2, (70, 35, 9)
SHAPE = (DOMAIN[0] + 2 * HALO, DOMAIN[1] + 2 * HALO, DOMAIN[2])
ORIGIN = (HALO, HALO, 0)
BOX = tuple(slice(o, o + d) for o, d in zip(ORIGIN, DOMAIN))
MODES = ("periodic", "zero_gradient")
EDGES = np.linspace(-30.0, 30.0, 25)
LEVEL = 0.0        # the columns of a random state cross it almost everywhere, and not at one place
MISSING = -1.0     # (finite: the last stencil multiplies by the position)
SEED = 31


def inputs(dtype, seed=SEED):
    """(the state with its ghost cells, the three 1-d coefficients along K: diagonally dominant, so the solve damps)."""
    rng = np.random.default_rng([seed, np.dtype(dtype).itemsize])
    state = rng.uniform(-1, 1, SHAPE).astype(dtype)
    nk = DOMAIN[2]
    lower, upper = rng.uniform(-1, 1, nk), rng.uniform(-1, 1, nk)
    diag = (4.0 + rng.uniform(0, 1, nk)) * rng.choice([-1.0, 1.0], nk)
    return state, [v.astype(dtype) for v in (lower, diag, upper)]


def step(state, coefs):
    """One step from ``state`` (never changed): the new state and everything the step leaves behind."""
    s = state.copy()
    boundary_ref.fill(s, ORIGIN, DOMAIN, (HALO,) * 4, MODES)
    lap = np.zeros_like(s)  # (the literal -4.0 in the fields' precision: the stencil is built with literal_float_precision to match)
    ORACLE.laplacian(s, lap, origin_inp=ORIGIN, origin_out=ORIGIN, domain=DOMAIN)
    s[BOX] = line_solve_ref.solve_along(*coefs, lap[BOX], 2, False)
    box = s[BOX]
    found = line_find_ref.find_along(box, 2, "crossing", LEVEL, "any", False, None, MISSING)  # (3, ni, nj)
    return {"state": s, "laplacian": lap[BOX], "stats": stats_ref.stats(box), "profile": level_stats_ref.profile(box),
            "counts": histogram_ref.count_box(box, EDGES, True), "found": found,
            "out": box.astype(np.float64) * found[0][:, :, None]}


def run(dtype, steps=3, seed=SEED):
    state, coefs = inputs(dtype, seed)
    out = []
    for _ in range(steps):
        out.append(step(state, coefs))
        state = out[-1]["state"]
    return out
