"""The numpy chain of the composed model step (tests/graph_step_ref.py) at the shape the GPU test uses: it is no vacuous reference --
finite, not constant, changing from step to step, with positions that are found and counters that hold every item."""

import functools

import numpy as np
import pytest

import graph_step_ref as S


@functools.lru_cache(maxsize=None)
def _steps(dtype_name):
    return S.run(np.dtype(dtype_name).type)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_the_chain_is_finite_varies_and_moves_from_step_to_step(dtype):
    steps = _steps(dtype)
    assert len(steps) == 3
    for n, r in enumerate(steps):
        assert r["state"].shape == S.SHAPE and r["state"].dtype == np.dtype(dtype)
        for name in ("state", "laplacian", "stats", "profile", "out"):
            assert np.isfinite(r[name]).all(), (n, name)
        for name in ("state", "laplacian", "out"):
            assert np.ptp(r[name]) > 0, (n, name)
        # the ghost cells hold what the boundary condition says of the state the step STARTED from
        before = S.inputs(np.dtype(dtype).type)[0] if n == 0 else steps[n - 1]["state"]
        assert np.array_equal(r["state"][:S.HALO, S.BOX[1]], before[S.DOMAIN[0]:S.DOMAIN[0] + S.HALO, S.BOX[1]])  # periodic in I
    for a, b in zip(steps, steps[1:]):
        assert not np.array_equal(a["state"][S.BOX], b["state"][S.BOX])
        assert a["stats"].tobytes() != b["stats"].tobytes() and a["counts"].tobytes() != b["counts"].tobytes()
        assert not np.array_equal(a["found"][0], b["found"][0])


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_positions_are_found_and_the_counters_hold_every_item(dtype):
    ni, nj, nk = S.DOMAIN
    for n, r in enumerate(_steps(dtype)):
        position, _, crossings = r["found"]
        assert position.shape == (ni, nj)
        found = position != S.MISSING
        assert found.mean() > 0.5, (n, found.mean())  # most columns cross the level ...
        assert np.unique(position[found]).size > 100, n  # ... and not at one place
        assert ((position[found] >= 0) & (position[found] <= nk - 1)).all() and (crossings[found] >= 1).all()
        assert np.ptp(r["out"][found]) > 0
        counts = r["counts"]
        assert counts.shape == (nk, S.EDGES.size - 1 + 3) and (counts.sum(axis=1) == ni * nj).all(), n
        assert counts[:, :-3].sum() > 0.9 * ni * nj * nk, n  # (the edges hold the values: the bins say something)
        assert r["stats"][0] == ni * nj * nk and r["stats"][1] == 0
