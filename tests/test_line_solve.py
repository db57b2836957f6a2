"""``gt4py_amd.linesolve`` without a GPU: the contract's restatement (tests/line_solve_ref.py) against ``numpy.linalg.solve`` on
the dense matrix and on cases whose answer is known exactly, every refusal of the C entry through the dry run (made-up addresses
that are never dereferenced), the declaration, the kernels' resources and the Python interface's argument checks.

The restatement against numpy, float64, seeded systems with n = 1 .. 64, periodic and not, |b| >= 2 (|a| + |c|): the largest
relative error max|x - x_numpy| / max|x_numpy| of a line is 4.452e-16 (MEASURED_WORST below; the run is deterministic, the
test asserts 16 times that, which only absorbs another LAPACK build)."""

import ctypes

import numpy as np
import pytest

import entry_checks as E
import line_solve_ref as R
from entry_checks import INV, OOB, UNS, as_arg, int64s
from gt4py_amd import _lib, linesolve

HOST = (8, 9, 5)  # the shape of a host field where a test states none
MEASURED_WORST = 4.452e-16


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _system(rng, n, dtype=np.float64):
    """A diagonally dominant line: |b| >= 2 (|a| + |c|), signs mixed."""
    a, c, d = (rng.uniform(-1, 1, n) for _ in range(3))
    b = (2.0 * (np.abs(a) + np.abs(c)) + rng.uniform(0.1, 1, n)) * rng.choice([-1.0, 1.0], n)
    return tuple(v.astype(dtype) for v in (a, b, c, d))


def _worst_against_numpy():
    rng = np.random.default_rng(20240)
    worst = 0.0
    for n in range(1, 65):
        for periodic in (False, True):
            if periodic and n < 3:
                continue
            for _ in range(4):
                a, b, c, d = _system(rng, n)
                x = R.solve(a, b, c, d, periodic)
                want = np.linalg.solve(R.dense(a, b, c, periodic), d)
                worst = max(worst, float(np.max(np.abs(x - want)) / np.max(np.abs(want))))
    return worst


def test_the_restatement_against_numpy_on_the_dense_matrix():
    worst = _worst_against_numpy()
    print(f"restatement against numpy.linalg.solve: worst relative error {worst:.3e}")
    assert worst <= 16 * MEASURED_WORST


def test_a_diagonal_system_with_powers_of_two_is_exact():
    rng = np.random.default_rng(1)
    for dtype in (np.float32, np.float64):
        for n in (1, 2, 3, 17):
            d = rng.uniform(-1, 1, (n, 5)).astype(dtype)
            b = (2.0 ** rng.integers(-6, 7, (n, 5)) * rng.choice([-1.0, 1.0], (n, 5))).astype(dtype)
            zero = np.zeros_like(b)
            assert R.same_bits(R.solve(zero, b, zero, d), d / b).all()
    # a[0] and c[n-1] are never read without the closure: NaN there changes nothing
    a, b, c, d = _system(rng, 9)
    x = R.solve(a, b, c, d)
    a[0] = c[8] = np.nan
    assert R.same_bits(R.solve(a, b, c, d), x).all()


def test_the_periodic_restatement_on_a_shift_invariant_system_gives_the_shifted_solution():
    """Constant coefficients: the cyclic matrix commutes with the shift, so the solution of the shifted right-hand side is the
    shifted solution -- within the bound of the numpy comparison."""
    rng = np.random.default_rng(2)
    worst = 0.0
    for n in (3, 4, 17, 64):
        for _ in range(8):
            av, cv = rng.uniform(-1, 1, 2)
            bv = 2.0 * (abs(av) + abs(cv)) + rng.uniform(0.1, 1)
            a, b, c = (np.full(n, v) for v in (av, bv, cv))
            d = rng.uniform(-1, 1, n)
            x = R.solve(a, b, c, d, periodic=True)
            for s in (1, n // 2, n - 1):
                xs = R.solve(a, b, c, np.roll(d, s), periodic=True)
                worst = max(worst, float(np.max(np.abs(xs - np.roll(x, s))) / np.max(np.abs(x))))
    assert worst <= 16 * MEASURED_WORST, worst


def test_solve_along_moves_the_line_axis_and_broadcasts_1d_coefficients():
    rng = np.random.default_rng(3)
    d = rng.uniform(-1, 1, (4, 5, 6)).astype(np.float32)
    for axis in range(3):
        n = d.shape[axis]
        a, b, c, _ = _system(rng, n, np.float32)
        x = R.solve_along(a, b, c, d, axis, periodic=True)
        assert x.dtype == np.float32 and x.shape == d.shape
        line = np.moveaxis(d, axis, 0)[:, 1, 2]
        assert R.same_bits(np.moveaxis(x, axis, 0)[:, 1, 2], R.solve(a, b, c, line, True)).all()


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_header_signature_and_the_abi_is_still_8():
    E.check_binding("gt4mi_line_solve",
                    ["const gt4mi_field* out", "const gt4mi_field* rhs", "int nfields", "const gt4mi_field* lower", "const gt4mi_field* diag",
                     "const gt4mi_field* upper", "const int64_t extent[3]", "int axis", "int elem_size", "int flags", "void* workspace",
                     "int64_t workspace_bytes", "void* stream", "int64_t* workspace_needed", "int* path", "int* launches"],
                    prefix="LINE", constants=("PERIODIC", "DRY_RUN", "PATH_LANES", "PATH_TILES", "PATH_ITEMS"),
                    phrases=("den = b[m] - a[m] * cp[m-1]", "gamma = -b[0]", "(alpha * beta) / gamma", "no reciprocal", "No pivoting", "in-place"))


OUT, RHS, LO, DI, UP, WS = 0x10_0000, 0x4000_0000, 0x8000_0000, 0xA000_0000, 0xC000_0000, 0xE000_0000  # made-up addresses, far apart
SHAPE = (6, 7, 5)


def _field(ptr, shape=SHAPE, *rest, **kwargs):  # (this file's shape)
    return E.field(ptr, shape, *rest, **kwargs)


def _call(out, rhs, lo, di, up, nfields=1, extent=(4, 5, 5), axis=0, size=8, flags=0, ws=None, ws_bytes=0):
    rc, msg, needed, path, launches = E.call("gt4mi_line_solve", as_arg(out), as_arg(rhs), nfields, as_arg(lo), as_arg(di), as_arg(up),
                                             int64s(extent), axis, size, flags | _lib.LINE_DRY_RUN, ws, ws_bytes, None,
                                             outs=(ctypes.c_int64(-7), 77, 77))
    return rc, msg, launches, needed, path


def _good():
    return [_field(OUT), _field(RHS), _field(LO), _field(DI), _field(UP)]


def test_every_refusal_of_the_c_entry_without_a_gpu():
    """Every check runs before the first launch: these calls carry made-up device addresses and the dry-run flag."""
    rc, msg, launches, needed, path = _call(*_good())
    # 5 x 5 lines of 4 points along I: rows of 32 doubles
    assert rc == 0 and launches == 1 and needed == 32 * 4 * 8 and path == _lib.LINE_PATH_TILES, msg
    rc, msg, launches, needed, path = _call(*_good(), flags=_lib.LINE_PERIODIC)
    assert rc == 0 and launches == 1 and needed == 2 * 32 * 4 * 8, msg
    for axis, lines, n, want in ((1, 20, 5, _lib.LINE_PATH_LANES), (2, 20, 5, _lib.LINE_PATH_LANES)):
        rc, msg, launches, needed, path = _call(*_good(), axis=axis)
        assert rc == 0 and needed == 32 * n * 8 and path == want, msg
    for size in (4, 8):
        args = [_field(p, itemsize=size) for p in (OUT, RHS, LO, DI, UP)]
        rc, msg, launches, needed, _ = _call(*args, size=size, flags=_lib.LINE_PERIODIC)
        assert rc == 0 and launches == 1 and needed == 2 * (256 // size) * 4 * size, msg
    # null pointers
    for n, what in enumerate((b"out is null", b"rhs is null", b"lower is null", b"diag is null", b"upper is null")):
        args = _good()
        args[n] = None
        rc, msg, launches, needed, path = _call(*args)
        assert rc == INV and what in msg and launches == 0 and needed == 0 and path == -1, msg
    rc, msg, *_ = _call(*_good(), extent=None)
    assert rc == INV and b"extent is null" in msg
    for n, what in enumerate((b"out 0 is null", b"rhs 0 is null", b"lower 0 is null", b"diag 0 is null", b"upper 0 is null")):
        args = _good()
        args[n] = _field(0)
        rc, msg, launches, *_ = _call(*args)
        assert rc == INV and what in msg and launches == 0, msg
    # counts, extents, axis, flags, item size
    for n in (0, -2):
        rc, msg, launches, *_ = _call(*_good(), nfields=n)
        assert rc == INV and b"nfields" in msg and launches == 0
    rc, msg, *_ = _call(*_good(), extent=(4, -1, 5))
    assert rc == INV and b"invalid extent -1 along axis 1" in msg
    for axis in (-1, 3):
        rc, msg, *_ = _call(*_good(), axis=axis)
        assert rc == INV and b"axis" in msg and b"is not 0 (I), 1 (J) or 2 (K)" in msg
    rc, msg, *_ = _call(*_good(), flags=2)
    assert rc == INV and b"flags" in msg
    for size in (2, 16):
        rc, msg, *_ = _call(*_good(), size=size)
        assert rc == UNS and b"item size %d" % size in msg
    # periodic needs three points
    for axis, extent in ((0, (2, 5, 5)), (1, (4, 1, 5)), (2, (4, 5, 2))):
        rc, msg, launches, *_ = _call(*_good(), extent=extent, axis=axis, flags=_lib.LINE_PERIODIC)
        assert rc == INV and b"at least 3 points" in msg and launches == 0, msg
        rc, msg, *_ = _call(*_good(), extent=extent, axis=axis)
        assert rc == 0, msg
    rc, msg, *_ = _call(*_good(), extent=(3, 5, 5), flags=_lib.LINE_PERIODIC)
    assert rc == 0, msg
    # a box that does not fit its field, per role and axis
    rc, msg, launches, *_ = _call(*_good(), extent=(6, 5, 5))
    assert rc == OOB and b"out 0" in msg and b"axis 0" in msg and launches == 0
    for n, what in enumerate((b"out 0", b"rhs 0", b"lower 0", b"diag 0", b"upper 0")):
        args = [_field(p, (8, 9, 6)) for p in (OUT, RHS, LO, DI, UP)]
        args[n] = _field(args[n].data, SHAPE)
        for axis, extent in ((1, (4, 7, 5)), (2, (4, 5, 6))):
            rc, msg, *_ = _call(*args, extent=extent)
            assert rc == OOB and what in msg and b"axis %d" % axis in msg, msg
    rc, msg, *_ = _call(_field(OUT), _field(RHS, origin=(1, -1, 0)), _field(LO), _field(DI), _field(UP))
    assert rc == OOB and b"negative origin -1 along axis 1" in msg
    # strides and alignment
    rc, msg, *_ = _call(_field(OUT, strides=(8, 52, 336)), *_good()[1:])
    assert rc == UNS and b"multiple of the item size" in msg
    rc, msg, *_ = _call(_field(OUT), _field(RHS), _field(LO), _field(DI + 4), _field(UP))
    assert rc == UNS and b"diag 0 is not aligned to its item size" in msg
    rc, msg, launches, *_ = _call(_field(OUT, strides=(0, 8, 56)), *_good()[1:])
    assert rc == INV and b"out 0 has stride 0 along axis 0" in msg and launches == 0
    rc, msg, *_ = _call(_field(OUT), _field(RHS, strides=(8, 0, 0)), _field(LO), _field(DI), _field(UP))
    assert rc == 0, msg  # a rhs may be broadcast
    # 1-d coefficients along the line axis: broadcast, exempt from the shape check on the other axes, n items needed
    for axis in range(3):
        n = (4, 5, 5)[axis]
        rc, msg, launches, *_ = _call(_field(OUT), _field(RHS), E.line(LO, n, axis), E.line(DI, n, axis), E.line(UP, n, axis), axis=axis)
        assert rc == 0 and launches == 1, msg
        rc, msg, *_ = _call(_field(OUT), _field(RHS), E.line(LO, n, axis), E.line(DI, n - 1, axis), E.line(UP, n, axis), axis=axis)
        assert rc == OOB and b"diag 0" in msg and b"axis %d" % axis in msg, msg
    rc, msg, *_ = _call(_field(OUT), _field(RHS), E.line(LO, 5, 1), _field(DI), _field(UP), axis=0)  # 1-d along the wrong axis
    assert rc == OOB and b"lower 0" in msg
    # the workspace: too small, misaligned, over a field; absent is fine in a dry run
    _, _, _, needed, _ = _call(*_good())
    rc, msg, launches, *_ = _call(*_good(), ws=WS, ws_bytes=needed - 1)
    assert rc == INV and b"workspace of %d bytes is too small, %d are needed" % (needed - 1, needed) in msg and launches == 0
    rc, msg, *_ = _call(*_good(), ws=WS + 4, ws_bytes=needed)
    assert rc == UNS and b"workspace is not aligned" in msg
    rc, msg, launches, *_ = _call(*_good(), ws=WS, ws_bytes=needed)
    assert rc == 0 and launches == 1, msg
    first = 8 * (1 + 6)  # byte offset of the box's first item
    for n, what in enumerate((b"workspace overlaps out 0", b"workspace overlaps rhs 0", b"workspace overlaps lower", b"workspace overlaps diag",
                              b"workspace overlaps upper")):
        base = (OUT, RHS, LO, DI, UP)[n]
        rc, msg, launches, *_ = _call(*_good(), ws=base + first + 8, ws_bytes=needed)
        assert rc == UNS and what in msg and launches == 0, msg
        rc, msg, *_ = _call(*_good(), ws=base + first - needed, ws_bytes=needed)  # ends where the box starts
        assert rc == 0, msg
    # overlap in memory: an out against a shifted rhs, another pair's rhs, a coefficient, another out
    rc, msg, launches, *_ = _call(_field(OUT), _field(OUT + 8), _field(LO), _field(DI), _field(UP))
    assert rc == UNS and b"out 0 and rhs 0 overlap in memory" in msg and launches == 0
    rc, msg, *_ = _call(_field(OUT), _field(OUT, (6, 7, 5), (8, 56, 336)), _field(LO), _field(DI), _field(UP))  # the same start, another pitch
    assert rc == UNS and b"out 0 and rhs 0 overlap in memory" in msg
    for n, what in ((2, b"out 0 and lower overlap"), (3, b"out 0 and diag overlap"), (4, b"out 0 and upper overlap")):
        args = _good()
        args[n] = _field(OUT)
        rc, msg, *_ = _call(*args)
        assert rc == UNS and what in msg, msg
    rc, msg, *_ = _call(_field(OUT), _field(RHS), E.line(LO, 4, 0), E.line(OUT + 80, 4, 0), E.line(UP, 4, 0))
    assert rc == UNS and b"out 0 and diag overlap in memory" in msg
    two = lambda a, b: E.table((a, b))  # noqa: E731
    rc, msg, *_ = _call(two(_field(OUT), _field(OUT + 0x10000)), two(_field(RHS), _field(OUT)), _field(LO), _field(DI), _field(UP), nfields=2)
    assert rc == UNS and b"out 0 and rhs 1 overlap in memory" in msg
    rc, msg, *_ = _call(two(_field(OUT), _field(OUT + 64)), two(_field(RHS), _field(RHS + 0x10000)), _field(LO), _field(DI), _field(UP), nfields=2)
    assert rc == UNS and b"out 0 and out 1 overlap in memory" in msg
    rc, msg, *_ = _call(two(_field(OUT), _field(OUT)), two(_field(OUT), _field(OUT)), _field(LO), _field(DI), _field(UP), nfields=2)
    assert rc == UNS and b"overlap in memory" in msg  # in place twice over one array
    # THE allowed overlap: out[n] is rhs[n], the same box; one rhs for two outs is fine as well
    rc, msg, launches, *_ = _call(_field(OUT), _field(OUT), _field(LO), _field(DI), _field(UP))
    assert rc == 0 and launches == 1, msg
    rc, msg, *_ = _call(two(_field(OUT), _field(OUT + 0x10000)), two(_field(OUT), _field(OUT + 0x10000)), _field(LO), _field(DI), _field(UP), nfields=2)
    assert rc == 0, msg
    rc, msg, *_ = _call(two(_field(OUT), _field(OUT + 0x10000)), two(_field(RHS), _field(RHS)), _field(LO), _field(DI), _field(UP), nfields=2)
    assert rc == 0, msg
    rc, msg, *_ = _call(_field(OUT), _field(RHS), _field(LO), _field(LO), _field(LO))  # coefficients may be one array
    assert rc == 0, msg
    # an extent with a zero entry: OK, nothing to launch -- after the checks
    rc, msg, launches, needed, _ = _call(*_good(), extent=(4, 0, 5))
    assert rc == 0 and launches == 0 and needed == 0, msg
    rc, msg, launches, *_ = _call(*_good(), extent=(7, 0, 5))
    assert rc == OOB and launches == 0


def test_a_call_without_a_workspace_is_refused_before_any_launch():
    lib = _lib.load()
    args = _good()
    rc = lib.gt4mi_line_solve(*[ctypes.byref(f) for f in args[:2]], 1, *[ctypes.byref(f) for f in args[2:]], (ctypes.c_int64 * 3)(4, 5, 5), 0, 8, 0,
                              None, 0, None, None, None, None)
    assert rc == INV and b"workspace is null" in lib.gt4mi_last_error()


def test_launches_are_one_per_eight_pairs_and_the_path_follows_the_strides():
    o = E.table(_field(OUT + n * 0x10000) for n in range(9))
    r = E.table(_field(RHS + n * 0x10000) for n in range(9))
    assert [_call(o, r, _field(LO), _field(DI), _field(UP), nfields=n)[2] for n in (1, 3, 8, 9)] == [1, 1, 1, 2]
    c_order = lambda p: _field(p, strides=(7 * 5 * 8, 5 * 8, 8))  # noqa: E731
    L, T, IT = _lib.LINE_PATH_LANES, _lib.LINE_PATH_TILES, _lib.LINE_PATH_ITEMS
    for axis, want in ((0, L), (1, L), (2, T)):
        assert _call(*[c_order(p) for p in (OUT, RHS, LO, DI, UP)], axis=axis)[4] == want
    for axis in range(3):  # fields that disagree: item by item
        assert _call(_field(OUT), c_order(RHS), _field(LO), _field(DI), _field(UP), axis=axis)[4] == IT
        assert _call(_field(OUT), _field(RHS), _field(LO), c_order(DI), _field(UP), axis=axis)[4] == IT
    # 1-d coefficients keep the path of the fields; a line of one point has no run to tile
    assert _call(_field(OUT), _field(RHS), E.line(LO, 4, 0), E.line(DI, 4, 0), E.line(UP, 4, 0), axis=0)[4] == T
    assert _call(_field(OUT), _field(RHS), E.line(LO, 5, 1), E.line(DI, 5, 1), E.line(UP, 5, 1), axis=1)[4] == L
    assert _call(*_good(), extent=(1, 5, 5), axis=0)[4] == IT


def test_the_kernels_are_in_the_resource_log_without_scratch():
    kernels = E.kernel_resources(r"line_solve\S*kernel")
    # 2 dtypes x the register budgets for 1, 4 and 8 entries x (lanes, items, tiles)
    assert len(kernels) == 18 and len({name for name, *_ in kernels}) == 18, kernels
    for name, scratch, waves, lds in kernels:
        assert int(scratch) == 0 and int(waves) >= 1, (name, scratch, waves, lds)
        assert (int(lds) > 0) == ("tile" in name) and int(lds) <= 36 * 1024, (name, lds)


# ---- the Python interface: every refusal before any GPU work ---------------------------------------------------------------
def _args(**over):
    args = dict(out=E.host_field(HOST), rhs=E.host_field(HOST), lower=E.host_field(HOST), diag=E.host_field(HOST), upper=E.host_field(HOST))
    args.update(over)
    return args.pop("out"), args.pop("rhs"), args


@pytest.mark.parametrize("kwargs, error, match", [
    (dict(halo=2.0), ValueError, "halo must be"),
    (dict(halo=-1), ValueError, "must not be negative"),
    (dict(halo=5), ValueError, "leave no domain"),
    (dict(halo=2, origin=(1, 2, 0)), ValueError, "negative origin -1 along axis 0"),
    (dict(origin=(0, 0, 0, 0)), ValueError, "at most three entries"),
    (dict(origin=(0, 0, 5)), ValueError, "leave no domain"),
    (dict(axis="X"), ValueError, "axis must be one of"),
    (dict(axis=0), ValueError, "axis must be one of"),
    (dict(periodic=True, upper=E.host_field((2,)), origin=(6, 0, 0)), ValueError, "at least 3 points"),
    (dict(periodic=True), TypeError, "device fields"),  # all checks passed: refused for being host memory
    (dict(), TypeError, "device fields"),
])
def test_python_refusals_need_no_gpu(kwargs, error, match):
    out, rhs, rest = _args()
    rest.update(kwargs)
    with pytest.raises(error, match=match):
        linesolve.solve_lines(out, rhs, **rest)
    with pytest.raises(error, match=match):
        linesolve.LineSolve([out], [rhs], **rest)


def test_python_refusals_about_the_fields_themselves():
    import torch

    S = linesolve.solve_lines
    out, rhs, rest = _args()
    with pytest.raises(ValueError, match="at least one"):
        S([], [], **rest)
    with pytest.raises(ValueError, match="2 out field.s. and 1 rhs field.s. were passed"):
        S([out, E.host_field(HOST)], [rhs], **rest)
    with pytest.raises(TypeError, match="host"):
        S(torch.zeros(8, 9, 5, dtype=torch.float64), rhs, **rest)  # as_device_array's own refusal
    with pytest.raises(TypeError):
        S(out, np.zeros((8, 9, 5)), **rest)
    with pytest.raises(TypeError):
        S(out, rhs, lower=np.zeros(8), diag=rest["diag"], upper=rest["upper"])
    with pytest.raises(ValueError, match="takes IJK fields"):
        S(E.host_field((8, 9)), rhs, **rest)
    with pytest.raises(ValueError, match="diag must be an IJK field or a 1-d array along I"):
        S(out, rhs, lower=rest["lower"], diag=E.host_field((8, 9)), upper=rest["upper"])
    # one dtype for everything, float32 or float64
    with pytest.raises(TypeError, match="share a dtype"):
        S(out, E.host_field(HOST, dtype="float32"), **rest)
    with pytest.raises(TypeError, match="share a dtype"):
        S(out, rhs, lower=rest["lower"], diag=rest["diag"], upper=E.host_field((8,), "float32"))
    ints = {k: E.host_field(v.shape, "int64") for k, v in rest.items()}
    with pytest.raises(TypeError, match="float32 or float64 fields"):
        S(E.host_field(HOST, dtype="int64"), E.host_field(HOST, dtype="int64"), **ints)
    # coefficient shapes: a 1-d array holds exactly n items along the line axis; IJK arrays agree along it
    rest = dict(rest, upper=E.host_field((8,)))
    with pytest.raises(TypeError, match="device fields"):
        S(out, rhs, **rest)
    with pytest.raises(ValueError, match="upper has 8 items, a line of 9 points along J needs 9"):
        S(out, rhs, axis="J", **rest)
    with pytest.raises(ValueError, match="upper has 8 items, a line of 10 points along I needs 10"):
        S(E.host_field((10, 9, 5)), E.host_field((10, 9, 5)), lower=E.host_field((10, 9, 5)), diag=E.host_field((10, 9, 5)), upper=rest["upper"], halo=1)
    with pytest.raises(ValueError, match="share their length along I: 8 and 10 differ"):
        S(out, E.host_field((10, 9, 5)), **rest)
    with pytest.raises(TypeError, match="device fields"):  # along J and K the smaller array sets the domain
        S(out, E.host_field((8, 11, 6)), **rest)
    # overlaps come from the library: a field as its own coefficient; in place is fine up to the device check
    with pytest.raises(TypeError, match="out 0 and diag overlap in memory"):
        S(out, rhs, lower=rest["lower"], diag=out, upper=rest["upper"])
    with pytest.raises(TypeError, match="out 0 and rhs 1 overlap in memory"):
        S([out, E.host_field(HOST)], [rhs, out], **rest)
    with pytest.raises(TypeError, match="device fields"):
        S(out, out, **rest)


def test_a_frozen_solve_knows_its_box_and_refuses_to_run_after_an_array_died(monkeypatch):
    """The weak references are taken last, behind the device check: what they guard is shown on a LineSolve whose device check
    is made to pass for host memory -- the call itself is never reached, the dead reference is found first."""
    E.on_device(monkeypatch)
    outs, rhss = [E.host_field((10, 9, 5), "float32") for _ in range(9)], [E.host_field((12, 9, 5), "float32") for _ in range(9)]
    a, b, c = E.host_field((10, 9, 5), "float32"), E.host_field((9,), "float32"), E.host_field((9,), "float32")
    ls = linesolve.LineSolve(outs, rhss, lower=a, diag=b, upper=c, axis="J", periodic=True, halo=1)
    assert (ls.n, ls.lines, ls.launches, ls.extent, ls.domain, ls.origin, ls.axis, ls.periodic, ls.path) == \
        (9, 50, 2, (10, 9, 5), (8, 7, 5), (1, 1, 0), "J", True, "lanes")
    assert ls.workspace.shape == (2 * 64 * 9,) and ls.workspace.dtype == np.float32  # cp and q: rows of 64 items for 50 lines
    del c
    E.refuses_a_dead_array(ls)
