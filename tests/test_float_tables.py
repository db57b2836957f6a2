"""CPU side of the directed float tables (tests/float_tables.py): a census of what the palette and its pairs reach, so that no
GPU case can pass for never meeting the case it names; every table program generated and compiled for gfx950; and the
self-check of tests/golden/math_truth.npz with the reference's own error against it (profiles/math_builtins_accuracy.txt)."""

import numpy as np
import pytest

import float_tables as ft
from test_fuzz_codegen import _load


def _parse(text, name, tmp_path, externals=None):
    from gt4py_amd.cartesian import definitions, frontend
    from gt4py_amd.cartesian.backend import hip_codegen

    defn = _load(text, name, tmp_path)
    st = frontend.parse_stencil(defn, externals=externals or {}, dtypes={},
                                options=definitions.BuildOptions(name=name, module=__name__, backend_opts={}))
    return hip_codegen.generate(st)


def _compiles(prog, name):
    from gt4py_amd import _lib

    return _lib.rtc_compile(prog.source, f"{name}.hip", ["-DGT4MI_UNIT_I_STRIDE=1", "-DGT4MI_NO_ALIAS=1"])[:4] == b"\x7fELF"


# ---- census -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ft.FLOATS)
def test_palette_holds_every_class(dtype):
    v = ft.palette(dtype)
    assert 30 <= len(v) <= 36 and len({x.tobytes() for x in v}) == len(v), len(v)  # some 33 distinct values
    census = ft.palette_census(dtype)
    print(dtype, len(v), census)
    assert all(n >= 1 for n in census.values()), census
    assert census["nan"] == 1  # one NaN: about 6 % of the pairs hold one
    fi = np.finfo(dtype)
    assert v.dtype.type(0.5) + np.nextafter(v.dtype.type(0.5), v.dtype.type(0)) == 1  # the value round_away_from_zero's spelling trips on
    assert fi.eps in v and 1 + fi.eps in v and fi.max / v.dtype.type(3) in v and 3 * fi.smallest_subnormal in v


@pytest.mark.parametrize("dtype", ft.FLOATS)
def test_pair_table_reaches_the_corners_it_is_for(dtype):
    a, b = ft.pairs(dtype)
    assert 900 <= len(a) <= 1300
    census = ft.pair_census(dtype)
    print(dtype, len(a), census)
    assert all(n >= 1 for n in census.values()), census
    share = float((np.isnan(a) | np.isnan(b)).mean())
    assert 0.04 < share < 0.08, share


@pytest.mark.parametrize("dtype", ft.FLOATS)
def test_nan_results_are_at_most_a_quarter_of_any_compared_output(dtype):
    """... with one exception that the palette forces and the test names: `sqrt(a)` is NaN for every negative non-zero `a`, a
    third of the palette -- asserted to be exactly those, which is the domain check of sqrt; `sqrt(abs(a))` is the output that
    exercises its rounding and is held to the quarter like the rest."""
    a, b = ft.pairs(dtype)
    want = ft.operator_expected(a, b, bools=True)
    want["o_pow"] = ft.pow_expected(a, b)
    if dtype == "float32":
        a32, b64 = ft.pairs("float32", "float64")
        want.update({f"mixed {k}": v for k, v in ft.mixed_expected(a32, b64).items()})
    for k, v in want.items():
        if v.dtype.kind == "f" and k != "o_sqrt":
            assert np.isnan(v).mean() <= 0.25, (k, float(np.isnan(v).mean()))
    np.testing.assert_array_equal(np.isnan(want["o_sqrt"]), np.isnan(a) | (a < 0))
    assert np.isnan(want["o_sqrt"]).mean() < 0.45
    special = ft.special_pow(want["o_pow"])
    assert 0.3 < special.mean() < 0.9, float(special.mean())  # both kinds of `**` result are well represented


@pytest.mark.parametrize("dtype", ft.FLOATS)
def test_numpy_emulation_of_the_device_helpers_agrees_with_the_ufuncs(dtype):
    """gt_min / gt_max / gt_mod as the PRELUDE spells them, evaluated in numpy with an exact fmod, against np.minimum / np.maximum /
    np.remainder on every pair: a mismatch on the GPU is then the device's, not the spelling's."""
    from edge_values import same_bits

    a, b = ft.pairs(dtype)
    dt = a.dtype.type
    with np.errstate(all="ignore"):
        nan = np.isnan(a) | np.isnan(b)
        same_bits(np.where(nan, a + b, np.where(a < b, a, b)), np.minimum(a, b), "gt_min")
        same_bits(np.where(nan, a + b, np.where(a > b, a, b)), np.maximum(a, b), "gt_max")
        m = np.fmod(a, b)
        adjusted = np.where(m != 0, np.where((b < 0) != (m < 0), m + b, m), np.copysign(dt(0), b))
        same_bits(np.where(b == 0, m, adjusted).astype(dt), np.remainder(a, b), "gt_mod")


def test_representable_powers_row():
    for dtype in ft.FLOATS:
        a, b, v = ft.representable_powers(dtype)
        assert len(a) >= 60 and (v != 0).all() and np.isfinite(v).all()
        assert any(x == 0.5 and n == 4 for x, n in zip(a, b))  # the cell the typed fuzzer met
        assert not any(x == 10 and n == 16 for x, n in zip(a, b)) if dtype == "float32" else True  # 1e16 has no float32
    a, b, v = ft.representable_powers("float64")
    np.testing.assert_array_equal(np.power(a, b), v)  # the host's pow is exact there, as the PRELUDE says


# ---- every program of the tables is generated and compiles for gfx950 ---------------------------------------------------------------
@pytest.mark.parametrize("dtype", ft.FLOATS)
def test_operator_programs_compile_and_get_both_kernel_kinds(dtype, tmp_path):
    """The program with the bool outputs has a point-per-thread kernel only (1-byte fields), the one without has a 16-byte-lane
    `_vec` kernel: between them both kernel kinds run the table."""
    kinds = {}
    for bools in (True, False):
        name, text, _ = ft.operator_program(dtype, bools)
        prog = _parse(text, name, tmp_path)
        assert len(prog.kernels) == 1 and prog.kernels[0].mapping == "ijk"
        kinds[bools] = prog.kernels[0].vec
        for call in ("gt_min(", "gt_max(", "gt_mod(", "gt_round(", "gt_round_away_from_zero(", "gt_sqrt(", "gt_floor("):
            assert call in prog.source, call
        if bools:
            assert all(f"gt_{c}(" in prog.source for c in ("isnan", "isinf", "isfinite"))
        assert _compiles(prog, name)
    assert kinds[True] == 0 and kinds[False] == 16 // np.dtype(dtype).itemsize, kinds


def test_mixed_program_compiles_with_a_vector_kernel(tmp_path):
    name, text, _ = ft.mixed_program()
    prog = _parse(text, name, tmp_path)
    assert prog.kernels[0].vec == 2 and "(double)" in prog.source
    assert _compiles(prog, name)


@pytest.mark.parametrize("dtype", ft.FLOATS)
def test_pow_literal_and_builtin_programs_compile(dtype, tmp_path):
    name, text, _ = ft.pow_program(dtype)
    prog = _parse(text, name, tmp_path)
    assert "gt_pow(" in prog.source and _compiles(prog, name)
    name, text, outs, ext, _ = ft.literal_program(dtype)
    prog = _parse(text, name, tmp_path, externals=ext)
    assert prog.source.count("__builtin_nan") >= 2 and prog.source.count("__builtin_inf") >= 4 and "-(0x0.0p+0)" in prog.source, prog.source
    assert _compiles(prog, name)
    name, text, _ = ft.builtin_program(dtype)
    prog = _parse(text, name, tmp_path)
    assert all(f"gt_{f}(" in prog.source for f in ft.BUILTINS) and _compiles(prog, name)


@pytest.mark.parametrize("dtype", ft.FLOATS)
def test_special_arguments_hold_what_each_builtin_needs(dtype):
    x = ft.special_arguments(dtype)
    dt = x.dtype.type
    fi = np.finfo(dt)
    assert len(x) < 128
    have = {v.tobytes() for v in x}
    for v in (0.0, -0.0, np.inf, -np.inf, 1, -1, fi.smallest_subnormal, -fi.smallest_subnormal, fi.tiny, -fi.tiny, 1 + fi.eps,
              -(1 + fi.eps), 1 - fi.eps, -2.5, 171, 172, 35, 36, 27, -27):
        assert dt(v).tobytes() in have, v
    assert np.isnan(x).sum() == 1
    with np.errstate(all="ignore"):
        for name, kinds in (("exp", (np.inf, 0.0)), ("sinh", (np.inf, -np.inf)), ("cosh", (np.inf,)), ("gamma", (np.inf,)), ("erfc", (0.0,))):
            y = ft.reference(name)(x)
            for k in kinds:  # the threshold: both sides of it are in the table, next to each other
                at = np.flatnonzero((y == k) & np.isfinite(x) & (np.abs(x) > 2))
                assert len(at) >= 1, (name, k)
                assert any(np.isfinite(ft.reference(name)(np.nextafter(x[i], dt(0)))) and ft.reference(name)(np.nextafter(x[i], dt(0))) != k
                           for i in at), (name, k)
        sub = ft.reference("exp")(x)
        assert ((sub > 0) & (sub < fi.tiny)).any() and ((ft.reference("erfc")(x) > 0) & (ft.reference("erfc")(x) < fi.tiny)).any()


# ---- the fixture ------------------------------------------------------------------------------------------------------------
def test_truth_fixture_shapes_and_arguments():
    assert ft.TRUTH_FILE.stat().st_size < 1 << 20
    for name in ft.BUILTINS:
        for dtype in ft.FLOATS:
            x, hi, lo = ft.truth(name, dtype)
            assert x.dtype == np.dtype(dtype) and x.shape == hi.shape == lo.shape == (ft.POINTS,), (name, dtype)
            assert hi.dtype == lo.dtype == np.float64 and np.isfinite(hi).all() and np.isfinite(x).all(), (name, dtype)
            np.testing.assert_array_equal(x, ft.arguments(name, dtype), err_msg=f"{name} {dtype}: the fixture's arguments are the seeded ones")
            with np.errstate(all="ignore"):
                assert (np.abs(lo) <= np.spacing(np.abs(hi)) / 2).all(), (name, dtype)  # hi is the nearest double
    # the ranges reach what they are for
    fi = np.finfo(np.float64)
    assert np.abs(ft.truth("sin", "float64")[0]).max() > 1e290 and np.abs(ft.truth("sin", "float32")[0]).max() > 1e37
    assert np.abs(ft.truth("tan", "float64")[1]).max() > 1e8  # next to a pole
    assert (np.abs(ft.truth("exp", "float64")[1]) < fi.tiny).any() and (ft.truth("erfc", "float64")[1] < 1e-300).any()
    assert np.abs(ft.truth("log", "float64")[1]).min() < 1e-12 and ft.truth("acosh", "float64")[1].min() < 1e-6
    assert ft.truth("gamma", "float64")[1].max() > 1e300 and ft.truth("exp", "float64")[1].max() > 1e280


def test_truth_is_the_correctly_rounded_value_on_a_regenerated_sample():
    """Where mpmath is importable: every 16th point of every function again at 400 bits, as exact rationals."""
    pytest.importorskip("mpmath")
    for name in ft.BUILTINS:
        for dtype in ft.FLOATS:
            x, hi, lo = ft.truth(name, dtype)
            again_hi, again_lo = ft.mp_truth(name, x[::16], prec=400)
            np.testing.assert_array_equal(hi[::16], again_hi, err_msg=f"{name} {dtype}")
            if dtype == "float64":
                np.testing.assert_allclose(lo[::16], again_lo, rtol=1e-12, atol=2.0 ** -140 * np.abs(hi[::16]).max(), err_msg=f"{name} {dtype}")


def test_reference_error_rows_are_recorded():
    """numpy / scipy against the truth, per function and dtype: printed, and the same as the rows of
    profiles/math_builtins_accuracy.txt.  The device's bound is this error plus ULPS -- the contract "within ULPS of the reference"
    restated against the truth -- so the reference's own error, 368 ulp for scipy's float64 erfc near its underflow, cannot fail a
    device that is accurate, and the device is never measured against itself."""
    rows = ft.recorded_accuracy()
    assert set(rows) == {(n, d) for n in ft.BUILTINS for d in ft.FLOATS}
    for name in ft.BUILTINS:
        for dtype in ft.FLOATS:
            print(ft.accuracy_row(name, dtype))
            worst, _ = ft.reference_error(name, dtype)
            assert np.isfinite(worst), (name, dtype)
            ref, bound, device = rows[(name, dtype)]
            assert abs(ref - worst) <= 0.006 and abs(bound - ft.bound(name, dtype)) <= 0.006, (name, dtype, ref, worst)
            assert device is None or device <= bound, (name, dtype, device, bound)
    assert ft.reference_error("sqrt", "float64")[0] <= 0.5 and ft.reference_error("sqrt", "float32")[0] <= 0.5  # correctly rounded
