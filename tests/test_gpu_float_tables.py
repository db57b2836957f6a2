"""GPU side of the directed float tables (tests/float_tables.py): generated kernels at IEEE edge values.

1. every float operator, comparison, predicate and rounding builtin on all ordered pairs of the palette, bit for bit against
   numpy's ufuncs, through a point-per-thread kernel and through a 16-byte-lane kernel; float32 with float64 for the promotion
2. `**` on the same pairs: pow's IEEE special cases in class and sign, the rest within 4 eps; representable powers exactly
3. float literals the generator emits (NaN, infinities, hex floats, -0.0)
4. the device-library builtins at poles, domain ends and thresholds: the class and sign the reference's numpy backend gives
5. the same builtins over their whole range against true values (tests/golden/math_truth.npz): within the reference's own
   measured error plus the ulps tests/test_math_builtins.py grants

Expected values are plain numpy / scipy on the host; nothing comes from either oracle."""

import numpy as np
import pytest

import float_tables as ft
from edge_values import same_bits
from test_fuzz_codegen import _load

pytestmark = pytest.mark.gpu


def _run(text, name, arrays, tmp_path, externals=None):
    """({field: array after the call}, [label of the kernel twin each launch was])"""
    import gt4py_amd.storage as gt_storage
    from gt4py_amd.cartesian import gtscript

    hip = gtscript.stencil(backend="hip:mi300", definition=_load(text, name, tmp_path), externals=externals or {})
    dev = {k: gt_storage.from_array(v, dtype=v.dtype, backend="hip:mi300", aligned_index=(0, 0, 0)) for k, v in arrays.items()}
    cls = type(hip)
    cls._gt_launch_cache_.clear()  # the entry this call prepares is then the only one
    hip(**dev, origin=(0, 0, 0), domain=next(iter(arrays.values())).shape)
    (_, _, _, keep), = cls._gt_launch_cache_.values()
    return {k: v.get() for k, v in dev.items()}, [label for _, label in keep[3][1]]


def _outputs(outs, shape):
    return {k: np.zeros(shape, np.dtype(d.rstrip("_"))) for k, d in outs.items()}


def _compare(got, want, what):
    for k, v in want.items():
        if v.dtype == np.bool_:
            assert got[k].dtype == np.bool_
            np.testing.assert_array_equal(got[k], v, err_msg=f"{what}: {k}")
        else:
            same_bits(got[k], v, f"{what}: {k}")


# ---- 1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bools", [True, False], ids=["point", "vec"])
@pytest.mark.parametrize("dtype", ft.FLOATS)
def test_float_operator_table(dtype, bools, tmp_path):
    """All ordered pairs of the palette through + - * / % min max mod, the select, unary minus, abs, floor, ceil, trunc, round,
    round_away_from_zero and sqrt -- and, in the program that a point-per-thread kernel runs, the six comparisons and isnan /
    isinf / isfinite of an operand and of a difference, product and quotient: every float bit for bit (the sign of a zero
    counts, the payload of a NaN does not), every bool exactly.  hiprtc's default modes keep float32 subnormals and round
    division and sqrt correctly, or this fails."""
    pa, pb = ft.pairs(dtype)
    a, b = ft.along_i(pa, dtype), ft.along_i(pb, dtype)
    name, text, outs = ft.operator_program(dtype, bools)
    got, ran = _run(text, name, {"a": a, "b": b, **_outputs(outs, a.shape)}, tmp_path)
    assert ran == ["point" if bools else "vec"], ran
    _compare(got, {"a": a, "b": b, **ft.operator_expected(a, b, bools)}, f"{dtype} operators ({ran[0]})")


def test_float32_with_float64_operator_table(tmp_path):
    """`a` float32, `b` float64: the result is float64 and `a` is widened exactly (every float32 of the palette, subnormals and
    max among them, against float64's)."""
    pa, pb = ft.pairs("float32", "float64")
    a, b = ft.along_i(pa, "float32"), ft.along_i(pb, "float64")
    name, text, outs = ft.mixed_program()
    got, ran = _run(text, name, {"a": a, "b": b, **_outputs(outs, a.shape)}, tmp_path)
    assert ran == ["vec"], ran
    _compare(got, {"a": a, "b": b, **ft.mixed_expected(a, b)}, "float32 with float64")


# ---- 2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ft.FLOATS)
def test_pow_on_every_pair(dtype, tmp_path):
    """Where numpy's `a ** b` is NaN, +-inf, +-0 or exactly 1 -- x ** +-0, 1 ** NaN, (-1) ** +-inf, (+-0) ** negative odd, a negative
    base with a fractional exponent, overflow, underflow -- the device's is the same class and sign; every other pair within 4 eps."""
    pa, pb = ft.pairs(dtype)
    a, b = ft.along_i(pa, dtype), ft.along_i(pb, dtype)
    name, text, outs = ft.pow_program(dtype)
    got, _ = _run(text, name, {"a": a, "b": b, **_outputs(outs, a.shape)}, tmp_path)
    ft.assert_pow(got["o_pow"], ft.pow_expected(a, b), f"{dtype} a ** b")


@pytest.mark.parametrize("dtype", ft.FLOATS)
def test_representable_powers_are_exact(dtype, tmp_path):
    """(+-0.5, +-1.5, +-3, 10, 2^-30) ** (1 .. 16) wherever the exact value -- Python fractions -- is a number of the dtype: bit for
    bit.  float64 by the double-double path of gt_pow, float32 by its repeated multiplication in double, rounded once."""
    pa, pb, exact = ft.representable_powers(dtype)
    a, b = ft.along_i(pa, dtype), ft.along_i(pb, dtype)
    name, text, outs = ft.pow_program(dtype)
    got, _ = _run(text, name, {"a": a, "b": b, **_outputs(outs, a.shape)}, tmp_path)
    same_bits(got["o_pow"], ft.along_i(exact, dtype), f"{dtype} representable powers")


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ft.FLOATS)
def test_float_literals(dtype, tmp_path):
    """Externals NaN, +-inf, the smallest subnormal, max and 0.1 of the dtype, and `-0.0` as the text spells it, as `a + literal`
    and as a plain store."""
    a = ft.along_i(ft.palette(dtype), dtype)
    name, text, outs, ext, consts = ft.literal_program(dtype)
    got, _ = _run(text, name, {"a": a, **_outputs(outs, a.shape)}, tmp_path, externals=ext)
    _compare(got, ft.literal_expected(a, consts), f"{dtype} literals")


# ---- 4 and 5 ----------------------------------------------------------------------------------------------------------------
_RESULTS = {}


def _builtins(dtype, tmp_path):
    """Every builtin at the special arguments followed by the fixture's arguments of ALL functions, in one launch per dtype."""
    if dtype not in _RESULTS:
        x = ft.along_i(np.concatenate([ft.special_arguments(dtype)] + [ft.truth(f, dtype)[0] for f in ft.BUILTINS]), dtype)
        name, text, outs = ft.builtin_program(dtype)
        got, _ = _run(text, name, {"x": x, **_outputs(outs, x.shape)}, tmp_path)
        same_bits(got["x"], x, "the argument field is untouched")
        for k in outs:  # every row and level computed the same
            same_bits(got[k], np.broadcast_to(got[k][:, :1, :1], x.shape), f"{dtype} {k}: rows and levels")
        _RESULTS[dtype] = (x[:, 0, 0], {k: v[:, 0, 0] for k, v in got.items()})
    return _RESULTS[dtype]


@pytest.mark.parametrize("dtype", ft.FLOATS)
@pytest.mark.parametrize("name", ft.BUILTINS)
def test_builtin_at_special_arguments(name, dtype, tmp_path):
    """+-0, +-inf, NaN, +-1, subnormals, domain ends and one step beyond, overflow and underflow thresholds and one step either
    side, gamma's poles, perfect cubes: where numpy / scipy -- the reference's numpy backend -- give NaN, +-inf or +-0, the device
    gives the same class and sign; where they give a number, the device's is finite and within the function's bound."""
    x, got = _builtins(dtype, tmp_path)
    n = len(ft.special_arguments(dtype))
    with np.errstate(all="ignore"):
        want = ft.reference(name)(x[:n])
    ft.assert_same_class(got[f"y_{name}"][:n], want, x[:n], ft.bound(name, dtype), f"{dtype} {name}")


@pytest.mark.parametrize("dtype", ft.FLOATS)
@pytest.mark.parametrize("name", ft.BUILTINS)
def test_builtin_against_the_truth_over_its_range(name, dtype, tmp_path):
    """The device's worst error in ulp against the true value, printed with its argument, within the reference's own worst
    error on the same points + ULPS (see profiles/math_builtins_accuracy.txt for both columns)."""
    x, got = _builtins(dtype, tmp_path)
    at = len(ft.special_arguments(dtype)) + ft.POINTS * ft.BUILTINS.index(name)
    tx, hi, lo = ft.truth(name, dtype)
    same_bits(x[at: at + ft.POINTS], tx, "arguments")
    err = ft.ulp_error(got[f"y_{name}"][at: at + ft.POINTS], hi, lo)
    worst = int(np.argmax(err))
    print("\nACCURACY " + ft.accuracy_row(name, dtype, (float(err[worst]), tx[worst])))
    bound = ft.bound(name, dtype)
    assert err[worst] <= bound, (f"{dtype} {name}: {err[worst]:.2f} ulp at x = {float(tx[worst]).hex()} (device "
                                 f"{float(got[f'y_{name}'][at + worst]).hex()}, true {float(hi[worst]).hex()}); the reference's worst is "
                                 f"{bound - ft.ULPS.get(name, 4):.2f} ulp, the bound {bound:.2f}")
