"""Directed float tables for the generated kernels (test infrastructure; imports no product code).

Four kinds of thing live here, shared by tests/test_float_tables.py (CPU) and tests/test_gpu_float_tables.py (GPU):

  palette / pairs        some 33 IEEE edge values per float dtype and all their ordered pairs, laid along I
  *_program / *_expected the GTScript text of a table program and its expected outputs in PLAIN NUMPY (neither oracle)
  special_arguments      arguments at poles, domain ends and overflow thresholds for the device-library builtins, and
                         `assert_same_class`: NaN, +-inf and +-0 must agree in class and sign, the rest within a bound in ulp
  truth                  tests/golden/math_truth.npz: 256 seeded arguments per function and dtype with the TRUE result
                         (mpmath, 200 bits; scripts/make_math_truth.py), `ulp_error` against it and `reference_error`, the
                         worst error numpy / scipy themselves make on the same points -- the device's bound is that + ULPS

The bound of a transcendental function is never taken from the device: it is the reference's own measured error plus the
ulps tests/test_math_builtins.py already grants between the device and the reference.
"""

from __future__ import annotations

import pathlib
import zlib
from fractions import Fraction

import numpy as np

FLOATS = ("float32", "float64")
TRUTH_FILE = pathlib.Path(__file__).parent / "golden" / "math_truth.npz"
ACCURACY_FILE = pathlib.Path(__file__).parent.parent / "profiles" / "math_builtins_accuracy.txt"
POINTS = 256
_QUIET = dict(all="ignore")


def table_domain(n: int):
    """`n` table entries along I; J and K of extent 2, so that a strip kernel's rows and levels are more than one."""
    return (n, 2, 2)


def along_i(values, dtype) -> np.ndarray:
    """`values` along I, the same on every row and level; padded with its first entry to a multiple of four, so that every row
    of a dense array starts on a 16-byte boundary and the host may launch the 16-byte-lane kernel."""
    line = np.asarray(values, dtype=dtype)
    line = np.concatenate([line, np.repeat(line[:1], -len(line) % 4)])
    return np.ascontiguousarray(np.broadcast_to(line[:, None, None], table_domain(len(line))))


# ---- palette ------------------------------------------------------------------------------------------------------------------
def palette(dtype) -> np.ndarray:
    dt = np.dtype(dtype).type
    fi = np.finfo(dt)
    sub, tiny, mx, eps = dt(fi.smallest_subnormal), dt(fi.tiny), dt(fi.max), dt(fi.eps)
    beyond = dt(2.0 ** fi.nmant)  # 2^23 / 2^52: from here on every value is a whole number
    with np.errstate(**_QUIET):
        vals = [s * dt(v) for v in (0.0, 0.5, 1, 1.5, 2.5, 3, 7) for s in (dt(1), dt(-1))]  # zeros and small numbers
        vals += [sub, -sub, dt(3) * sub, -(dt(3) * sub), tiny, -tiny, tiny * (dt(1) + eps)]  # subnormal boundary
        vals += [eps, dt(1) + eps]
        vals += [np.nextafter(dt(0.5), dt(0))]  # 0.49999997f / 0.49999999999999994: + 0.5 rounds up to 1
        vals += [beyond + dt(1), -(beyond + dt(1)), dt(2) * beyond]
        vals += [mx, -mx, mx / dt(3)]
        vals += [dt(np.inf), dt(-np.inf), dt(np.nan)]
    return np.asarray(vals, dtype=dt)


def pairs(dtype, dtype_b=None):
    """(a, b): every ordered pair of the palette(s), a changing slowest."""
    va, vb = palette(dtype), palette(dtype_b or dtype)
    return np.repeat(va, len(vb)), np.tile(vb, len(va))


def palette_census(dtype) -> dict:
    v = palette(dtype)
    tiny = np.finfo(v.dtype).tiny
    zero = v == 0
    return {"pos_zero": int((zero & ~np.signbit(v)).sum()), "neg_zero": int((zero & np.signbit(v)).sum()),
            "subnormal": int((~zero & (np.abs(v) < tiny)).sum()), "smallest_normal": int((np.abs(v) == tiny).sum()),
            "max": int((np.abs(v) == np.finfo(v.dtype).max).sum()), "pos_inf": int((v == np.inf).sum()),
            "neg_inf": int((v == -np.inf).sum()), "nan": int(np.isnan(v).sum()),
            "tie": int((np.abs(v[np.isfinite(v)]) % 1 == 0.5).sum()),
            "whole_beyond_mantissa": int((np.isfinite(v) & (np.abs(v) > 2.0 ** np.finfo(v.dtype).nmant) & (np.abs(v) < 2.0 ** 60)).sum())}


def pair_census(dtype) -> dict:
    """How often the pair table reaches the corners the operator table is for."""
    a, b = pairs(dtype)
    tiny = np.finfo(a.dtype).tiny
    fa, fb = np.isfinite(a), np.isfinite(b)
    with np.errstate(**_QUIET):
        q, p = a / b, a * b
        zeros = (a == 0) & (b == 0) & (np.signbit(a) != np.signbit(b))
        return {"subnormal quotient": int((fa & fb & (q != 0) & (np.abs(q) < tiny)).sum()),
                "overflowing product": int((fa & fb & np.isinf(p)).sum()),
                "x % +-inf": int((fa & np.isinf(b)).sum()), "x % +-0": int((fa & (b == 0)).sum()),
                "min / max of (-0, +0)": int((zeros & np.signbit(a)).sum()), "min / max of (+0, -0)": int((zeros & np.signbit(b)).sum()),
                "NaN on the left": int((np.isnan(a) & ~np.isnan(b)).sum()), "NaN on the right": int((~np.isnan(a) & np.isnan(b)).sum())}


# ---- part 1: the operator table ---------------------------------------------------------------------------------------------
def _raz(x):  # gtc/ufuncs.py's spelling of round_away_from_zero
    return np.copysign(np.floor(np.abs(x) + x.dtype.type(0.5)), x)


#: name -> (GTScript expression, the same in numpy); every result has the operands' dtype
BINARY = {
    "o_add": ("a + b", np.add), "o_sub": ("a - b", np.subtract), "o_mul": ("a * b", np.multiply), "o_div": ("a / b", np.true_divide),
    "o_rem": ("a % b", np.remainder), "o_min": ("min(a, b)", np.minimum), "o_max": ("max(a, b)", np.maximum),
    "o_mod": ("mod(a, b)", np.remainder), "o_sel": ("a if a > b else b", lambda a, b: np.where(a > b, a, b)),
}
UNARY = {
    "o_neg": ("-a", np.negative), "o_abs": ("abs(a)", np.abs), "o_floor": ("floor(a)", np.floor), "o_ceil": ("ceil(a)", np.ceil),
    "o_trunc": ("trunc(a)", np.trunc), "o_round": ("round(a)", np.round), "o_raz": ("round_away_from_zero(a)", _raz),
    "o_sqrt": ("sqrt(a)", np.sqrt), "o_sqrt_abs": ("sqrt(abs(a))", lambda a: np.sqrt(np.abs(a))),
}
BOOLS = {
    "c_gt": ("a > b", np.greater), "c_lt": ("a < b", np.less), "c_ge": ("a >= b", np.greater_equal), "c_le": ("a <= b", np.less_equal),
    "c_eq": ("a == b", np.equal), "c_ne": ("a != b", np.not_equal),
    "p_nan": ("isnan(a)", lambda a, b: np.isnan(a)), "p_inf": ("isinf(a)", lambda a, b: np.isinf(a)),
    "p_fin": ("isfinite(a)", lambda a, b: np.isfinite(a)), "p_nan_sub": ("isnan(a - b)", lambda a, b: np.isnan(a - b)),
    "p_inf_mul": ("isinf(a * b)", lambda a, b: np.isinf(a * b)), "p_fin_div": ("isfinite(a / b)", lambda a, b: np.isfinite(a / b)),
}


def _program(name, inputs, outputs, body, imports=()):
    sig = [f"{k}: Field[np.{d}]" for k, d in inputs.items()] + [f"{k}: Field[np.{d}]" for k, d in outputs.items()]
    head = "".join(f"    from __externals__ import {x}\n" for x in imports)
    return (f"\n\ndef {name}({', '.join(sig)}):\n{head}    with computation(PARALLEL), interval(...):\n"
            + "".join(f"        {ln}\n" for ln in body))


def operator_program(dtype: str, bools: bool):
    """(name, text, {output: dtype name}).  With the bool outputs the program has 1-byte fields and gets a point-per-thread
    kernel only; without them every array has 4- or 8-byte items and the host launches the 16-byte-lane kernel."""
    name = f"float_ops_{dtype}" + ("_all" if bools else "")
    outs = {k: dtype for k in list(BINARY) + list(UNARY)}
    body = [f"{k} = {e}" for k, (e, _) in {**BINARY, **UNARY}.items()]
    if bools:
        outs.update({k: "bool_" for k in BOOLS})
        body += [f"{k} = {e}" for k, (e, _) in BOOLS.items()]
    return name, _program(name, {"a": dtype, "b": dtype}, outs, body), outs


def operator_expected(a, b, bools: bool) -> dict:
    with np.errstate(**_QUIET):
        want = {k: f(a, b) for k, (_, f) in BINARY.items()}
        want.update({k: f(a) for k, (_, f) in UNARY.items()})
        if bools:
            want.update({k: f(a, b) for k, (_, f) in BOOLS.items()})
    return want


def mixed_program():
    """`a` float32, `b` float64: every binary operator computes in float64 after widening `a` exactly."""
    outs = {k: "float64" for k in BINARY}
    return "float_ops_mixed", _program("float_ops_mixed", {"a": "float32", "b": "float64"}, outs,
                                       [f"{k} = {e}" for k, (e, _) in BINARY.items()]), outs


def mixed_expected(a, b) -> dict:
    assert a.dtype == np.float32 and b.dtype == np.float64
    with np.errstate(**_QUIET):
        return {k: f(a.astype(np.float64), b) for k, (_, f) in BINARY.items()}


# ---- part 2: ** --------------------------------------------------------------------------------------------------------------
def pow_program(dtype: str):
    name = f"float_pow_{dtype}"
    return name, _program(name, {"a": dtype, "b": dtype}, {"o_pow": dtype}, ["o_pow = a ** b"]), {"o_pow": dtype}


def pow_expected(a, b):
    with np.errstate(**_QUIET):
        return np.power(a, b)


def special_pow(want) -> np.ndarray:
    """Where numpy's result is one of pow's IEEE special cases: NaN, +-inf, +-0 or exactly 1."""
    return ~np.isfinite(want) | (want == 0) | (want == 1)


def assert_pow(got, want, what: str, ulps: int = 4):
    """Special results: same class and sign (an exact 1 stays an exact 1).  Every other result within `ulps` eps of numpy's --
    what tests/test_math_builtins.py grants `**` -- where a subnormal result's unit is its spacing."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    special = special_pow(want)
    bad = special & ~_same_special(got, want)
    eps = np.finfo(want.dtype).eps
    with np.errstate(**_QUIET):
        unit = np.maximum(eps * np.abs(want), np.spacing(np.abs(want)))
        off = ~special & ~(np.isfinite(got) & (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulps * unit.astype(np.float64)))
    _report(bad | off, got, want, what, f"({int(bad.sum())} special cases, {int(off.sum())} beyond {ulps} eps)")


def representable_powers(dtype):
    """(bases, exponents, exact values) of the directed row: base ** n for whole n = 1..16, kept where the exact value -- computed
    with Python's fractions -- is a number of the dtype."""
    dt = np.dtype(dtype).type
    a, b, v = [], [], []
    for base in (0.5, -0.5, 1.5, -1.5, 3.0, -3.0, 10.0, 2.0 ** -30):
        for n in range(1, 17):
            exact = Fraction(base) ** n
            with np.errstate(**_QUIET):
                r = dt(float(exact)) if abs(exact) < Fraction(float(np.finfo(dt).max)) else dt(np.inf)
            if np.isfinite(r) and Fraction(float(r)) == exact:
                a.append(base), b.append(float(n)), v.append(r)
    return np.asarray(a, dt), np.asarray(b, dt), np.asarray(v, dt)


# ---- part 3: literals --------------------------------------------------------------------------------------------------------
def literal_program(dtype: str):
    """(name, text, outputs, externals, {output: numpy value}).  The externals are numpy scalars of the dtype, so the literal has
    the field's dtype; `-0.0` is spelled in the text and is a float64 literal, so its two outputs are float64 in both programs."""
    dt = np.dtype(dtype).type
    fi = np.finfo(dt)
    ext = {"C_NAN": dt(np.nan), "C_PINF": dt(np.inf), "C_NINF": dt(-np.inf), "C_SUB": dt(fi.smallest_subnormal),
           "C_MAX": dt(fi.max), "C_TENTH": dt(0.1)}
    outs, body, consts = {}, [], {}
    for k, v in ext.items():
        outs[f"s_{k.lower()}"] = outs[f"l_{k.lower()}"] = dtype
        body += [f"s_{k.lower()} = a + {k}", f"l_{k.lower()} = {k}"]
        consts[k.lower()] = v
    outs["s_negzero"] = outs["l_negzero"] = "float64"
    body += ["s_negzero = a + -0.0", "l_negzero = -0.0"]
    consts["negzero"] = np.float64(-0.0)
    name = f"float_literals_{dtype}"
    return name, _program(name, {"a": dtype}, outs, body, imports=tuple(ext)), outs, ext, consts


def literal_expected(a, consts) -> dict:
    want = {}
    with np.errstate(**_QUIET):
        for k, v in consts.items():
            wide = np.result_type(a.dtype, v.dtype)
            want[f"s_{k}"] = a.astype(wide) + v.astype(wide)
            want[f"l_{k}"] = np.full(a.shape, v, dtype=v.dtype)
    return want


# ---- parts 4 and 5: the device-library builtins ------------------------------------------------------------------------------
#: the transcendental builtins and sqrt (`**` and `%`, the other two device-library calls, are parts 1 and 2)
BUILTINS = ("sin", "cos", "tan", "asin", "acos", "atan", "sinh", "cosh", "tanh", "asinh", "acosh", "atanh", "sqrt", "exp", "log",
            "log10", "cbrt", "gamma", "erf", "erfc")
ULPS = {"gamma": 16, "tan": 8, "erfc": 32}  # tests/test_math_builtins.py's table; everything else 4


def reference(name):
    """The function the reference's numpy backend binds to a builtin (gtc/ufuncs.py)."""
    if name in ("gamma", "erf", "erfc"):
        import scipy.special

        return getattr(scipy.special, name)
    return {"asin": np.arcsin, "acos": np.arccos, "atan": np.arctan, "asinh": np.arcsinh, "acosh": np.arccosh,
            "atanh": np.arctanh}.get(name) or getattr(np, name)


def builtin_program(dtype: str):
    name = f"float_builtins_{dtype}"
    outs = {f"y_{f}": dtype for f in BUILTINS}
    return name, _program(name, {"x": dtype}, outs, [f"y_{f} = {f}(x)" for f in BUILTINS]), outs


def _flip(f, lo, hi, pred):
    """Neighbouring floats (x, y) between lo and hi (same sign, pred(f(lo)) false, pred(f(hi)) true) with pred(f(x)) false and
    pred(f(y)) true: bisection on the integer view, which orders floats of one sign by magnitude."""
    dt = lo.dtype.type
    ut = {4: np.uint32, 8: np.uint64}[lo.dtype.itemsize]
    sign = dt(-1) if lo < 0 else dt(1)
    i, j = int(np.abs(lo).view(ut)), int(np.abs(hi).view(ut))
    assert i < j and not pred(f(lo)) and pred(f(hi))
    while j - i > 1:
        m = (i + j) // 2
        x = sign * np.asarray(m, dtype=ut).view(lo.dtype)[()]
        if pred(f(x)):
            j = m
        else:
            i = m
    return sign * np.asarray(i, dtype=ut).view(lo.dtype)[()], sign * np.asarray(j, dtype=ut).view(lo.dtype)[()]


def special_arguments(dtype) -> np.ndarray:
    """The union of the special arguments of every builtin; each function is run at all of them."""
    dt = np.dtype(dtype).type
    fi = np.finfo(dt)
    sub, tiny, eps, one = dt(fi.smallest_subnormal), dt(fi.tiny), dt(fi.eps), dt(1)
    v = [dt(0.0), dt(-0.0), dt(np.inf), dt(-np.inf), dt(np.nan), one, -one, sub, -sub, tiny, -tiny]
    v += [one + eps, -(one + eps), one - eps, -(one - eps), np.nextafter(one, dt(0)), dt(0.5), dt(-0.5), dt(2), dt(-2)]  # domain ends
    v += [dt(-2.5), dt(-3), dt(171), dt(172), dt(35), dt(36)]  # gamma: poles, a negative argument, the last finite factorials
    v += [dt(c) for c in (8, -8, 27, -27, 64, 125, 343, 1000, 1e9)]  # perfect cubes
    with np.errstate(**_QUIET):
        flips = [(np.exp, dt(1), dt(fi.max), np.isinf), (np.exp, dt(-1), dt(-fi.max), lambda y: y == 0),
                 (np.exp, dt(-1), dt(-fi.max), lambda y: y < tiny),  # the first subnormal result
                 (np.sinh, dt(1), dt(fi.max), np.isinf), (np.cosh, dt(1), dt(fi.max), np.isinf),
                 (reference("gamma"), dt(1), dt(1000), np.isinf), (reference("erfc"), dt(1), dt(1000), lambda y: y == 0),
                 (reference("erfc"), dt(1), dt(1000), lambda y: y < tiny)]
        for f, lo, hi, pred in flips:
            x, y = _flip(f, lo, hi, pred)
            more = [np.nextafter(x, dt(0)), x, y, np.nextafter(y, y * dt(2))]
            v += more + ([-m for m in more] if f in (np.sinh, np.cosh) else [])
    return np.asarray(v, dtype=dt)


def _same_special(got, want) -> np.ndarray:
    """Elementwise: NaN where NaN, the same infinity, a zero of the same sign, the same bits otherwise."""
    with np.errstate(**_QUIET):
        return np.where(np.isnan(want), np.isnan(got), (got == want) & (np.signbit(got) == np.signbit(want)))


def _report(bad, got, want, what, counts="", x=None):
    if bad.any():
        idx = np.argwhere(bad)[:8]
        rows = "; ".join((f"x = {float(x[tuple(i)]).hex()}: " if x is not None else f"{tuple(int(n) for n in i)}: ")
                         + f"got {float(got[tuple(i)]).hex()} want {float(want[tuple(i)]).hex()}" for i in idx)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ {counts}; first: {rows}")


def assert_same_class(got, want, x, bound_ulp: float, what: str):
    """Where `want` is NaN, +-inf or +-0, `got` must be the same class and sign; where it is finite and non-zero, `got` must be
    finite and within `bound_ulp` units in the last place of it."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    special = ~np.isfinite(want) | (want == 0)
    bad = special & ~_same_special(got, want)
    with np.errstate(**_QUIET):
        err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
        off = ~special & ~(np.isfinite(got) & (err <= bound_ulp))
    _report(bad | off, got, want, what, f"({int(bad.sum())} in class or sign, {int(off.sum())} beyond {bound_ulp:.1f} ulp)", x)


# ---- part 5: arguments over the whole range, the truth, and errors in ulp ---------------------------------------------------
def _log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _signed(rng, v):
    return v * rng.choice([-1.0, 1.0], len(v))


def _near_half_pi_multiples(rng, dt, n):
    """Floats of the dtype next to multiples of pi / 2: the zeros of sin and cos, the poles of tan."""
    k = np.concatenate([np.arange(1, 9), rng.integers(9, 2 ** 20, n)])[:n].astype(np.float64)
    near = (k * (np.pi / 2)).astype(dt)
    step = rng.integers(-1, 2, n)
    out = np.where(step < 0, np.nextafter(near, dt(0)), np.where(step > 0, np.nextafter(near, dt(np.inf)), near))
    return _signed(rng, out.astype(np.float64))


def arguments(name: str, dtype) -> np.ndarray:
    """POINTS seeded arguments of the dtype on which the true result is finite: the whole range, log-uniform in magnitude, and
    dense where the function has a zero or a pole."""
    dt = np.dtype(dtype).type
    fi = np.finfo(dt)
    f32 = dt is np.float32
    rng = np.random.default_rng(zlib.crc32(f"truth {name} {np.dtype(dtype).name}".encode()))
    n, h, q = POINTS, POINTS // 2, POINTS // 4
    tiny, sub, mx, eps = float(fi.tiny), float(fi.smallest_subnormal), float(fi.max), float(fi.eps)
    top = 3e38 if f32 else 1e300
    exp_hi, exp_lo = (88.72, -103.9) if f32 else (709.78, -745.1)  # exp: largest finite result, smallest non-zero one
    if name in ("sin", "cos", "tan"):
        x = np.concatenate([_signed(rng, _log_uniform(rng, tiny, 1e22, 96)), _signed(rng, _log_uniform(rng, 1.0, top, 96)),
                            _near_half_pi_multiples(rng, dt, 64)])
    elif name in ("atan", "asinh", "cbrt"):
        x = _signed(rng, _log_uniform(rng, sub if name == "cbrt" else tiny, top if name == "atan" else mx, n))
    elif name in ("asin", "acos", "atanh"):
        x = _signed(rng, np.concatenate([_log_uniform(rng, tiny, 1.0, h), 1.0 - _log_uniform(rng, eps / 2, 0.5, h)]))
        if name == "atanh":
            x = np.clip(x, -float(np.nextafter(dt(1), dt(0))), float(np.nextafter(dt(1), dt(0))))
    elif name in ("sinh", "cosh"):
        x = _signed(rng, np.concatenate([_log_uniform(rng, tiny, exp_hi, h), rng.uniform(0, exp_hi, h)]))
    elif name == "tanh":
        x = _signed(rng, np.concatenate([_log_uniform(rng, tiny, 20.0, h), rng.uniform(0, 20.0, h)]))
    elif name == "acosh":
        x = np.concatenate([1.0 + _log_uniform(rng, eps, 1.0, h), _log_uniform(rng, 1.0, mx, h)])
    elif name == "sqrt":
        x = _log_uniform(rng, sub, mx, n)
    elif name == "exp":
        x = np.concatenate([_signed(rng, _log_uniform(rng, tiny, exp_hi, h)), rng.uniform(exp_lo, exp_hi, h)])
    elif name in ("log", "log10"):
        x = np.concatenate([_log_uniform(rng, sub, mx, h), 1.0 + _signed(rng, _log_uniform(rng, eps, 0.5, h))])
    elif name == "gamma":
        over = 35.0 if f32 else 171.6
        x = np.concatenate([_log_uniform(rng, tiny, over, h), rng.uniform(0.0, over, h)])
    elif name == "erf":
        x = _signed(rng, np.concatenate([_log_uniform(rng, tiny, 6.0, h), rng.uniform(0, 6.0, h)]))
    elif name == "erfc":
        under = 10.0 if f32 else 27.2  # erfc: the smallest non-zero result
        x = np.concatenate([_log_uniform(rng, tiny, under, h), rng.uniform(-6.0, under, h)])
    else:
        raise ValueError(name)
    x = x.astype(dt)
    assert x.shape == (POINTS,) and np.isfinite(x).all(), name
    return x


def mp_truth(name: str, x, prec: int = 200):
    """(hi, lo) float64 arrays: hi the correctly rounded true value of the builtin at the float64 numbers `x`, lo the rest
    (true - hi, rounded).  Exact rationals carry the rounding, so subnormal results round once."""
    import mpmath

    with mpmath.workprec(prec):
        f = getattr(mpmath, name)
        if name == "cbrt":  # (mpmath's is the principal complex root of a negative number)
            f = lambda v: mpmath.sign(v) * mpmath.cbrt(abs(v))  # noqa: E731
        hi, lo = np.empty(len(x)), np.empty(len(x))
        for n, v in enumerate(np.asarray(x, dtype=np.float64)):
            p, q = mpmath.libmp.to_rational(mpmath.mpf(f(mpmath.mpf(float(v))))._mpf_)
            t = Fraction(p, q)
            hi[n] = float(t)  # int / int: correctly rounded
            lo[n] = float(t - Fraction(hi[n]))
    return hi, lo


_TRUTH = {}


def truth(name: str, dtype):
    """(x, hi, lo) from the fixture; for float32 `hi` is the float64 value of the truth and lo is zeros."""
    if not _TRUTH:
        with np.load(TRUTH_FILE) as z:
            _TRUTH.update({k: z[k] for k in z.files})
    key = f"{name}_{np.dtype(dtype).name}"
    x, hi = _TRUTH[key + "_x"], _TRUTH[key + "_hi"]
    return x, hi, _TRUTH.get(key + "_lo", np.zeros_like(hi))


def ulp_error(got, hi, lo) -> np.ndarray:
    """|got - true| in units of the spacing of the dtype of `got` at |true|: a subnormal result is measured in subnormal
    spacings.  (got - hi is exact in float64 wherever the error is small.)"""
    got = np.asarray(got)
    with np.errstate(**_QUIET):
        unit = np.spacing(np.abs(hi.astype(got.dtype))).astype(np.float64)
        err = np.abs((got.astype(np.float64) - hi) - lo) / unit
    return np.where(np.isfinite(got), err, np.inf)


def reference_error(name: str, dtype):
    """(worst error in ulp, its argument) of numpy / scipy, evaluated in the dtype, against the truth."""
    x, hi, lo = truth(name, dtype)
    with np.errstate(**_QUIET):
        err = ulp_error(reference(name)(x), hi, lo)
    n = int(np.argmax(err))
    return float(err[n]), x[n]


def bound(name: str, dtype) -> float:
    """What the device may be off by: the reference's own worst error plus the ulps granted between the two."""
    return reference_error(name, dtype)[0] + ULPS.get(name, 4)


def accuracy_row(name, dtype, device=None) -> str:
    ref, at = reference_error(name, dtype)
    dev = f"{device[0]:10.2f}  {float(device[1]).hex()}" if device else f"{'-':>10}  -"
    return f"{name:6} {np.dtype(dtype).name:8} {ref:10.2f}  {float(at).hex():26} {ref + ULPS.get(name, 4):10.2f} {dev}"


def recorded_accuracy() -> dict:
    """{(function, dtype): (reference's worst ulp, bound, device's worst ulp or None)} from profiles/math_builtins_accuracy.txt."""
    rows = {}
    for line in ACCURACY_FILE.read_text().splitlines():
        w = line.split()
        if len(w) >= 7 and not line.startswith("#"):
            rows[(w[0], w[1])] = (float(w[2]), float(w[4]), None if w[5] == "-" else float(w[5]))
    return rows
