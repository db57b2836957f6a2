"""Without a GPU: the edge-value fields of tests/edge_values.py reach the cases the GPU tests name (a CENSUS of the oracle alone), and
the expected values do not rest on one restatement (oracle.ref_numpy against the independent GTScript interpreter and against a
per-point restatement written here with numpy scalars).

Census of the committed seeds, domain (130, 20, 2), limiter on, coefficient field (float64 | float32 fields; nonfinite 0 %).
W is the dtype of lap / res / d: float64 unless the float32 literals (HDIFF_INTERNAL_F32) are asked for.
hdiff   regime fields  W    nonfinite | I: >0   <0  =0(res!=0) underflow | J: >0   <0  =0(res!=0) underflow | out: -0   +0 subnormal changed-by-limiter non-finite | f32 sums inf
        ties   float64 f64  0.00      |    4160  154     771         0  |    4323  170     819         0  |     250  378       0         3935            0.000  |     0
        ties   float64 f64  0.01      |    4001  213     717         0  |    4143  235     753         0  |     229  327       0         3592            0.099  |     0
        ties   float32 f64  0.00      |    4188  156     761         0  |    4339  157     803         0  |     232  409       0         3904            0.000  |     0
        ties   float32 f64  0.01      |    4037  225     688         0  |    4189  247     735         0  |     228  319       0         3594            0.090  |     0
        ties   float32 f32  0.00      |    4188  156     761         0  |    4339  157     803         0  |     232  409       0         3904            0.000  |     0
        ties   float32 f32  0.01      |    4037  225     688         0  |    4189  247     735         0  |     228  319       0         3594            0.090  |     0
        tiny   float64 f64  0.00      |    2496  900    1528      1023  |    2654  944    1541      1044  |     109  220     863         3129            0.000  |     0
        tiny   float64 f64  0.01      |    2525  917    1364       914  |    2675  931    1400       964  |      85  212     796         2913            0.102  |     0
        tiny   float32 f64  0.00      |    3382 1064     489         0  |    3540 1115     500         0  |     108  239    1029         3448            0.000  |     0
        tiny   float32 f64  0.01      |    3307 1056     427         0  |    3448 1045     491         0  |     131  196     994         3052            0.106  |     0
        tiny   float32 f32  0.00      |    2562  922    1444       961  |    2679  969    1504      1006  |      87  218     873         3218            0.000  |     0
        tiny   float32 f32  0.01      |    2497  911    1378       953  |    2579  894    1508      1019  |     113  181     834         2822            0.106  |     0
        huge   float64 f64  0.00      |    3126  557    1289         0  |    3265  605    1331         0  |     193  373       0         3138            0.126  |     0
        huge   float64 f64  0.01      |    3003  609    1218         0  |    3188  623    1204         0  |     151  294       0         2989            0.209  |     0
        huge   float32 f64  0.00      |    3162  577    1288         0  |    3292  599    1324         0  |     196  389       0         3146            0.027  |    60
        huge   float32 f64  0.01      |    3074  606    1146         0  |    3138  652    1246         0  |     181  330       0         2847            0.137  |    55
        huge   float32 f32  0.00      |    3158  574    1275         0  |    3289  596    1308         0  |     185  350       0         3190            0.130  |    60
        huge   float32 f32  0.01      |    3068  599    1128         0  |    3134  640    1229         0  |     171  295       0         2903            0.221  |    55
(5 240 I-fluxes and 5 460 J-fluxes, 5 200 outputs, 5 808 neighbour sums per case)
lap5    regime `ties0`, (-0, +0) outputs per variant 0-3, smallest over the three shapes, both shares of non-finite points and both literal precisions:
        float64: [(83, 1340), (83, 1340), (769, 625), (414, 1431)]
        float32: [(81, 1178), (81, 1178), (692, 567), (410, 1282)]; `huge`: variant 1 is inf where variant 0 is finite at 1 to 10 points
tridiag out / sup / rhs together: subnormal, inf, NaN, -0, +0, non-finite share
        float64 (17, 5, 5)   :    65   66    194    159    184 0.204
        float64 (66, 3, 57)  :  1487  173   7245   4376   5682 0.219
        float64 (66, 3, 121) :  2977  197  18042   9278  11431 0.254
        float64 (64, 3, 161) :  3920  155  21038  12306  15342 0.229
        float64 (66, 2, 100) :  1652  115   9345   5215   6377 0.239
        float32 (17, 5, 5)   :    59  106    258    134    138 0.285
        float32 (66, 3, 57)  :  2099  123   5699   4444   5229 0.172
        float32 (66, 3, 121) :  4329  172  17350   8719  10853 0.244
        float32 (64, 3, 161) :  5913  150  18217  11659  14782 0.198
        float32 (66, 2, 100) :  2468  125   8891   4998   5919 0.228
Floors asserted below: 50 of every flux class per direction, 50 outputs each of -0 and +0 (and subnormal in `tiny`), 20 outputs
that the limiter changes, 50 underflowing products per direction (`tiny`, W = float32 on float32 fields and float64 fields), 50
float32 neighbour sums that are inf while finite in float64 (`huge`); Laplacians: 50 outputs each of -0 and +0 per variant in
`ties0` (eight equally likely values give a -0 Laplacian once in 32768 points, see edge_values.LAP_REGIMES); tridiagonal solve:
50 each of subnormal, inf, NaN, -0, +0 over out / sup / rhs; and in EVERY case the GPU tests compare at most half of the outputs
are non-finite.
"""

import numpy as np
import pytest

import edge_values as E
import test_gpu_edge_values as GE  # (its cases and expected values; nothing in it touches the GPU at import)
from oracle import gtscript_interp as gi
from oracle import ref_numpy as R

DTYPES = [np.float64, np.float32]
DOMAIN = (130, 20, 2)


# ---- the comparer ------------------------------------------------------------------------------------------------------------
def test_same_bits_sees_what_array_equal_does_not():
    a = np.array([0.0, -0.0, 1.0, np.nan, np.inf, 5e-324])
    assert E.same_bits(a, a.copy())
    assert E.same_bits(a, np.array([0.0, -0.0, 1.0, -np.nan, np.inf, 5e-324]))  # sign / payload of a NaN: not compared
    assert np.array_equal(a, np.array([-0.0, 0.0, 1.0, np.nan, np.inf, 5e-324]), equal_nan=True)
    with pytest.raises(AssertionError, match=r"2 of 6 elements differ.*sign of zero 2, NaN against number 0, inf against finite 0, other 0"):
        E.same_bits(a, np.array([-0.0, 0.0, 1.0, np.nan, np.inf, 5e-324]))
    with pytest.raises(AssertionError, match=r"sign of zero 0, NaN against number 1, inf against finite 1, other 1.*got 0x0.0000000000001p-1022 \[0x1\] want 0x0.0000000000002p-1022 \[0x2\]"):
        E.same_bits(a, np.array([0.0, -0.0, np.nan, np.nan, 1.0, 1e-323]))
    with pytest.raises(AssertionError, match="dtype"):
        E.same_bits(a, a.astype(np.float32))
    with pytest.raises(AssertionError, match="shape"):
        E.same_bits(a, a[:5])
    f = np.array([[1.0, -0.0]], dtype=np.float32)
    with pytest.raises(AssertionError, match=r"\(0, 1\): got -0x0.0p\+0 \[0x80000000\] want 0x0.0p\+0 \[0x0\]"):
        E.same_bits(f, np.array([[1.0, 0.0]], dtype=np.float32))
    assert E.same_bits(f.T[::-1], f.T[::-1].copy())  # any strides


def test_fields_are_seeded_and_hold_only_their_palette():
    for regime in E.REGIMES + ("ties0",):
        for dtype in DTYPES:
            vals, prob = E.palette(regime, dtype)
            assert vals.dtype == dtype and abs(prob.sum() - 1) < 1e-12
            a = E.lap_field(regime, dtype, (40, 30, 2))
            assert E.differing_bits(a, E.lap_field(regime, dtype, (40, 30, 2))) == 0
            bits = {v.tobytes() for v in vals}
            assert {v.tobytes() for v in a.ravel()} == bits  # every value of the palette, and nothing else
            b = E.lap_field(regime, dtype, (40, 30, 2), 0.05)
            assert 0 < (~np.isfinite(b)).sum() < 0.1 * b.size and np.isnan(b).any() and (b == np.inf).any() and (b == -np.inf).any()


# ---- census: horizontal diffusion ----------------------------------------------------------------------------------------------
def _hdiff_census(regime, dtype, nonfinite, lit):
    u, c = E.hdiff_fields(regime, dtype, DOMAIN, nonfinite)
    W = np.float32 if (lit == 32 and dtype == np.float32) else np.float64
    on = GE._hdiff_want(u, c, DOMAIN, True, "field", lit, None)[2:-2, 2:-2]
    off = GE._hdiff_want(u, c, DOMAIN, False, "field", lit, None)[2:-2, 2:-2]
    return E.hdiff_flux_census(u, DOMAIN, W), E.classes(on), E.differing_bits(on, off)


@pytest.mark.parametrize("nonfinite", [0.0, 0.01])
@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("dtype,lit", [(np.float64, 64), (np.float32, 64), (np.float32, 32)])
def test_census_hdiff(dtype, lit, regime, nonfinite):
    flux, out, changed = _hdiff_census(regime, dtype, nonfinite, lit)
    print(f"{regime:5s} {np.dtype(dtype).name} W=f{lit} nonfinite {nonfinite}: I {flux['I']} J {flux['J']} out {out} limiter changes {changed} "
          f"f32 sums inf {flux['sum_inf_in_T_finite_in_f64']}")
    for axis in "IJ":
        assert min(flux[axis][k] for k in ("pos", "neg", "zero_res_nonzero")) >= 50, (axis, flux[axis])
        if regime == "tiny" and (dtype == np.float64 or lit == 32):
            assert flux[axis]["underflow"] >= 50, (axis, flux[axis])
    assert out["neg_zero"] >= 50 and out["pos_zero"] >= 50, out
    if regime == "tiny":
        assert out["subnormal"] >= 50, out
    assert changed >= 20
    if regime == "huge" and dtype == np.float32:
        assert flux["sum_inf_in_T_finite_in_f64"] >= 50
    assert out["nonfinite_share"] <= 0.5


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_at_most_half_of_every_compared_hdiff_output_is_nonfinite(dtype, regime):
    """Every case of test_gpu_edge_values.py: geometry, flag combination, share of non-finite points, special coefficients."""
    worst = 0.0
    for nonfinite in (0.0, 0.01):
        for domain, _ in GE._hdiff_geometries(dtype):
            u, c = E.hdiff_fields(regime, dtype, domain, nonfinite)
            for combo in GE._hdiff_combos(dtype):
                worst = max(worst, E.classes(GE._hdiff_want(u, c, domain, *combo)[2:-2, 2:-2])["nonfinite_share"])
    u, _ = E.hdiff_fields(regime, dtype, DOMAIN)
    c = E.special_coeff(dtype, u.shape, np.random.default_rng(11))
    special = E.classes(GE._hdiff_want(u, c, DOMAIN, True, "field", 64, None)[2:-2, 2:-2])
    assert min(special[k] for k in ("neg_zero", "pos_zero", "nan")) >= 50, special
    worst = max(worst, special["nonfinite_share"])
    for scalar in (-0.0, float(np.finfo(dtype).smallest_subnormal), 0.3):  # (a coefficient of inf makes every output non-finite:
        for sdt in (np.float64, np.float32):                               # that case is about inf * 0 = NaN, not about the cap)
            worst = max(worst, E.classes(GE._hdiff_want(u, c, DOMAIN, True, "scalar", 64, sdt, scalar)[2:-2, 2:-2])["nonfinite_share"])
    print(f"{regime} {np.dtype(dtype).name}: largest non-finite share of a compared output {worst:.3f}")
    assert worst <= 0.5


# ---- census: Laplacians -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_census_lap5(dtype):
    for shape in ((132, 22, 2), (515, 8, 2), (136, 48, 3)):  # the arrays of (130, 20, 2), (513, 6, 2) and the ring's (128, 40, 3)
        for regime in E.LAP_REGIMES:
            for nonfinite in (0.0, 0.01):
                inp = E.lap_field(regime, dtype, shape, nonfinite)
                for lit32 in (False, True) if dtype == np.float32 else (False,):
                    outs = [GE._lap_want(inp, v, lit32)[1:-1, 1:-1] for v in range(4)]
                    cl = [E.classes(o) for o in outs]
                    print(f"lap5 {np.dtype(dtype).name} literal32 {lit32} {shape} {regime} nonfinite {nonfinite}: (-0, +0, non-finite share) per variant "
                          f"{[(c['neg_zero'], c['pos_zero'], round(c['nonfinite_share'], 3)) for c in cl]}, v0 != v1 at {E.differing_bits(outs[0], outs[1])}")
                    assert all(c["nonfinite_share"] <= 0.5 for c in cl)
                    if regime == "ties0":
                        assert all(c["neg_zero"] >= 50 and c["pos_zero"] >= 50 for c in cl), cl
                    if regime == "huge" and dtype == np.float32 and not lit32:
                        # variant 0 widens every addend, variant 1 adds in float32 first: inf against finite
                        assert E.differing_bits(outs[0], outs[1]) > 0
                        assert (np.isinf(outs[1]) & np.isfinite(outs[0])).sum() > 0


# ---- census: tridiagonal solve ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_census_tridiag(dtype):
    for shape in GE.TRIDIAG_SHAPES + [(66, 2, 100)]:
        _, (s, r, o) = GE._tridiag_case(dtype, shape)
        cl = E.classes(np.concatenate([o.ravel(), s.ravel(), r.ravel()]))
        print(f"tridiag {np.dtype(dtype).name} {shape}: {cl}")
        assert min(cl[k] for k in ("subnormal", "inf", "nan", "neg_zero", "pos_zero")) >= 50, cl
        assert cl["nonfinite_share"] <= 0.5 and E.classes(o)["nonfinite_share"] <= 0.5
        inf, diag, sup, rhs = E.tridiag_fields(dtype, shape)
        assert (diag == 0).sum() > 0 and np.isfinite(np.concatenate([inf, diag, sup, rhs])).all()
        lo, hi = np.abs(diag[diag != 0]).min(), np.abs(diag).max()
        assert lo <= np.finfo(dtype).tiny * 2.0 ** 12 and hi == np.finfo(dtype).max / 4  # the wide-exponent palette, both ends


# ---- three restatements agree ----------------------------------------------------------------------------------------------------
SMALL = (20, 12, 2)


def _interp(definition, fields, scalars, domain, lit):
    from gt4py_amd.cartesian.backend import hip_templates

    gi.run(getattr(hip_templates, definition), fields, scalars, domain, literal_float=lit)


@pytest.mark.parametrize("nonfinite", [0.0, 0.01])
@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("dtype,lit", [(np.float64, 64), (np.float32, 64), (np.float32, 32)])
def test_hdiff_oracle_interpreter_and_scalar_restatement_agree(dtype, lit, regime, nonfinite):
    u, c = E.hdiff_fields(regime, dtype, SMALL, nonfinite)
    o = (2, 2, 0)
    for definition, limiter, kind in (("hdiff_limiter_field", True, "field"), ("hdiff_plain_field", False, "field"),
                                      ("hdiff_limiter_scalar", True, "scalar"), ("hdiff_plain_scalar", False, "scalar")):
        want = GE._hdiff_want(u, c, SMALL, limiter, kind, lit, np.float64)
        got = np.full(u.shape, GE.SENTINEL, dtype)
        fields = {"in_field": (u.copy(), o), "out_field": (got, o)}
        if kind == "field":
            fields["coeff"] = (c.copy(), o)
        _interp(definition, fields, {} if kind == "field" else {"coeff": GE.SCALAR}, SMALL, lit)
        E.same_bits(got, want, f"interpreter against ref_numpy: {definition} {regime}")
    # the limiter form with a coefficient field, point by point with numpy scalars of the dtypes the rules prescribe
    T = np.dtype(dtype).type
    W = np.float32 if (lit == 32 and dtype == np.float32) else np.float64
    want = GE._hdiff_want(u, c, SMALL, True, "field", lit, None)
    got = np.full(u.shape, GE.SENTINEL, dtype)
    with np.errstate(all="ignore"):
        def lap(a, b, k):
            s = ((u[a + 1, b, k] + u[a - 1, b, k]) + u[a, b + 1, k]) + u[a, b - 1, k]  # in T
            return (W(4.0) * W(u[a, b, k])) - W(s)

        def flux(a, b, k, da, db):
            res = lap(a + da, b + db, k) - lap(a, b, k)
            d = W(T(u[a + da, b + db, k] - u[a, b, k]))  # the difference in T, then widened
            return W(0) if (res * d) > W(0) else res

        for a in range(2, 2 + SMALL[0]):
            for b in range(2, 2 + SMALL[1]):
                for k in range(SMALL[2]):
                    s = ((flux(a, b, k, 1, 0) - flux(a - 1, b, k, 1, 0)) + flux(a, b, k, 0, 1)) - flux(a, b - 1, k, 0, 1)
                    got[a, b, k] = T(W(u[a, b, k]) - (W(c[a, b, k]) * s))
    E.same_bits(got, want, f"scalar restatement against ref_numpy: hdiff_limiter_field {regime}")


@pytest.mark.parametrize("dtype,lit", [(np.float64, 64), (np.float32, 64), (np.float32, 32)])
def test_lap5_expected_values_agree_with_the_interpreter(dtype, lit):
    for regime in E.LAP_REGIMES:
        for nonfinite in (0.0, 0.01):
            inp = E.lap_field(regime, dtype, (SMALL[0] + 2, SMALL[1] + 2, SMALL[2]), nonfinite)
            for variant, name in enumerate(GE.LAP_NAMES):
                want = GE._lap_want(inp, variant, lit == 32 and dtype == np.float32)
                E.same_bits(E.lap5_expected(inp, np.full(inp.shape, GE.SENTINEL, dtype), variant, lit == 32), want, "the two numpy forms")
                got = np.full(inp.shape, GE.SENTINEL, dtype)
                _interp("lap_" + name, {"inp": (inp.copy(), (1, 1, 0)), "out": (got, (1, 1, 0))}, {}, SMALL, lit)
                E.same_bits(got, want, f"interpreter against the numpy form: lap_{name} {regime} nonfinite {nonfinite}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_tridiag_oracle_interpreter_and_scalar_restatement_agree(dtype):
    shape = (6, 5, 12)
    T = np.dtype(dtype).type
    for seed in range(4):
        inf, diag, sup, rhs = E.tridiag_fields(dtype, shape, seed)
        s_w, r_w, o_w = sup.copy(), rhs.copy(), np.full(shape, GE.SENTINEL, dtype)
        R.tridiag(inf, diag, s_w, r_w, o_w)
        s_i, r_i, o_i = sup.copy(), rhs.copy(), np.full(shape, GE.SENTINEL, dtype)
        z = (0, 0, 0)
        _interp("tridiagonal_solver", {"inf": (inf.copy(), z), "diag": (diag.copy(), z), "sup": (s_i, z), "rhs": (r_i, z), "out": (o_i, z)}, {}, shape, 64)
        s_p, r_p, o_p = sup.copy(), rhs.copy(), np.full(shape, GE.SENTINEL, dtype)
        with np.errstate(all="ignore"):
            for i in range(shape[0]):
                for j in range(shape[1]):
                    a, d, s, r, o = inf[i, j], diag[i, j], s_p[i, j], r_p[i, j], o_p[i, j]
                    s[0] = T(s[0] / d[0])
                    r[0] = T(r[0] / d[0])
                    for k in range(1, shape[2]):
                        new_s = T(s[k] / T(d[k] - T(s[k - 1] * a[k])))
                        r[k] = T(T(r[k] - T(a[k] * r[k - 1])) / T(d[k] - T(s[k - 1] * a[k])))  # sup[k - 1] is still the old level's
                        s[k] = new_s
                    o[-1] = r[-1]
                    for k in range(shape[2] - 2, -1, -1):
                        o[k] = T(r[k] - T(s[k] * o[k + 1]))
        for name, want, interp, point in (("out", o_w, o_i, o_p), ("sup", s_w, s_i, s_p), ("rhs", r_w, r_i, r_p)):
            E.same_bits(interp, want, f"interpreter against ref_numpy: tridiag {name} seed {seed}")
            E.same_bits(point, want, f"scalar restatement against ref_numpy: tridiag {name} seed {seed}")
        cl = E.classes(np.concatenate([o_w.ravel(), s_w.ravel(), r_w.ravel()]))
        assert cl["nan"] > 0 and cl["inf"] > 0 and cl["subnormal"] > 0 and cl["nonfinite_share"] <= 0.5, cl
