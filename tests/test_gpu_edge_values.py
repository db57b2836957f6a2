"""GPU: every shipped path of the three kernel families -- and the generated kernels of the same definitions -- BIT FOR BIT against
the oracle on fields made of IEEE edge values (tests/edge_values.py): exact ties of the flux limiter, zeros of both signs,
subnormals, products that underflow, sums that overflow in float32 and not in float64, divisions by zero, inf / inf, and a sparse
share of NaN and infinities.  The comparison is `edge_values.same_bits` over the WHOLE array: the sign of a zero counts, and
everything outside the compute domain keeps its sentinel.  tests/test_edge_values.py (no GPU) asserts that these very fields reach
the cases named here, and that the expected values do not rest on one restatement.

Shapes are the smallest that still select each path: (130, 20, 2) runs the LDS-sharing strips (aligned_index (2, 2, 0)), their lead
columns ((0, 0, 0), (3, 0, 0)), the register J-march (odd pitch) and the point-per-thread kernel (K-contiguous); (7, 9, 2) the
transposed skinny kernel; (125, 17, 2) / (249, 17, 2) a last strip of one column and a wave with one row; (513, 6, 2) the masked
16-byte lanes of lap5; K = 5, 57, 121, 161 the streaming tridiagonal kernel and its three on-chip stacks.

Wall time of this file on one MI355X: 8 s for its 56 tests (the slowest, the generated tridiagonal solve with its hiprtc build,
1.9 s; the cases of the hand-written kernels 0.01 - 0.3 s each).
"""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import edge_values as E  # noqa: E402
from oracle import ref_numpy as R  # noqa: E402  (oracle = checker only)

DTYPES = [np.float64, np.float32]
SENTINEL = -7.0
SCALAR = 0.375  # abs(ties) * 0.125
LAP_NAMES = ["notebook", "docs", "suite", "avg"]


def _name(dtype):
    return np.dtype(dtype).name


# ---- horizontal diffusion ---------------------------------------------------------------------------------------------------
def _hdiff_combos(dtype):
    """(limiter, coefficient kind, literal_float_precision, dtype of a scalar coefficient)"""
    combos = [(lim, kind, 64, np.float64) for lim in (True, False) for kind in ("field", "scalar")]
    if dtype == np.float32:
        combos += [(True, "field", 32, None), (True, "scalar", 32, np.float32), (True, "scalar", 32, np.float64)]
    return combos


def _hdiff_flags(limiter, kind, lit, sdt):
    from gt4py_amd import _lib

    return ((_lib.HDIFF_LIMITER if limiter else 0) | (_lib.HDIFF_INTERNAL_F32 if lit == 32 else 0)
            | (_lib.HDIFF_COEFF_F32 if kind == "scalar" and sdt == np.float32 else 0))


def _hdiff_want(u, c, domain, limiter, kind, lit, sdt, scalar=SCALAR):
    want = np.full(u.shape, SENTINEL, u.dtype)
    R.hdiff(u, want, c if kind == "field" else sdt(scalar), origin_in=(2, 2, 0), origin_out=(2, 2, 0), origin_coeff=(2, 2, 0),
            domain=domain, limiter=limiter, literal_float_precision=lit)
    return want


def _hdiff_run(G, u, c, domain, layout, align, limiter, kind, lit, sdt, scalar=SCALAR, ring=None):
    d_in, d_out = G.DevArray(u, layout, align_index=align), G.DevArray(np.full(u.shape, SENTINEL, u.dtype), layout, align_index=align)
    d_cf = G.DevArray(c, layout, align_index=align) if kind == "field" else float(sdt(scalar))
    args = (d_in, d_out, d_cf, (2, 2, 0), (2, 2, 0), (2, 2, 0) if kind == "field" else None, domain, _hdiff_flags(limiter, kind, lit, sdt))
    if ring is None:
        G.hdiff(*args)
    else:
        G.hdiff_ring(*args, ring)
    return d_out.get()


def _ring_mask(shape, origin, domain, outer, inner):
    m = np.zeros(shape[:2], dtype=bool)
    (oi, oj), (di, dj) = origin[:2], domain[:2]
    m[oi - outer[0]:oi + di + outer[1], oj - outer[2]:oj + dj + outer[3]] = True
    m[oi + inner[0]:oi + di - inner[1], oj + inner[2]:oj + dj - inner[3]] = False
    return m


def _hdiff_geometries(dtype):
    """(domain, [(layout, aligned_index)])"""
    main = [("ifirst", (2, 2, 0)), ("ifirst", (0, 0, 0)), ("ifirst", (3, 0, 0)), ("ifirst_unaligned", (0, 0, 0)), ("kfirst", (0, 0, 0))]
    return [((130, 20, 2), main), ((7, 9, 2), [("ifirst", (2, 2, 0))]),
            ((125, 17, 2) if dtype == np.float64 else (249, 17, 2), [("ifirst", (2, 2, 0))])]


@pytest.mark.parametrize("nonfinite", [0.0, 0.01])
@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_hdiff_every_path_bit_for_bit_at_edge_values(dtype, regime, nonfinite):
    """Whole-domain kernels (LDS-sharing strips, lead columns, register J-march, point per thread, transposed skinny, last strip
    of one column) and the boundary ring (J-march strips of 16 columns, transposed tiles of 2): limiter on / off, coefficient
    field / scalar, and for float32 fields the float32 internals with a field, a float32 scalar and a float64 scalar."""
    import gpu_util as G

    for domain, layouts in _hdiff_geometries(dtype):
        u, c = E.hdiff_fields(regime, dtype, domain, nonfinite)
        for combo in _hdiff_combos(dtype):
            want = _hdiff_want(u, c, domain, *combo)
            for layout, align in layouts:
                got = _hdiff_run(G, u, c, domain, layout, align, *combo)
                E.same_bits(got, want, f"hdiff {_name(dtype)} {regime} nonfinite {nonfinite} {domain} {layout} {align} {combo}")
            if domain == (130, 20, 2):
                for widths in ((16, 16, 2, 2), (2, 2, 2, 2)):
                    mask = _ring_mask(u.shape, (2, 2, 0), domain, (0, 0, 0, 0), widths)
                    got = _hdiff_run(G, u, c, domain, "ifirst", (2, 2, 0), *combo, ring=widths)
                    E.same_bits(got, np.where(mask[:, :, None], want, u.dtype.type(SENTINEL)),
                                f"hdiff ring {widths} {_name(dtype)} {regime} nonfinite {nonfinite} {combo}")


@pytest.mark.parametrize("regime", E.REGIMES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_hdiff_coefficient_of_negative_zero_subnormal_and_inf(dtype, regime):
    """coeff * (...) with a coefficient of -0.0 (the sign of a zero product), a subnormal (the product underflows) and inf
    (inf * 0 = NaN): as a field, and as a scalar of either precision."""
    import gpu_util as G

    domain = (130, 20, 2)
    u, _ = E.hdiff_fields(regime, dtype, domain)
    c = E.special_coeff(dtype, u.shape, np.random.default_rng(11))
    sub = float(np.finfo(dtype).smallest_subnormal)
    for lit in (64, 32) if dtype == np.float32 else (64,):
        for layout, align in (("ifirst", (2, 2, 0)), ("ifirst_unaligned", (0, 0, 0)), ("kfirst", (0, 0, 0))):
            combo = (True, "field", lit, None)
            E.same_bits(_hdiff_run(G, u, c, domain, layout, align, *combo), _hdiff_want(u, c, domain, *combo),
                        f"hdiff special coefficient field {_name(dtype)} {regime} {layout} literal {lit}")
        for sdt in (np.float64, np.float32):
            for scalar in (-0.0, sub, np.inf, 0.3):  # (0.3 is not a float32 value: the two scalar precisions differ)
                combo = (True, "scalar", lit, sdt)
                E.same_bits(_hdiff_run(G, u, c, domain, "ifirst", (2, 2, 0), *combo, scalar=scalar),
                            _hdiff_want(u, c, domain, *combo, scalar=scalar),
                            f"hdiff scalar coefficient {scalar!r} as {sdt.__name__} {_name(dtype)} {regime} literal {lit}")


# ---- 5-point Laplacians ----------------------------------------------------------------------------------------------------
def _lap_want(inp, variant, literal32, origin=(1, 1, 0), domain=None):
    want = np.full(inp.shape, SENTINEL, inp.dtype)
    if inp.dtype == np.float64 or literal32:  # the literal has the field's dtype: the oracle module's form
        return R.laplacian(inp, want, origin_inp=origin, origin_out=origin, domain=domain, variant=LAP_NAMES[variant])
    return E.lap5_expected(inp, want, variant, False, origin, domain)


@pytest.mark.parametrize("nonfinite", [0.0, 0.01])
@pytest.mark.parametrize("regime", E.LAP_REGIMES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_lap5_every_path_bit_for_bit_at_edge_values(dtype, regime, nonfinite):
    """Variants 0-3.  float64: (130, 20, 2) in four layouts, (513, 6, 2) with masked 16-byte lanes at two alignments.  float32:
    float64 and float32 literals, both domains, three alignments of the origin column."""
    import gpu_util as G
    from gt4py_amd import _lib

    if dtype == np.float64:
        cases = [((130, 20, 2), layout, (1, 1, 0), False) for layout in ("ifirst", "ifirst_unaligned", "kfirst", "jfirst")]
        cases += [((513, 6, 2), "ifirst", align, False) for align in ((0, 0, 0), (1, 1, 0))]
    else:
        cases = [(domain, "ifirst", align, lit32) for domain in ((130, 20, 2), (513, 6, 2)) for align in ((1, 1, 0), (0, 0, 0), (2, 0, 0))
                 for lit32 in (False, True)]
    for domain, layout, align, lit32 in cases:
        inp = E.lap_field(regime, dtype, (domain[0] + 2, domain[1] + 2, domain[2]), nonfinite)
        for variant in range(4):
            want = _lap_want(inp, variant, lit32)
            d_in = G.DevArray(inp, layout, align_index=align)
            d_out = G.DevArray(np.full(inp.shape, SENTINEL, dtype), layout, align_index=align)
            G.lap5(d_in, d_out, (1, 1, 0), (1, 1, 0), domain, variant, _lib.LAP_LITERAL_F32 if lit32 else 0)
            E.same_bits(d_out.get(), want, f"lap5 {_name(dtype)} {regime} nonfinite {nonfinite} {domain} {layout} {align} v{variant} literal32 {lit32}")


@pytest.mark.parametrize("regime", E.LAP_REGIMES)
def test_lap5_ring_bit_for_bit_at_edge_values(regime):
    """gt4mi_lap5_ring_f64: (domain grown by 1) minus (domain shrunk by 3) on (128, 40, 3), nothing else written."""
    import gpu_util as G

    H, domain, outer, inner = 4, (128, 40, 3), (1, 1, 1, 1), (3, 3, 3, 3)
    shape = (domain[0] + 2 * H, domain[1] + 2 * H, domain[2])
    mask = _ring_mask(shape, (H, H, 0), domain, outer, inner)
    for nonfinite in (0.0, 0.01):
        inp = E.lap_field(regime, np.float64, shape, nonfinite)
        for variant in range(4):
            full = _lap_want(inp, variant, False)  # on [1, -1) of the whole array
            d_in, d_out = G.DevArray(inp, "ifirst", (H, H, 0)), G.DevArray(np.full(shape, SENTINEL), "ifirst", (H, H, 0))
            G.lap5_ring(d_in, d_out, (H, H, 0), (H, H, 0), domain, outer, inner, variant=variant)
            E.same_bits(d_out.get(), np.where(mask[:, :, None], full, SENTINEL), f"lap5 ring {regime} nonfinite {nonfinite} v{variant}")


# ---- tridiagonal solve -----------------------------------------------------------------------------------------------------
TRIDIAG_SHAPES = [(17, 5, 5), (66, 3, 57), (66, 3, 121), (64, 3, 161)]


@functools.lru_cache(maxsize=None)
def _tridiag_case(dtype, shape):
    inf, diag, sup, rhs = E.tridiag_fields(dtype, shape)
    s, r, o = sup.copy(), rhs.copy(), np.full(shape, SENTINEL, dtype)
    R.tridiag(inf, diag, s, r, o)
    return (inf, diag, sup, rhs), (s, r, o)


@pytest.mark.parametrize("layout", ["ifirst", "kfirst"])
@pytest.mark.parametrize("dtype", DTYPES)
def test_tridiag_every_path_bit_for_bit_at_edge_values(dtype, layout):
    """`out` and the in-place `sup` and `rhs`: quotients that are subnormal, round at the subnormal boundary, overflow, x / 0,
    0 / 0 and inf / inf, in the streaming kernel (K = 5), the on-chip stacks (57, 121, 161 levels) and the any-stride kernel."""
    import gpu_util as G

    origins = {n: (0, 0, 0) for n in ("inf", "diag", "sup", "rhs", "out")}
    for shape in TRIDIAG_SHAPES:
        fields, (s_w, r_w, o_w) = _tridiag_case(dtype, shape)
        d = [G.DevArray(a, layout) for a in fields + (np.full(shape, SENTINEL, dtype),)]
        G.tridiag(*d, origins, shape)
        for name, got, want in (("out", d[4].get(), o_w), ("sup", d[2].get(), s_w), ("rhs", d[3].get(), r_w)):
            E.same_bits(got, want, f"tridiag {name} {_name(dtype)} {shape} {layout}")
        for n in (0, 1):
            E.same_bits(d[n].get(), fields[n], f"tridiag input {n} changed")


@pytest.mark.parametrize("dtype", DTYPES)
def test_tridiag_with_out_sharing_the_array_of_rhs_at_edge_values(dtype):
    import gpu_util as G

    shape = (66, 2, 100)
    inf, diag, sup, rhs = E.tridiag_fields(dtype, shape)
    s_w, r_w = sup.copy(), rhs.copy()
    R.tridiag(inf, diag, s_w, r_w, r_w)  # out IS rhs
    d = [G.DevArray(a, "ifirst") for a in (inf, diag, sup, rhs)]
    G.tridiag(*d, d[3], {n: (0, 0, 0) for n in ("inf", "diag", "sup", "rhs", "out")}, shape)
    E.same_bits(d[3].get(), r_w, f"tridiag out = rhs {_name(dtype)}")
    E.same_bits(d[2].get(), s_w, f"tridiag sup {_name(dtype)}")


# ---- the generated (hiprtc) kernels of the same definitions ----------------------------------------------------------------------
def _stencils(definition, dtype):
    from gt4py_amd.cartesian import gtscript

    return [gtscript.stencil(backend="hip:mi300", definition=definition, dtypes={"T": dtype}, use_kernel_library=lib) for lib in (False, True)]


def _storage(host, origin):
    import gt4py_amd.storage as gt_storage

    return gt_storage.from_array(host, host.dtype, backend="hip:mi300", aligned_index=origin)


@pytest.mark.parametrize("dtype", DTYPES)
def test_generated_hdiff_bit_for_bit_at_edge_values(dtype):
    """hip_templates.hdiff_limiter_field through the code generator and hiprtc (its own option list): against the oracle, and
    against the kernel library's output for the same fields."""
    from gt4py_amd.cartesian.backend import hip_templates

    domain, origin = (130, 20, 2), (2, 2, 0)
    stencils = _stencils(hip_templates.hdiff_limiter_field, dtype)
    for regime in E.REGIMES:
        for nonfinite in (0.0, 0.01):
            u, c = E.hdiff_fields(regime, dtype, domain, nonfinite)
            want = _hdiff_want(u, c, domain, True, "field", 64, None)
            outs = []
            for st in stencils:
                d_out = _storage(np.full(u.shape, SENTINEL, dtype), origin)
                st(_storage(u, origin), d_out, _storage(c, origin), origin=origin, domain=domain)
                outs.append(d_out.get())
            E.same_bits(outs[0], want, f"generated hdiff {_name(dtype)} {regime} nonfinite {nonfinite}")
            E.same_bits(outs[0], outs[1], f"generated hdiff against the kernel library {_name(dtype)} {regime} nonfinite {nonfinite}")


@pytest.mark.parametrize("variant", range(4))
@pytest.mark.parametrize("dtype", DTYPES)
def test_generated_lap5_bit_for_bit_at_edge_values(dtype, variant):
    from gt4py_amd.cartesian.backend import hip_templates

    domain, origin = (130, 20, 2), (1, 1, 0)
    stencils = _stencils(getattr(hip_templates, "lap_" + LAP_NAMES[variant]), dtype)
    for regime in E.LAP_REGIMES:
        for nonfinite in (0.0, 0.01):
            inp = E.lap_field(regime, dtype, (domain[0] + 2, domain[1] + 2, domain[2]), nonfinite)
            want = _lap_want(inp, variant, False)
            outs = []
            for st in stencils:
                d_out = _storage(np.full(inp.shape, SENTINEL, dtype), origin)
                st(_storage(inp, origin), d_out, origin=origin, domain=domain)
                outs.append(d_out.get())
            E.same_bits(outs[0], want, f"generated lap5 v{variant} {_name(dtype)} {regime} nonfinite {nonfinite}")
            E.same_bits(outs[0], outs[1], f"generated lap5 v{variant} against the kernel library {_name(dtype)} {regime} nonfinite {nonfinite}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_generated_tridiag_bit_for_bit_at_edge_values(dtype):
    from gt4py_amd.cartesian.backend import hip_templates

    shape = (66, 3, 57)
    fields, (s_w, r_w, o_w) = _tridiag_case(dtype, shape)
    outs = []
    for st in _stencils(hip_templates.tridiagonal_solver, dtype):
        dev = [_storage(a.copy(), (0, 0, 0)) for a in fields + (np.full(shape, SENTINEL, dtype),)]
        st(*dev)
        outs.append([dev[n].get() for n in (4, 2, 3)])
    for n, (name, want) in enumerate((("out", o_w), ("sup", s_w), ("rhs", r_w))):
        E.same_bits(outs[0][n], want, f"generated tridiag {name} {_name(dtype)}")
        E.same_bits(outs[0][n], outs[1][n], f"generated tridiag {name} against the kernel library {_name(dtype)}")
