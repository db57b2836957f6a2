"""``gt4py_amd.sampling`` on the GPU: bit for bit against the contract's restatement (tests/point_sample_ref.py), NaN compared as
NaN, over EVERY byte of the result's buffer -- padding and the allocation's slack keep a NaN-payload sentinel, compared as integers
--, with the fields and the result in the four layouts of tests/device_layouts.py, for float32 / float64 fields against float32 /
float64 positions, the four methods, column and point mode, no reach and an asymmetric one, 1 to 9 fields per call, point and level
counts on both sides of a wave, positions on nodes, halves, the ends of the readable box, beyond them, +-inf and NaN, clamped or
filled; byte for byte against ``HorizontalInterp`` and ``DepartureInterp`` on the device; with positions rewritten between two calls
of one object, and handed over from and to a stencil in stream order."""

import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import device_layouts as L  # noqa: E402  (the layouts; test infrastructure)
import point_sample_ref as S  # noqa: E402
from oracle import ref_numpy as ORACLE  # noqa: E402  (oracle = checker only)

DOMAINS = [(1, 1, 1), (3, 5, 2), (17, 33, 5), (65, 63, 7)]
NPOINTS = [1, 63, 64, 65, 130]  # around one wave and two
LEVELS = [1, 5, 65]  # in column mode the level is the fastest lane index: 65 levels cross a wave
REACHES = [0, ((3, 1), (0, 2))]
DTYPES = [(np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32), (np.float64, np.float64)]  # (fields, positions)
COUNTS = [1, 3, 8, 9]
OUTSIDE = [("clamp", 0.0), ("fill", -999.25), ("fill", float("nan"))]
SPECIAL = 12  # items _point_list plants per axis


@pytest.fixture(scope="module", autouse=True)
def _leave_no_cached_device_memory():
    """The small buffers of this file go back to the driver when it is done (tests/test_placement.py, which may run behind it in
    the same process, searches the FREE device memory)."""
    yield
    import torch

    torch.cuda.empty_cache()


def _reach4(reach):
    return (reach,) * 4 if isinstance(reach, int) else (reach[0][0], reach[0][1], reach[1][0], reach[1][1])


# ---- inputs: arrays of the dtype the device gets, so that the restatement sees what the device sees -----------------------------
def _point_list(rng, domain, reach4, npoints, point_mode, pdtype, special=True):
    """The position arrays of ``npoints`` points: random around the readable box (up to 3 cells beyond it), exact nodes, exact
    halves and -- ``special``, as many as fit -- xmin and xmax themselves, the next representable positions beyond them, a point 3
    cells beyond each, -0.0, +-inf, NaN and +-1e300 at random points.  Returns (the arrays, the points that hold a planted item)."""
    out, planted = [], set()
    axes = list(zip(domain, (reach4[0], reach4[2], 0), (reach4[1], reach4[3], 0)))
    for n, lo, hi in axes[: 3 if point_mode else 2]:
        p = rng.uniform(-lo - 3.0, n - 1 + hi + 3.0, npoints)
        kind = rng.integers(0, 4, npoints)
        p = np.where(kind == 0, np.clip(np.round(p), -lo, n - 1 + hi), np.where(kind == 1, np.floor(p) + 0.5, p))
        with np.errstate(over="ignore"):
            p = p.astype(pdtype)
        if special:
            xmin, xmax = pdtype(-lo), pdtype(n - 1 + hi)
            with np.errstate(over="ignore"):
                items = np.array([xmin, xmax, np.nextafter(xmin, pdtype(-np.inf)), np.nextafter(xmax, pdtype(np.inf)), np.inf, -np.inf, np.nan,
                                  xmin - pdtype(3), xmax + pdtype(3), -0.0, 1e300, -1e300][:SPECIAL]).astype(pdtype)
            where = rng.permutation(npoints)[: items.size]
            p[where] = items[: where.size]
            planted |= set(where.tolist())
        out.append(p)
    return out, sorted(planted)


def _field_values(rng, shape, nfields, fdtype):
    out = []
    for n in range(nfields):
        if n % 3 == 0:
            q = rng.uniform(-1, 1, shape)
        elif n % 3 == 1:  # smooth and large: the cubic's overshoots are limited
            q = np.cumsum(np.cumsum(rng.uniform(0.1, 1, shape), axis=0), axis=1) * 10.0 ** rng.integers(-3, 4)
        else:
            q = 280.0 + rng.uniform(-1, 1, shape)
        out.append(q.astype(fdtype))
    return out


class _Case:
    """The device arrays of one call and what the restatement says about them."""


def _setup(domain, npoints, *, point_mode=False, fdtype=np.float64, pdtype=np.float64, layout="ifirst", result_layout=None, reach=0,
           nfields=1, order=None, seed=0, positions=None, special=True, own_result=False):
    ni, nj, nk = domain
    c = _Case()
    c.reach4 = lo_i, hi_i, lo_j, hi_j = _reach4(reach)
    # (positions and fields from generators of their own: the same seed gives the same of each whatever else differs)
    rng_p, rng_q = (np.random.default_rng([seed, ni, nj, nk, lo_i, hi_i, lo_j, hi_j, what]) for what in (0, 1))
    # one ghost cell in front of the readable box on the low sides, one ghost row / column behind the array the product sees
    readable = (lo_i + ni + hi_i, lo_j + nj + hi_j)
    shape = (readable[0] + 2, readable[1] + 2, nk)
    c.origin = (1 + lo_i, 1 + lo_j, 0)
    c.rbox = (slice(1, 1 + readable[0]), slice(1, 1 + readable[1]))
    c.planted = []
    if positions is None:
        positions, c.planted = _point_list(rng_p, domain, c.reach4, npoints, point_mode, pdtype, special)
    c.positions = [np.ascontiguousarray(p, dtype=pdtype) for p in positions]
    c.order = list(range(nfields)) if order is None else list(order)
    c.qs = _field_values(rng_q, shape, max(c.order) + 1, fdtype)
    c.srcs = [L.Dev(shape, fdtype, layout, c.qs[n], c.origin[0]) for n in c.order]
    c.pos = [L.Line(p) for p in c.positions]
    nf = len(c.order)
    c.result = None
    if not own_result:
        # The caller's result in one of the four layouts, with a sentinel in the row and the column that L.Dev hides, in the padding
        # and (point mode, "kfirst") in a second level.  The blocks of two fields must not interleave in memory (the library's rule
        # for any two dst), so the field is the slowest axis: axis 0 of C order ("kfirst"), axis 2 of the three other layouts.
        nkk = 1 if point_mode else nk
        c.field_last = (result_layout or layout) != "kfirst"
        if c.field_last:
            c.result = L.Dev((npoints + 1, nkk + 1, nf), fdtype, result_layout or layout, None, 0)
            out3 = c.result.given.permute(2, 0, 1)
            c.box = (slice(0, npoints), slice(0, nkk), slice(0, nf))
        else:
            c.result = L.Dev((nf + 1, npoints + 1, 2 if point_mode else nk), fdtype, "kfirst", None, 0)
            out3 = c.result.given[:, :, :nkk]
            c.box = (slice(0, nf), slice(0, npoints), slice(0, nkk))
        c.out = out3[:, :, 0] if point_mode else out3
    c.point_mode, c.nk, c.npoints, c.fdtype = point_mode, nk, npoints, fdtype
    return c


def _want(c, method, outside="clamp", fill_value=0.0):
    args = c.positions + ([] if c.point_mode else [None])
    return {n: S.sample(c.qs[n][c.rbox], *args, method, c.reach4, outside, fill_value) for n in c.order}


def _run(domain, npoints, method, *, outside="clamp", fill_value=0.0, **kwargs):
    """One call through ``sampling.Sample``; the result's buffer is compared whole against the restatement, every input must come
    back unchanged.  Returns (the samples as the device left them, by field number; the case)."""
    from gt4py_amd import sampling

    c = _setup(domain, npoints, **kwargs)
    halo = ((c.reach4[0], c.reach4[1]), (c.reach4[2], c.reach4[3]))
    s = sampling.Sample([d.given for d in c.srcs], pos_i=c.pos[0].given, pos_j=c.pos[1].given, pos_k=c.pos[2].given if c.point_mode else None,
                        method=method, outside=outside, fill_value=fill_value, halo=halo, origin=c.origin, out=None if c.result is None else c.out)
    nf = len(c.order)
    assert (s.domain, s.npoints, s.launches, s.method, s.outside, s.origin) == (domain, npoints, -(-nf // 8), method, outside, c.origin)
    assert s.result.shape == ((nf, npoints) if c.point_mode else (nf, npoints, c.nk)) and s.result.dtype == np.dtype(c.fdtype)
    s()
    what = (f"{method} {'point' if c.point_mode else 'column'} mode, domain {domain}, {npoints} points, {np.dtype(c.fdtype)} fields "
            f"{c.positions[0].dtype} positions, reach {c.reach4}, outside={outside} ({fill_value}), {nf} fields")
    want = _want(c, method, outside, fill_value)
    stacked = np.stack([want[n] for n in c.order])
    if c.result is None:
        got = s.get()
        assert s.result.tensor.is_contiguous() and got.dtype == stacked.dtype and S.same_bits(got, stacked).all(), what
    else:
        stacked3 = stacked[:, :, None] if c.point_mode else stacked
        got = c.result.assert_box(c.box, stacked3.transpose(1, 2, 0) if c.field_last else stacked3, what)
        got = got.transpose(2, 0, 1) if c.field_last else got
        got = got[:, :, 0] if c.point_mode else got
        assert S.same_bits(got, s.get()).all()
    for slot, d in enumerate(c.srcs):
        d.assert_unchanged(f"{what}: field {slot}")
    for name, p in zip(("pos_i", "pos_j", "pos_k"), c.pos):
        p.assert_unchanged(f"{what}: {name}")
    return {n: got[slot] for slot, n in enumerate(c.order)}, c


# ---- the grid: a seeded selection of the product that keeps every value of every factor ----------------------------------------------
FACTORS = (DOMAINS, NPOINTS, L.LAYOUTS, DTYPES, list(S.METHODS), [False, True], REACHES, COUNTS, OUTSIDE)


def _cases(count=48, seed=2031):
    rng = np.random.default_rng(seed)

    def column(values):
        reps = [values[n % len(values)] for n in range(count)]
        return [reps[n] for n in rng.permutation(count)]

    columns = [column(v) for v in FACTORS]
    for values, col in zip(FACTORS, columns):
        assert all(v in col for v in values)
    return list(zip(*columns))


def _case_id(case):
    domain, npoints, layout, (fd, pd), method, point_mode, reach, count, (outside, fill_value) = case
    return (f"{'x'.join(map(str, domain))}-{npoints}p-{layout}-{np.dtype(fd).name}-{np.dtype(pd).name}-{method}-{'point' if point_mode else 'column'}-"
            f"r{''.join(map(str, _reach4(reach)))}-{count}-{outside}{'' if outside == 'clamp' else fill_value}")


@pytest.mark.parametrize("case", _cases(), ids=_case_id)
def test_every_byte_against_the_restatement(case):
    domain, npoints, layout, (fdtype, pdtype), method, point_mode, reach, count, (outside, fill_value) = case
    _run(domain, npoints, method, outside=outside, fill_value=fill_value, point_mode=point_mode, fdtype=fdtype, pdtype=pdtype, layout=layout,
         reach=reach, nfields=count, seed=1)


@pytest.mark.parametrize("point_mode", [False, True], ids=["column", "point"])
@pytest.mark.parametrize("nk", LEVELS)
@pytest.mark.parametrize("npoints", NPOINTS)
def test_point_and_level_counts_on_both_sides_of_a_wave(npoints, nk, point_mode):
    """Every pair of the two counts, in both modes; the method, the dtypes, the layouts and the fill rule take turns."""
    turn = NPOINTS.index(npoints) * len(LEVELS) + LEVELS.index(nk)
    method = S.METHODS[turn % 4]
    fdtype, pdtype = DTYPES[(turn // 4 + turn) % 4]
    outside, fill_value = OUTSIDE[turn % 3]
    _run((6, 5, nk), npoints, method, outside=outside, fill_value=fill_value, point_mode=point_mode, fdtype=fdtype, pdtype=pdtype,
         layout=L.LAYOUTS[turn % 4], result_layout=L.LAYOUTS[(turn + 1) % 4], reach=REACHES[turn % 2], nfields=2, seed=2)


@pytest.mark.parametrize("method", S.METHODS)
def test_the_object_owns_a_c_ordered_result_when_none_is_given(method):
    for point_mode in (False, True):
        _run((17, 33, 5), 130, method, point_mode=point_mode, fdtype=np.float32, reach=((3, 1), (0, 2)), nfields=9, seed=3, own_result=True)


@pytest.mark.parametrize("point_mode", [False, True], ids=["column", "point"])
@pytest.mark.parametrize("method", S.METHODS)
def test_every_special_position_is_among_the_inputs_and_fill_marks_exactly_the_points_outside(method, point_mode):
    domain, reach, npoints = (17, 33, 5), ((3, 1), (0, 2)), 130
    for pdtype in (np.float32, np.float64):
        kwargs = dict(point_mode=point_mode, fdtype=np.float32, pdtype=pdtype, reach=reach, nfields=2, seed=4)
        clamp, c = _run(domain, npoints, method, **kwargs)
        outside = np.zeros(npoints, dtype=bool)
        for p, n, lo, hi in zip(c.positions, domain, (3, 0, 0), (1, 2, 0)):
            x = p.astype(np.float64)
            assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any() and (np.signbit(x) & (x == 0)).any()
            assert (x == -lo).any() and (x == n - 1 + hi).any() and (x == np.nextafter(pdtype(-lo), pdtype(-np.inf))).any()
            assert (x == np.nextafter(pdtype(n - 1 + hi), pdtype(np.inf))).any() and (x == -lo - 3).any() and (x == n - 1 + hi + 3).any()
            finite = x[np.isfinite(x)]
            assert (finite == np.floor(finite)).any() and (finite - np.floor(finite) == 0.5).any()
            outside |= (x < -lo) | (x > n - 1 + hi) | np.isnan(x)
        assert outside.any() and not outside.all()
        for fill_value in (-999.25, float("nan")):
            fill, _ = _run(domain, npoints, method, outside="fill", fill_value=fill_value, **kwargs)
            item = S.fill_item(fill_value, np.float32)
            for n in clamp:
                assert S.same_bits(fill[n][outside], np.full(fill[n][outside].shape, item)).all()  # in every field and every level
                assert S.same_bits(fill[n][~outside], clamp[n][~outside]).all()  # every other point: the bits of the clamp mode
                assert not (fill[n][~outside] == np.float32(-999.25)).any()


@pytest.mark.parametrize("point_mode", [False, True], ids=["column", "point"])
@pytest.mark.parametrize("method", S.METHODS)
def test_planted_infinite_and_nan_positions_change_no_other_point(method, point_mode):
    domain, reach, npoints = (17, 33, 5), ((3, 1), (0, 2)), 130
    kwargs = dict(point_mode=point_mode, fdtype=np.float64, pdtype=np.float64, reach=reach, nfields=3, seed=5)
    clean, c = _run(domain, npoints, method, special=False, **kwargs)
    assert all(np.isfinite(p).all() for p in c.positions) and all(np.isfinite(v).all() for v in clean.values())
    dirty_positions = [p.copy() for p in c.positions]
    at = {0: [3, 64], 1: [63, 129], 2: [65, 100]}
    for axis, p in enumerate(dirty_positions):
        p[at[axis][0]], p[at[axis][1]] = np.nan, (np.inf if axis % 2 == 0 else -np.inf)
    touched = np.zeros(npoints, dtype=bool)
    touched[[q for axis in range(len(dirty_positions)) for q in at[axis]]] = True
    nan_at = [at[axis][0] for axis in range(len(dirty_positions))]
    for outside, fill_value in (("clamp", 0.0), ("fill", 1.0e30)):
        if outside == "fill":  # (the random positions reach beyond the readable box: the clean run fills those as well)
            clean, _ = _run(domain, npoints, method, special=False, outside=outside, fill_value=fill_value, **kwargs)
        dirty, _ = _run(domain, npoints, method, positions=dirty_positions, outside=outside, fill_value=fill_value, **kwargs)
        for n in clean:
            assert S.same_bits(dirty[n][~touched], clean[n][~touched]).all(), (n, outside)  # no other point
            if outside == "clamp":
                assert np.isnan(dirty[n][nan_at]).all() and np.isfinite(dirty[n][touched]).sum() == np.isfinite(dirty[n][touched]).size // 2
            else:
                assert (dirty[n][touched] == 1.0e30).all()


# ---- against the two interpolators, on the device ----------------------------------------------------------------------------------
def _grid_positions(rng, shape, domain, reach):
    """Absolute position fields over ``shape`` = the domain (or its first two axes): around the readable box, beyond it, +-inf; no NaN
    (which NaN an operation on a NaN yields is not part of the contract, and the tests below compare BYTES)."""
    out = []
    for n in domain[: len(shape)] if len(shape) == 3 else domain[:2]:
        p = rng.uniform(-reach - 3.0, n - 1 + reach + 3.0, shape)
        kind = rng.integers(0, 4, shape)
        p = np.where(kind == 0, np.round(p), np.where(kind == 1, np.floor(p) + 0.5, p))
        where = rng.permutation(p.size)[:4]
        p.reshape(-1)[where] = [np.inf, -np.inf, -float(reach), n - 1.0 + reach][: where.size]
        out.append(p)
    return out


@pytest.mark.parametrize("method", S.METHODS)
def test_column_mode_returns_the_bytes_horizontal_interp_writes(method):
    import torch

    from gt4py_amd import horizontal, sampling

    rng = np.random.default_rng(6)
    reach = 2
    for (ni, nj, nk), fdtype, pdtype in (((9, 6, 5), np.float32, np.float64), ((5, 4, 66), np.float64, np.float32), ((1, 1, 1), np.float64, np.float64)):
        shape = (ni + 2 * reach + 1, nj + 2 * reach + 1, nk)
        box = (slice(reach, reach + ni), slice(reach, reach + nj))
        q = (280.0 + rng.uniform(-1, 1, shape)).astype(fdtype)
        pi, pj = (p.astype(pdtype) for p in _grid_positions(rng, (ni, nj), (ni, nj, nk), reach))
        src = L.Dev(shape, fdtype, "ifirst", q, reach)
        theirs = L.Dev(shape, fdtype, "ifirst", None, reach)
        d_pi, d_pj = (torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in (pi, pj))  # Field[IJ], C order: point p = i * nj + j
        full_i, full_j = (torch.zeros(shape[:2], dtype=d.dtype, device="cuda") for d in (d_pi, d_pj))
        full_i[box], full_j[box] = d_pi, d_pj
        horizontal.interpolate(theirs.given, src.given, pos_i=full_i[:-1, :-1], pos_j=full_j[:-1, :-1], method=method, halo=reach)
        ours = sampling.sample(src.given, pos_i=d_pi.reshape(-1), pos_j=d_pj.reshape(-1), method=method, halo=reach)
        want = S.sample(q[:-1, :-1], pi.reshape(-1), pj.reshape(-1), None, method, (reach,) * 4)
        field = theirs.assert_box(box, want.reshape(ni, nj, nk), f"{method} {(ni, nj, nk)}: HorizontalInterp")
        ut = L.NP_UINT[field.itemsize]
        assert ours.shape == (1, ni * nj, nk) and np.array_equal(ours[0].view(ut), field.reshape(ni * nj, nk).view(ut)), (method, ni, nj, nk)


@pytest.mark.parametrize("method", S.METHODS)
def test_point_mode_returns_the_bytes_departure_interp_writes(method):
    import torch

    from gt4py_amd import departure, sampling

    rng = np.random.default_rng(7)
    reach = 2
    for (ni, nj, nk), fdtype, pdtype in (((9, 6, 5), np.float32, np.float64), ((5, 4, 9), np.float64, np.float32), ((3, 2, 1), np.float64, np.float64),
                                         ((4, 3, 3), np.float32, np.float32)):
        shape = (ni + 2 * reach + 1, nj + 2 * reach + 1, nk)
        box = (slice(reach, reach + ni), slice(reach, reach + nj))
        q = (280.0 + rng.uniform(-1, 1, shape)).astype(fdtype)
        pi, pj = (p.astype(pdtype) for p in _grid_positions(rng, (ni, nj, nk), (ni, nj, nk), reach)[:2])
        pk = rng.uniform(-1.5, nk + 0.5, (ni, nj, nk))
        pk.reshape(-1)[rng.permutation(pk.size)[:6]] = [0.0, nk - 1.0, np.inf, -np.inf, 0.5, nk - 1.5]
        pk = pk.astype(pdtype)
        src = L.Dev(shape, fdtype, "ifirst", q, reach)
        theirs = L.Dev(shape, fdtype, "ifirst", None, reach)
        lists = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in (pi, pj, pk)]  # C order: point p = (i * nj + j) * nk + k
        full = [torch.zeros(shape, dtype=d.dtype, device="cuda") for d in lists]
        for f, d in zip(full, lists):
            f[box] = d
        departure.interpolate_3d(theirs.given, src.given, pos_i=full[0][:-1, :-1], pos_j=full[1][:-1, :-1], pos_k=full[2][:-1, :-1], method=method,
                                 halo=reach)
        ours = sampling.sample(src.given, pos_i=lists[0].reshape(-1), pos_j=lists[1].reshape(-1), pos_k=lists[2].reshape(-1), method=method,
                               halo=reach)
        want = S.sample(q[:-1, :-1], pi.reshape(-1), pj.reshape(-1), pk.reshape(-1), method, (reach,) * 4)
        field = theirs.assert_box(box, want.reshape(ni, nj, nk), f"{method} {(ni, nj, nk)}: DepartureInterp")
        ut = L.NP_UINT[field.itemsize]
        assert ours.shape == (1, ni * nj * nk) and np.array_equal(ours[0].view(ut), field.reshape(-1).view(ut)), (method, ni, nj, nk)


# ---- what the bits do not depend on -------------------------------------------------------------------------------------------------
def test_the_bits_of_a_sample_do_not_depend_on_layout_position_in_the_call_call_size_or_the_other_points():
    domain, reach, npoints = (17, 33, 5), ((3, 1), (0, 2)), 130
    for point_mode in (False, True):
        for method in S.METHODS:
            kwargs = dict(point_mode=point_mode, fdtype=np.float32, pdtype=np.float64, reach=reach, seed=8)
            nine, c = _run(domain, npoints, method, nfields=9, **kwargs)  # two launches
            for layout in L.LAYOUTS[1:]:
                other, _ = _run(domain, npoints, method, nfields=3, layout=layout, result_layout="kfirst", **kwargs)
                for n in other:
                    assert S.same_bits(other[n], nine[n]).all(), (method, layout, n)
            # field 8 -- the second launch's first entry above -- alone, as entry 2 of 3, as the last of 8, and field 0 behind it
            for order in ([8], [3, 5, 8], [7, 6, 5, 4, 3, 2, 1, 8], [8, 0]):
                other, _ = _run(domain, npoints, method, order=order, **kwargs)
                for n in order:
                    assert S.same_bits(other[n], nine[n]).all(), (method, order, n)
            # the points in reverse order, and the first 65 of them alone
            back, _ = _run(domain, npoints, method, nfields=1, positions=[p[::-1] for p in c.positions], **kwargs)
            assert S.same_bits(back[0][::-1], nine[0]).all(), method
            some, _ = _run(domain, 65, method, nfields=1, positions=[p[:65] for p in c.positions], **kwargs)
            assert S.same_bits(some[0], nine[0][:65]).all(), method


# ---- the frozen object ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("point_mode", [False, True], ids=["column", "point"])
def test_rewriting_the_position_arrays_between_two_calls_moves_the_samples(point_mode):
    import torch

    from gt4py_amd import sampling

    c = _setup((17, 33, 5), 65, point_mode=point_mode, fdtype=np.float32, pdtype=np.float32, reach=1, nfields=2, seed=9, own_result=True)
    s = sampling.Sample([d.given for d in c.srcs], pos_i=c.pos[0].given, pos_j=c.pos[1].given, pos_k=c.pos[2].given if point_mode else None,
                        method="cubic_monotone", outside="fill", fill_value=-1.0, halo=1, origin=c.origin)
    result_ptr = s.result.ptr
    s()
    first = s.get()
    assert S.same_bits(first, np.stack(list(_want(c, "cubic_monotone", "fill", -1.0).values()))).all()
    moved, _ = _point_list(np.random.default_rng(10), (17, 33, 5), c.reach4, 65, point_mode, np.float32)
    for line, p in zip(c.pos, moved):
        line.given.copy_(torch.from_numpy(p))  # (in stream order, behind the first call)
    c.positions = moved
    s()
    second = s.get()
    assert s.result.ptr == result_ptr  # nothing was allocated
    assert S.same_bits(second, np.stack(list(_want(c, "cubic_monotone", "fill", -1.0).values()))).all()
    assert not S.same_bits(first, second).all()
    assert S.same_bits(s.column(1).get(), second[1]).all()


def test_hand_over_from_a_stencil_and_to_a_stencil_in_stream_order():
    """A device_sync=False stencil writes a field, Sample reads it, a device_sync=False stencil reads the result -- a storage whose
    axes I, J and K are the point, the level and the field (the slowest axis of the storage layout: the blocks of two fields do not
    interleave), handed to Sample as its (field, point, level) view --, nothing in between: the stencils applied to the restatement."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import sampling
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates

    backend, (ni, nj, nk), h, npoints, nf = "hip:mi300", (48, 40, 9), 2, 70, 5
    rng = np.random.default_rng(11)
    shape = (ni + 2 * h, nj + 2 * h, nk)
    raw = rng.uniform(-1, 1, shape)
    others = [rng.uniform(-1, 1, shape) for _ in range(nf - 1)]
    (pi, pj), _ = _point_list(rng, (ni, nj, nk), (h,) * 4, npoints, False, np.float64)
    lap = gtscript.stencil(backend=backend, definition=hip_templates.lap_notebook, dtypes={"T": np.float64}, device_sync=False)
    d_raw, *d_others = (gt_storage.from_array(a, backend=backend, aligned_index=(h, h, 0)) for a in [raw] + others)
    d_first = gt_storage.zeros(shape, backend=backend, aligned_index=(h, h, 0))
    d_samples, d_out = (gt_storage.zeros((npoints, nk, nf), backend=backend) for _ in range(2))
    d_pi, d_pj = torch.from_numpy(pi).cuda(), torch.from_numpy(pj).cuda()
    stations = sampling.Sample([d_first] + d_others, pos_i=d_pi, pos_j=d_pj, method="cubic", halo=h, out=d_samples.tensor.permute(2, 0, 1))
    assert stations.domain == (ni, nj, nk) and stations.origin == (h, h, 0) and stations.result.ptr == d_samples.ptr
    for _ in range(2):  # (the second round finds everything already written: the same result)
        lap(d_raw, d_first, origin=(1, 1, 0), domain=(shape[0] - 2, shape[1] - 2, nk))
        stations()
        lap(d_samples, d_out, origin=(1, 1, 0), domain=(npoints - 2, nk - 2, nf))
    torch.cuda.synchronize()
    first = np.zeros(shape)
    ORACLE.laplacian(raw, first, origin_inp=(1, 1, 0), origin_out=(1, 1, 0), domain=(shape[0] - 2, shape[1] - 2, nk))
    samples = np.ascontiguousarray(np.stack([S.sample(q, pi, pj, None, "cubic", (h,) * 4) for q in [first] + others]).transpose(1, 2, 0))
    want = np.zeros_like(samples)
    ORACLE.laplacian(samples, want, origin_inp=(1, 1, 0), origin_out=(1, 1, 0), domain=(npoints - 2, nk - 2, nf))
    assert np.array_equal(d_first.get().view(np.uint64), first.view(np.uint64))
    assert S.same_bits(d_samples.get(), samples).all()
    assert S.same_bits(d_out.get(), want).all()


def test_an_object_refuses_to_run_after_an_array_has_died():
    import torch

    from gt4py_amd import sampling

    c = _setup((3, 5, 2), 7, nfields=1, seed=12, own_result=True)
    pos_i, pos_j = (torch.from_numpy(p).cuda() for p in c.positions)
    s = sampling.Sample(c.srcs[0].given, pos_i=pos_i, pos_j=pos_j)
    s()
    assert s.get().shape == (1, 7, 2)
    del pos_j
    gc.collect()
    with pytest.raises(RuntimeError, match="no longer exists"):
        s()
