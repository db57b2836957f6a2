"""``gt4py_amd.sampling`` without a GPU: the two forms of the contract's restatement (tests/point_sample_ref.py) held against each
other bit for bit, the properties the contract states (items moved by ``nearest``, the fill rule at and next to the ends of the
readable box, NaN and infinite positions, the one rounding of the fill value), every refusal of the C entry through the dry run
(made-up addresses that are never dereferenced), the declaration, the kernels' resources and the Python interface's argument
checks."""

import math

import numpy as np
import pytest

import entry_checks as E
import point_sample_ref as S
from entry_checks import INV, OOB, UNS, as_arg, int64s
from gt4py_amd import _lib, sampling

HOST = (10, 9, 5)  # the shape of a host field where a test states none
REACHES = [(0, 0, 0, 0), (1, 1, 1, 1), (3, 1, 0, 2)]


def _readable(rng, ni, nj, nk, reach, dtype=np.float64):
    return rng.uniform(-2, 2, (ni + reach[0] + reach[1], nj + reach[2] + reach[3], nk)).astype(dtype)


def _positions(rng, n, lo, hi, count, dtype):
    """``count`` positions along an axis of ``n`` points and a reach of lo / hi: random, integers, halves and every special item."""
    p = rng.uniform(-lo - 3.0, n + hi + 2.0, count)
    kind = rng.integers(0, 4, count)
    p = np.where(kind == 0, np.round(p), np.where(kind == 1, np.floor(p) + 0.5, p))
    special = [-float(lo), float(n - 1 + hi), np.nextafter(-float(lo), -np.inf), np.nextafter(float(n - 1 + hi), np.inf), -0.0, np.inf, -np.inf,
               np.nan, 1e300, -1e300, 0.0, n - 1.0]
    where = rng.permutation(count)[: len(special)]
    p[where] = special[: where.size]
    with np.errstate(over="ignore"):
        return p.astype(dtype)


# ---- the two forms of the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("point_mode", [False, True], ids=["column", "point"])
@pytest.mark.parametrize("method", S.METHODS)
def test_the_plain_python_and_the_numpy_restatement_agree_bit_for_bit(method, point_mode):
    rng = np.random.default_rng([31, point_mode])
    combos = [((0, 0, 0, 0), np.float64, np.float64), ((1, 1, 1, 1), np.float32, np.float32), ((3, 1, 0, 2), np.float32, np.float64),
              ((2, 2, 2, 2), np.float64, np.float32)]
    for (ni, nj, nk), count in (((1, 1, 1), 5), ((4, 3, 2), 40), ((6, 5, 5), 70)):
        for reach, fdtype, pdtype in combos:
            src = _readable(rng, ni, nj, nk, reach, fdtype)
            src.flat[0] = -0.0
            if src.size > 8:
                src[1, 1, 0], src[2, 0, nk - 1] = np.inf, np.nan
            pi = _positions(rng, ni, reach[0], reach[1], count, pdtype)
            pj = _positions(rng, nj, reach[2], reach[3], count, pdtype)
            pk = _positions(rng, nk, 0, 0, count, pdtype) if point_mode else None
            for outside, fill_value in (("clamp", 0.0), ("fill", -999.25), ("fill", math.nan)):
                a = S.sample(src, pi, pj, pk, method, reach, outside, fill_value)
                b = S.sample_plain(src, pi, pj, pk, method, reach, outside, fill_value)
                assert a.shape == b.shape == ((count,) if point_mode else (count, nk)) and a.dtype == b.dtype == src.dtype
                assert S.same_bits(a, b).all(), (method, point_mode, (ni, nj, nk), reach, fdtype, pdtype, outside)


# ---- the contract's properties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nearest_at_integer_positions_returns_the_source_items_bit_for_bit(dtype):
    rng = np.random.default_rng(32)
    reach, (ni, nj, nk) = (2, 1, 0, 3), (5, 4, 3)
    ut = S.UINT[np.dtype(dtype).itemsize]
    src = rng.integers(0, np.iinfo(ut).max, (ni + 3, nj + 3, nk), dtype=ut, endpoint=True).view(dtype)  # any bit pattern: NaN payloads too
    ii, jj, kk = (a.reshape(-1) for a in np.meshgrid(np.arange(-2, ni + 1), np.arange(0, nj + 3), np.arange(nk), indexing="ij"))
    pi, pj, pk = ii.astype(np.float64), jj.astype(np.float32).astype(np.float64), kk.astype(np.float64)
    for outside in ("clamp", "fill"):  # (in range: nothing is filled)
        column = S.sample(src, pi, pj, None, "nearest", reach, outside, 5.0)
        assert np.array_equal(column.view(ut), src.view(ut)[ii + 2, jj, :])
        point = S.sample(src, pi, pj, pk, "nearest", reach, outside, 5.0)
        assert np.array_equal(point.view(ut), src.view(ut)[ii + 2, jj, kk])
        assert np.array_equal(S.sample_plain(src, pi[:40], pj[:40], pk[:40], "nearest", reach, outside, 5.0).view(ut), point.view(ut)[:40])


@pytest.mark.parametrize("pdtype", [np.float32, np.float64])
@pytest.mark.parametrize("method", S.METHODS)
def test_fill_spares_the_ends_of_the_readable_box_and_takes_the_next_position_beyond(method, pdtype):
    rng = np.random.default_rng(33)
    reach, (ni, nj, nk) = (3, 1, 0, 2), (6, 5, 4)
    src = _readable(rng, ni, nj, nk, reach, np.float32)
    ends = [(-3.0, float(ni)), (0.0, float(nj + 1)), (0.0, float(nk - 1))]
    inside = np.array([1.25, 2.5, 1.5], dtype=pdtype)
    for axis, (xmin, xmax) in enumerate(ends):
        for end, beyond in ((xmin, np.nextafter(pdtype(xmin), pdtype(-np.inf))), (xmax, np.nextafter(pdtype(xmax), pdtype(np.inf)))):
            assert pdtype(end) == end and beyond != end and abs(float(beyond) - end) <= (1e-6 if pdtype is np.float32 else 1e-15) * max(1.0, abs(end)) + 2e-45
            for point_mode in (False, True):
                if axis == 2 and not point_mode:
                    continue
                pos = np.repeat(inside[:, None], 2, axis=1)
                pos[axis] = [end, beyond]
                pi, pj, pk = pos[0], pos[1], (pos[2] if point_mode else None)
                clamp = S.sample(src, pi, pj, pk, method, reach, "clamp")
                fill = S.sample(src, pi, pj, pk, method, reach, "fill", -7.5)
                assert S.same_bits(fill[0], clamp[0]).all() and not (fill[0] == -7.5).any(), (axis, end)  # exactly at the end: NOT filled
                assert (fill[1] == np.float32(-7.5)).all(), (axis, beyond)  # the next representable position beyond: filled
                assert S.same_bits(clamp[1], clamp[0]).all()  # (clamped, it is the end itself)


@pytest.mark.parametrize("point_mode", [False, True], ids=["column", "point"])
@pytest.mark.parametrize("method", S.METHODS)
def test_nan_and_infinite_positions(method, point_mode):
    rng = np.random.default_rng(34)
    reach, (ni, nj, nk) = (1, 2, 2, 0), (5, 4, 4)
    for fdtype in (np.float32, np.float64):
        src = _readable(rng, ni, nj, nk, reach, fdtype)
        base = [np.full(9, 2.25), np.full(9, 1.5), np.full(9, 1.75)]
        ends = [(-1.0, ni + 1.0), (-2.0, nj - 1.0), (0.0, nk - 1.0)]
        axes = 3 if point_mode else 2
        for axis in range(axes):
            pos = [b.copy() for b in base[:axes]]
            pos[axis][:6] = [np.nan, np.inf, -np.inf, ends[axis][1], ends[axis][0], 2.0]
            args = pos + ([None] if not point_mode else [])
            clamp = S.sample(src, *args, method, reach, "clamp")
            assert np.isnan(clamp[0]).all() and not np.isnan(clamp[1:]).any()  # NaN passes through; nothing else is touched
            if method == "nearest":
                assert (np.atleast_1d(clamp[0]).view(S.UINT[src.itemsize]) == S.QNAN[src.itemsize]).all()
            assert S.same_bits(clamp[1], clamp[3]).all() and S.same_bits(clamp[2], clamp[4]).all()  # +-inf clamps to the ends
            assert S.same_bits(clamp[6:], np.repeat(clamp[6:7], 3, axis=0)).all()
            for fill_value in (-1.0e10, math.nan):
                fill = S.sample(src, *args, method, reach, "fill", fill_value)
                want = S.fill_item(fill_value, fdtype)
                for p in range(3):  # NaN, +inf, -inf: filled, in every level
                    assert S.same_bits(np.atleast_1d(fill[p]), np.full(np.atleast_1d(fill[p]).shape, want)).all()
                assert S.same_bits(fill[3:], clamp[3:]).all()  # every other point: exactly the bits of the clamp mode


def test_the_fill_value_is_rounded_once_to_the_item_type():
    src = np.zeros((2, 2, 2), dtype=np.float32)
    pi, pj = np.array([-1.0, 0.5]), np.array([0.0, 0.5])
    for value, want in ((16777217.0, 16777216.0), (1.0 + 2.0 ** -24 + 2.0 ** -50, 1.0 + 2.0 ** -23), (1e300, np.inf), (-1e-300, -0.0), (0.1, np.float32(0.1))):
        out = S.sample(src, pi, pj, None, "linear", (0, 0, 0, 0), "fill", value)
        assert out.dtype == np.float32 and S.same_bits(out[0], np.full(2, want, dtype=np.float32)).all(), value
        assert (out[1] == 0.0).all()
        assert S.same_bits(out, S.sample_plain(src, pi, pj, None, "linear", (0, 0, 0, 0), "fill", value)).all()
    out = S.sample(src.astype(np.float64), pi, pj, np.array([0.0, 5.0]), "cubic", (0, 0, 0, 0), "fill", 0.1)
    assert out.dtype == np.float64 and out.tolist() == [0.1, 0.1]  # (point mode: K beyond the last level)


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_header_signature_and_the_abi_is_still_8():
    E.check_binding("gt4mi_point_sample",
                    ["const gt4mi_field* dst", "const gt4mi_field* src", "int nfields", "const gt4mi_field* pos_i",
                     "const gt4mi_field* pos_j", "const gt4mi_field* pos_k", "int64_t npoints", "const int64_t extent[3]",
                     "const int64_t reach[4]", "int elem_size", "int pos_elem_size", "int method", "int flags", "double fill_value",
                     "void* stream", "int* launches"],
                    phrases=("no reference counterpart", "gt4mi_horizontal_interp in absolute mode", "gt4mi_departure_interp in absolute mode",
                             "K has no ghost levels", "p < xmin, p > xmax or p != p", "rounded once", "LAUNCH time",
                             "number or order of the points", "ceil(nfields / 8)"))
    assert "enum { GT4MI_SAMPLE_FILL = 2, GT4MI_SAMPLE_DRY_RUN = 256 };" in (E.ROOT / "include" / "gt4py_amd.h").read_text()
    assert (_lib.SAMPLE_FILL, _lib.SAMPLE_DRY_RUN) == (2, 256)


DST, SRC, PI, PJ, PK = 0x10_0000, 0x4000_0000, 0x8000_0000, 0xC000_0000, 0x1_0000_0000  # made-up device addresses, far apart
NP, NK = 10, 3


def _field(ptr, nk=NK, shape_ij=(8, 8), strides=None, origin=(2, 2, 0), itemsize=8):  # (nk first; this file's plane and origin)
    return E.field(ptr, (*shape_ij, nk), strides, origin, itemsize)


def _result(ptr, npoints=NP, nk=NK, strides=None, itemsize=8, origin=(0, 0, 0)):
    """One field's block of a C-ordered result: axis 0 the point, axis 1 the level (contiguous)."""
    if strides is None:
        strides = (nk * itemsize, itemsize, 0)
    return _lib.Field.make(ptr, (npoints, nk, 1), strides, origin)


def _list(ptr, npoints=NP, itemsize=8, stride=None):
    return _lib.Field.make(ptr, (npoints, 1, 1), (itemsize if stride is None else stride, 0, 0), (0, 0, 0))


def _call(dst, src, pi, pj, pk=None, nfields=1, npoints=NP, extent=(4, 4, NK), reach=(1, 1, 1, 1), size=8, pos_size=8, method=1, flags=0,
          fill_value=0.0):
    return E.call("gt4mi_point_sample", as_arg(dst), as_arg(src), nfields, as_arg(pi), as_arg(pj), as_arg(pk), npoints, int64s(extent),
                  int64s(reach), size, pos_size, method, flags | _lib.SAMPLE_DRY_RUN, fill_value, None, outs=(77,))


def test_every_refusal_of_the_c_entry_without_a_gpu():
    """Every check runs before the first launch: these calls carry made-up device addresses and the dry-run flag."""
    d, s, pi, pj, pk = _result(DST), _field(SRC), _list(PI), _list(PJ), _list(PK)
    d1 = _result(DST, nk=1)  # point mode: one item per point
    column, point = [d, s, pi, pj], [d1, s, pi, pj, pk]
    for good in (column, point):
        rc, msg, launches = _call(*good)
        assert rc == 0 and launches == 1, msg
    for method in range(4):
        for flags in (0, _lib.SAMPLE_FILL):
            for size, pos_size in ((4, 4), (4, 8), (8, 4)):
                args = [_result(DST, itemsize=size), _field(SRC, itemsize=size), _list(PI, itemsize=pos_size), _list(PJ, itemsize=pos_size)]
                rc, msg, launches = _call(*args, size=size, pos_size=pos_size, method=method, flags=flags, fill_value=math.nan)
                assert rc == 0 and launches == 1, msg
                args[0] = _result(DST, nk=1, itemsize=size)
                rc, msg, launches = _call(*args, _list(PK, itemsize=pos_size), size=size, pos_size=pos_size, method=method, flags=flags)
                assert rc == 0 and launches == 1, msg
    # null pointers (pos_k excepted: it selects the mode)
    for n, what in enumerate((b"dst is null", b"src is null", b"pos_i is null", b"pos_j is null")):
        args = list(point)
        args[n] = None
        rc, msg, launches = _call(*args)
        assert rc == INV and b"point_sample: " + what in msg and launches == 0, msg
    rc, msg, _ = _call(*column, extent=None)
    assert rc == INV and b"extent is null" in msg
    rc, msg, _ = _call(*column, reach=None)
    assert rc == INV and b"reach is null" in msg
    for n, what in enumerate((b"dst 0 is null", b"src 0 is null", b"pos_i 0 is null", b"pos_j 0 is null", b"pos_k 0 is null")):
        args = list(point)
        args[n] = _list(0) if n >= 2 else _field(0)
        rc, msg, launches = _call(*args)
        assert rc == INV and what in msg and launches == 0, msg
    # counts, extents, flags, method, reach
    for n in (0, -2):
        rc, msg, launches = _call(*column, nfields=n)
        assert rc == INV and b"nfields" in msg and launches == 0
    for n in (-1, 2 ** 31):
        rc, msg, launches = _call(*column, npoints=n)
        assert rc == INV and b"invalid npoints" in msg and launches == 0
    rc, msg, _ = _call(*column, extent=(4, -1, NK))
    assert rc == INV and b"invalid extent -1 along axis 1" in msg
    rc, msg, _ = _call(*column, extent=(4, 4, 2 ** 31))
    assert rc == INV and b"invalid extent 2147483648 along axis 2" in msg
    for flags in (1, 4, 512, 2 | 8):
        rc, msg, _ = _call(*column, flags=flags)
        assert rc == INV and b"flags" in msg
    for method in (4, -1):
        rc, msg, launches = _call(*column, method=method)
        assert rc == INV and b"unknown method" in msg and launches == 0
    for side in range(4):
        reach = [1, 1, 1, 1]
        reach[side] = -1
        rc, msg, _ = _call(*column, reach=reach)
        assert rc == INV and b"negative reach -1" in msg
    rc, msg, _ = _call(*column, reach=(2 ** 31, 0, 0, 0))
    assert rc == UNS and b"is too large" in msg
    # item sizes other than 4 or 8
    rc, msg, _ = _call(*column, size=2)
    assert rc == UNS and b"field item size 2" in msg
    rc, msg, _ = _call(*column, pos_size=16)
    assert rc == UNS and b"position item size 16" in msg
    # a box that does not fit its field: the (npoints, nk) box of a dst, the READABLE box of a src, the npoints items of a position array
    rc, msg, launches = _call(*column, npoints=NP + 1)
    assert rc == OOB and b"dst 0" in msg and b"axis 0" in msg and launches == 0
    rc, msg, _ = _call(_result(DST, nk=NK - 1), s, pi, pj)
    assert rc == OOB and b"dst 0" in msg and b"axis 1" in msg
    rc, msg, _ = _call(d, s, pi, pj, pk)  # point mode writes one item per point: a result with levels is fine, a src with fewer is not
    assert rc == 0, msg
    rc, msg, _ = _call(*column, extent=(6, 4, NK))  # src has no room for the reach behind 6 points
    assert rc == OOB and b"src 0" in msg and b"reach 1 along axis 0" in msg
    rc, msg, _ = _call(*column, extent=(6, 4, NK), reach=(1, 0, 1, 1))
    assert rc == 0, msg
    rc, msg, _ = _call(*column, reach=(1, 1, 3, 1))
    assert rc == OOB and b"src 0" in msg and b"axis 1 leaves no room for a reach of 3" in msg
    rc, msg, _ = _call(d, _field(SRC, nk=NK - 1), pi, pj)  # every level of a src is readable
    assert rc == OOB and b"src 0" in msg and b"axis 2" in msg
    rc, msg, _ = _call(d, s, _list(PI, npoints=NP - 1), pj)
    assert rc == OOB and b"pos_i 0" in msg and b"axis 0" in msg
    rc, msg, _ = _call(d1, s, pi, pj, _list(PK, npoints=NP - 1))
    assert rc == OOB and b"pos_k 0" in msg and b"axis 0" in msg
    rc, msg, _ = _call(d, _field(SRC, origin=(2, -1, 0)), pi, pj)
    assert rc == OOB and b"negative origin -1 along axis 1" in msg
    # strides and alignment the kernels do not take
    rc, msg, _ = _call(_result(DST, strides=(28, 8, 0)), s, pi, pj)
    assert rc == UNS and b"multiple of the item size" in msg
    rc, msg, _ = _call(_result(DST + 4), s, pi, pj)
    assert rc == UNS and b"dst 0 is not aligned to its item size" in msg
    rc, msg, _ = _call(d1, s, pi, pj, _list(PK + 4))
    assert rc == UNS and b"pos_k 0 is not aligned to its item size" in msg
    # stride 0: refused for a dst on an extent above 1, fine on an extent of 1; a src and a position array broadcast; any other stride
    rc, msg, launches = _call(_result(DST, strides=(0, 8, 0)), s, pi, pj)
    assert rc == INV and b"dst 0 has stride 0 along axis 0" in msg and launches == 0
    rc, msg, _ = _call(_result(DST, strides=(24, 0, 0)), s, pi, pj)
    assert rc == INV and b"dst 0 has stride 0 along axis 1" in msg
    rc, msg, _ = _call(_result(DST, strides=(24, 0, 0)), s, pi, pj, pk)  # point mode: one level
    assert rc == 0, msg
    rc, msg, _ = _call(_result(DST, strides=(8, 8 * NP, 0)), _field(SRC, strides=(8, 64, 0)), _list(PI, stride=0), _list(PJ, stride=24))
    assert rc == 0, msg  # a point-contiguous result, a Field[IJ] as src, one position for every point, a strided position array
    # overlap in memory: a dst against a src's READABLE box, each position array, another dst
    rc, msg, launches = _call(d, _field(DST), pi, pj)
    assert rc == UNS and b"dst 0 and src 0 overlap in memory" in msg and launches == 0
    last = 8 * (NP * NK - 1)  # byte offset of the dst box's last item
    ghost = 8 * (1 + 8 * 1)  # ... and of the first item of a src's readable box at reach 1
    rc, msg, _ = _call(d, _field(DST + last - ghost), pi, pj)  # the first ghost cell a gather may read IS dst's last item
    assert rc == UNS and b"dst 0 and src 0 overlap in memory" in msg
    rc, msg, _ = _call(d, _field(DST + last - ghost + 8), pi, pj)  # the byte ranges do not meet
    assert rc == 0, msg
    rc, msg, _ = _call(d, s, _list(DST + 64), pj)
    assert rc == UNS and b"dst 0 and pos_i overlap in memory" in msg
    rc, msg, _ = _call(d, s, pi, _list(DST + last))
    assert rc == UNS and b"dst 0 and pos_j overlap in memory" in msg
    rc, msg, _ = _call(d, s, pi, _list(DST + last + 8))
    assert rc == 0, msg
    rc, msg, _ = _call(d1, s, pi, pj, _list(DST + 8))
    assert rc == UNS and b"dst 0 and pos_k overlap in memory" in msg
    two = lambda a, b: E.table((a, b))  # noqa: E731
    rc, msg, _ = _call(two(d, _result(DST + 0x1000)), two(s, _field(DST + 64)), pi, pj, nfields=2)
    assert rc == UNS and b"dst 0 and src 1 overlap in memory" in msg
    rc, msg, _ = _call(two(d, _result(DST + last)), two(s, _field(SRC + 0x1000)), pi, pj, nfields=2)
    assert rc == UNS and b"dst 0 and dst 1 overlap in memory" in msg
    rc, msg, launches = _call(two(d, _result(DST + last + 8)), two(s, s), pi, pi, nfields=2)  # C order; one src twice; one array for both axes
    assert rc == 0 and launches == 1, msg
    # no points, or an extent with a zero entry: OK, nothing to launch -- after the checks
    for kwargs in (dict(npoints=0), dict(extent=(4, 0, NK)), dict(extent=(0, 4, NK)), dict(extent=(4, 4, 0))):
        rc, msg, launches = _call(*column, **kwargs)
        assert rc == 0 and launches == 0, (msg, kwargs)
    rc, msg, launches = _call(*point, npoints=0)
    assert rc == 0 and launches == 0, msg
    rc, msg, launches = _call(*column, npoints=0, extent=(7, 4, NK))
    assert rc == OOB and launches == 0


def test_launches_are_one_per_eight_fields():
    d = E.table(_result(DST + n * 8 * NP * NK) for n in range(9))  # the blocks of a C-ordered (9, NP, NK) result
    s = E.table(_field(SRC + n * 0x1000) for n in range(9))
    pi, pj, pk = _list(PI), _list(PJ), _list(PK)
    assert [_call(d, s, pi, pj, nfields=n)[2] for n in (1, 3, 8, 9)] == [1, 1, 1, 2]
    assert [_call(d, s, pi, pj, pk, nfields=n)[2] for n in (1, 3, 8, 9)] == [1, 1, 1, 2]


def test_the_kernels_are_in_the_resource_log_without_scratch():
    kernels = E.kernel_resources(r"point_sample_kernel")
    # 2 field types x 2 position types x 4 methods x the instantiations for 1, 4 and 8 entries x 2 modes
    assert len(kernels) == 96 and len({name for name, *_ in kernels}) == 96, kernels
    for name, scratch, waves, lds in kernels:
        assert int(scratch) == 0 and int(lds) == 0, (name, scratch, waves, lds)


# ---- the Python interface: every refusal before any GPU work ---------------------------------------------------------------
def _good(**over):
    args = dict(pos_i=E.host_field((7,)), pos_j=E.host_field((7,)))
    args.update(over)
    return E.host_field(HOST), args


@pytest.mark.parametrize("kwargs, error, match", [
    (dict(halo=2.0), ValueError, "halo must be"),
    (dict(halo=-1), ValueError, "must not be negative"),
    (dict(halo=5), ValueError, "leave no domain"),
    (dict(halo=2, origin=(1, 2, 0)), ValueError, "point_sample: src 0: origin 1 along axis 0 leaves no room for a reach of 2"),
    (dict(origin=(0, 0, 6)), ValueError, "leave no domain"),
    (dict(method="quintic"), ValueError, "method must be one of"),
    (dict(outside="wrap"), ValueError, "outside must be one of"),
    (dict(fill_value="zero"), TypeError, "fill_value must be a number"),
    (dict(out=E.host_field((1, 7, 4))), ValueError, r"out must have shape \(1, 7, 5\) and dtype float64"),
    (dict(out=E.host_field((1, 7, 5), "float32")), ValueError, "out must have shape"),
    (dict(pos_k=E.host_field((7,)), out=E.host_field((1, 7, 5))), ValueError, r"out must have shape \(1, 7\)"),
    (dict(halo=((1, 2), (0, 3)), method="cubic_monotone", outside="fill", fill_value=-1), TypeError, "sample works on device fields"),
    (dict(pos_k=E.host_field((7,)), out=E.host_field((1, 7))), TypeError, "sample works on device fields"),
    (dict(), TypeError, "sample works on device fields"),  # all checks passed: host arrays are refused last
])
def test_python_refusals_need_no_gpu(kwargs, error, match):
    field, pos = _good()
    pos.update(kwargs)
    with pytest.raises(error, match=match):
        sampling.sample(field, **pos)
    with pytest.raises(error, match=match):
        sampling.Sample([field], **pos)


def test_python_refusals_about_the_arrays_themselves(monkeypatch):
    import torch

    from gt4py_amd.storage.device_array import DeviceArray

    R = sampling.Sample
    field, pos = _good()
    # what Python itself refuses is refused before any library call
    calls = []
    real = _lib.load().gt4mi_point_sample
    monkeypatch.setattr(_lib.load(), "gt4mi_point_sample", lambda *a: calls.append(a) or real(*a))
    with pytest.raises(ValueError, match="at least one field"):
        R([], **pos)
    with pytest.raises(TypeError, match="host"):
        R(torch.zeros(10, 9, 5, dtype=torch.float64), **pos)  # as_device_array's own refusal
    with pytest.raises(TypeError):
        R(field, **dict(pos, pos_j=np.zeros(7)))
    with pytest.raises(ValueError, match="takes IJK fields"):
        R(E.host_field((10, 9)), **pos)
    with pytest.raises(ValueError, match="pos_j must be a 1-d array of positions, not an array of 2"):
        R(field, **dict(pos, pos_j=E.host_field((7, 1))))
    with pytest.raises(ValueError, match="pos_k must be a 1-d array of positions, not an array of 3"):
        R(field, **dict(pos, pos_k=E.host_field((10, 9, 5))))
    with pytest.raises(ValueError, match="pos_i and pos_j share a length: 7 and 8 differ"):
        R(field, **dict(pos, pos_j=E.host_field((8,))))
    with pytest.raises(ValueError, match="pos_i and pos_k share a length: 7 and 6 differ"):
        R(field, **dict(pos, pos_k=E.host_field((6,))))
    with pytest.raises(ValueError, match="at least one point"):
        R(field, pos_i=E.host_field((0,)), pos_j=E.host_field((0,)))
    with pytest.raises(TypeError, match="the fields of one call share a dtype"):
        R([field, E.host_field(HOST, dtype="float32")], **pos)
    with pytest.raises(TypeError, match="float32 or float64 fields"):
        R(E.host_field(HOST, dtype="int64"), **pos)
    with pytest.raises(TypeError, match="pos_i and pos_j share a dtype: float64 and float32 differ"):
        R(field, **dict(pos, pos_j=E.host_field((7,), "float32")))
    with pytest.raises(TypeError, match="pos_i and pos_k share a dtype"):
        R(field, **dict(pos, pos_k=E.host_field((7,), "float32")))
    with pytest.raises(TypeError, match="position arrays are float32 or float64"):
        R(field, pos_i=E.host_field((7,), "int32"), pos_j=E.host_field((7,), "int32"))
    assert not calls
    with pytest.raises(TypeError, match="device fields"):  # float32 fields against float64 positions is a combination of its own
        R(E.host_field(HOST, dtype="float32"), **pos)
    assert len(calls) == 1  # (the dry run)
    # the caller's result on top of a field, of a position array
    flat = E.host_field((7 * 5 + 7,))
    with pytest.raises(TypeError, match="dst 0 and pos_i overlap in memory"):
        R(field, pos_i=flat[:7], pos_j=pos["pos_j"], out=DeviceArray(flat.tensor[6:41].view(1, 7, 5)))
    big = E.host_field((10, 9, 5))
    with pytest.raises(TypeError, match="dst 0 and src 0 overlap in memory"):
        R(big, **pos, out=DeviceArray(big.tensor.view(-1)[:35].view(1, 7, 5)))
    with pytest.raises(TypeError, match="dst 0 and dst 1 overlap in memory"):
        R([field, E.host_field(HOST)], **pos, out=DeviceArray(flat.tensor[:35].view(1, 7, 5).expand(2, 7, 5)))


def test_a_frozen_call_knows_its_shapes_and_refuses_to_run_after_an_array_died(monkeypatch):
    """The weak references are taken last, behind the device check: what they guard is shown on a Sample whose device check is made
    to pass for host memory -- the call itself is never reached, the dead reference is found first."""
    E.on_device(monkeypatch)
    fields = [E.host_field((12, 9, 5), "float32") for _ in range(9)]
    pi, pj, pk = (E.host_field((11,), "float64") for _ in range(3))
    column = sampling.Sample(fields, pos_i=pi, pos_j=pj, method="cubic", halo=((2, 1), (1, 3)))
    assert (column.launches, column.domain, column.origin, column.npoints, column.method, column.outside) == (2, (9, 5, 5), (2, 1, 0), 11, "cubic", "clamp")
    assert column.result.shape == (9, 11, 5) and column.result.dtype == np.float32 and column.result.tensor.is_contiguous()
    assert column.column(8).shape == (11, 5) and column.column(8).ptr == column.result.ptr + 8 * 11 * 5 * 4
    with pytest.raises(IndexError):
        column.column(9)
    with pytest.raises(RuntimeError, match="has not been called yet"):
        column.get()
    out = E.host_field((9, 11), "float32")
    point = sampling.Sample(fields, pos_i=pi, pos_j=pj, pos_k=pk, outside="fill", fill_value=-1, out=out)
    assert point.result.ptr == out.ptr and point.result.shape == (9, 11) and point.column(2).shape == (11,)
    assert (point.launches, point.domain, point.fill_value, point.outside) == (2, (12, 9, 5), -1.0, "fill")
    del pk
    E.refuses_a_dead_array(point)
