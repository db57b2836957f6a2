"""``gt4py_amd.horizontal`` without a GPU: properties of the arithmetic contract (on its restatement
tests/horizontal_interp_ref.py, whose plain-Python and numpy forms are held against each other bit for bit), every refusal of the C
entry through the dry run (made-up addresses that are never dereferenced), the declaration, the kernels' resources and the Python
interface's argument checks."""


import numpy as np
import pytest

import entry_checks as E
import horizontal_interp_ref as H
from entry_checks import INV, OOB, UNS, as_arg, int64s
from gt4py_amd import _lib, horizontal

HOST = (10, 9, 5)  # the shape of a host field where a test states none
REACHES = [(0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (3, 1, 0, 2)]


def _index_fields(ni, nj, nk=None):
    shape = (ni, nj) if nk is None else (ni, nj, nk)
    i_of = np.broadcast_to(np.arange(ni, dtype=np.float64).reshape((ni, 1) + (1,) * (len(shape) - 2)), shape)
    j_of = np.broadcast_to(np.arange(nj, dtype=np.float64).reshape((1, nj) + (1,) * (len(shape) - 2)), shape)
    return i_of.copy(), j_of.copy()


def _readable(rng, ni, nj, nk, reach, dtype=np.float64):
    return rng.uniform(-2, 2, (ni + reach[0] + reach[1], nj + reach[2] + reach[3], nk)).astype(dtype)


# ---- the two forms of the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", H.METHODS)
def test_the_plain_python_and_the_numpy_restatement_agree_bit_for_bit(method):
    rng = np.random.default_rng(11)
    for reach in REACHES:
        for fdtype, pdtype in ((np.float64, np.float64), (np.float32, np.float32), (np.float32, np.float64), (np.float64, np.float32)):
            for relative in (False, True):
                ni, nj, nk = 6, 5, 2
                src = _readable(rng, ni, nj, nk, reach, fdtype)
                src[2, 1, 0], src[3, 3, 1], src[0, 0, 0] = np.inf, np.nan, -0.0
                pi = rng.uniform(-4, ni + 3, (ni, nj, nk))
                pj = rng.uniform(-4, nj + 3, (ni, nj, nk))
                whole = rng.uniform(size=pi.shape) < 0.3
                pi[whole], pj[whole] = np.round(pi[whole]), np.round(pj[whole])  # some exact integers
                pi.flat[:8] = [0.5, -0.0, np.inf, -np.inf, 1e300, np.nan, float(-reach[0]), float(ni - 1 + reach[1])]
                pj.flat[3:9] = [2.5, np.nan, -1e300, float(nj - 1 + reach[3]), 1.0, float(-reach[2])]
                if relative:
                    i_of, j_of = _index_fields(ni, nj, nk)
                    pi, pj = pi - i_of, pj - j_of
                pi, pj = pi.astype(pdtype), pj.astype(pdtype)
                a = H.interp(src, pi, pj, method, relative, reach)
                b = H.interp_plain(src, pi, pj, method, relative, reach)
                assert a.dtype == b.dtype == src.dtype and H.same_bits(a, b).all(), (method, reach, fdtype, pdtype, relative)


def test_the_weights_of_the_cubic():
    assert [w.hex() for w in H.cubic_weights(0.0)] == [x.hex() for x in (-0.0, 1.0, 0.0, -0.0)]
    assert H.cubic_weights(0.5) == [-1 / 16, 9 / 16, 9 / 16, -1 / 16]
    rng = np.random.default_rng(12)
    worst = max(abs(sum(H.cubic_weights(float(t))) - 1.0) for t in rng.uniform(0, 1, 200_000))
    assert worst <= 4e-16, worst


# ---- the contract's properties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", H.METHODS)
def test_identity_integer_positions_return_the_source(method):
    rng = np.random.default_rng(13)
    for reach in REACHES:
        for dtype in (np.float32, np.float64):
            ni, nj, nk = 9, 7, 3
            src = _readable(rng, ni, nj, nk, reach, dtype)
            src[src == 0] = 1.0
            box = src[reach[0]:reach[0] + ni, reach[2]:reach[2] + nj]
            pi, pj = _index_fields(ni, nj)
            for relative, (a, b) in ((False, (pi, pj)), (True, (np.zeros_like(pi), np.zeros_like(pj)))):
                out = H.interp(src, a, b, method, relative, reach)
                assert np.array_equal(out, box)
                assert H.same_bits(out, np.ascontiguousarray(box)).all()  # nonzero values: bit-equal
            # zeros: numerically equal (-0.0 may come back as +0.0)
            src[reach[0] + 1, reach[2] + 1, 0] = -0.0
            assert np.array_equal(H.interp(src, pi, pj, method, False, reach), box)


def test_linear_reproduces_integer_affine_fields_at_eighths():
    rng = np.random.default_rng(14)
    reach = (1, 1, 1, 1)
    ni, nj, nk = 12, 10, 2
    a0, a1, a2 = (int(x) for x in rng.integers(-9, 10, 3))
    gi, gj = np.arange(-1, ni + 1, dtype=np.float64)[:, None, None], np.arange(-1, nj + 1, dtype=np.float64)[None, :, None]
    src = a0 + a1 * gi + a2 * gj + np.zeros((1, 1, nk))
    pi = rng.integers(0, 8 * (ni - 1), (ni, nj, nk)) / 8.0
    pj = rng.integers(0, 8 * (nj - 1), (ni, nj, nk)) / 8.0
    out = H.interp(src, pi, pj, H.LINEAR, False, reach)
    assert np.array_equal(out, a0 + a1 * pi + a2 * pj)


def test_cubic_reproduces_integer_cubics_at_halves():
    rng = np.random.default_rng(15)
    reach = (2, 2, 2, 2)
    ni, nj, nk = 10, 9, 2
    c = [int(x) for x in rng.integers(-5, 6, 8)]

    def f(x, y):
        return c[0] + c[1] * x + c[2] * y + c[3] * x * y + c[4] * x * x + c[5] * y * y * y + c[6] * x * x * x + c[7] * x * x * y

    gi, gj = np.arange(-2, ni + 2, dtype=np.float64)[:, None, None], np.arange(-2, nj + 2, dtype=np.float64)[None, :, None]
    src = f(gi, gj) + np.zeros((1, 1, nk))
    pi = rng.integers(0, ni - 1, (ni, nj, nk)) + 0.5
    pj = rng.integers(0, nj - 1, (ni, nj, nk)) + 0.5
    out = H.interp(src, pi, pj, H.CUBIC, False, reach)
    assert np.array_equal(out, f(pi, pj))  # (multiples of 1/256 of a few thousand: every operation is exact in float64)


def test_the_monotone_limiter():
    rng = np.random.default_rng(16)
    reach = (2, 2, 2, 2)
    ni, nj, nk = 40, 30, 3  # 3 600 points
    src = _readable(rng, ni, nj, nk, reach)
    pi, pj = rng.uniform(-3, ni + 2, (ni, nj, nk)), rng.uniform(-3, nj + 2, (ni, nj, nk))
    cubic = H.interp(src, pi, pj, H.CUBIC, False, reach)
    mono = H.interp(src, pi, pj, H.CUBIC_MONOTONE, False, reach)
    b_i = np.clip(np.floor(np.clip(pi, -2, ni + 1)).astype(int), -2, ni + 1)
    b_j = np.clip(np.floor(np.clip(pj, -2, nj + 1)).astype(int), -2, nj + 1)
    k_of = np.broadcast_to(np.arange(nk), (ni, nj, nk))
    corners = np.stack([src[np.clip(b_i + di, -2, ni + 1) + 2, np.clip(b_j + dj, -2, nj + 1) + 2, k_of] for di in (0, 1) for dj in (0, 1)])
    mn, mx = corners.min(axis=0), corners.max(axis=0)
    assert ((mono >= mn) & (mono <= mx)).all()
    inside = (cubic >= mn) & (cubic <= mx)
    assert 0.2 < inside.mean() < 1.0  # both cases occur
    assert H.same_bits(mono[inside], cubic[inside]).all()
    assert ((mono[~inside] == mn[~inside]) | (mono[~inside] == mx[~inside])).all()


@pytest.mark.parametrize("method", H.METHODS)
def test_positions_outside_the_box_return_the_edge_replicated_value(method):
    rng = np.random.default_rng(17)
    for reach in REACHES:
        ni, nj, nk = 6, 5, 2
        src = _readable(rng, ni, nj, nk, reach)
        lo_i, hi_i, lo_j, hi_j = reach
        pi, pj = _index_fields(ni, nj)
        for far in (7.0, 1e300, np.inf):
            out = H.interp(src, pi - far - lo_i - ni, pj, method, False, reach)  # beyond the low I end: the first readable column
            assert np.array_equal(out, np.broadcast_to(src[0:1, lo_j:lo_j + nj], out.shape))
            out = H.interp(src, pi, pj + far + hi_j + nj, method, False, reach)  # beyond the high J end: the last readable row
            assert np.array_equal(out, np.broadcast_to(src[lo_i:lo_i + ni, -1:], out.shape))
        # xmin and xmax themselves
        out = H.interp(src, np.full_like(pi, -lo_i), np.full_like(pj, nj - 1 + hi_j), method, False, reach)
        assert np.array_equal(out, np.broadcast_to(src[0:1, -1:], out.shape))


@pytest.mark.parametrize("method", H.METHODS)
def test_broadcast_positions_and_relative_mode(method):
    rng = np.random.default_rng(18)
    reach = (3, 1, 0, 2)
    ni, nj, nk = 8, 6, 4
    src = _readable(rng, ni, nj, nk, reach, np.float32)
    pi, pj = rng.uniform(-4, ni + 2, (ni, nj)), rng.uniform(-1, nj + 3, (ni, nj))
    a = H.interp(src, pi, pj, method, False, reach)
    b = H.interp(src, np.repeat(pi[:, :, None], nk, axis=2), np.repeat(pj[:, :, None], nk, axis=2), method, False, reach)
    assert H.same_bits(a, b).all()
    # relative mode IS absolute mode with the index added (in float64: the one addition of step 1)
    di, dj = rng.uniform(-3, 3, (ni, nj)), rng.uniform(-3, 3, (ni, nj))
    i_of, j_of = _index_fields(ni, nj)
    assert H.same_bits(H.interp(src, di, dj, method, True, reach), H.interp(src, i_of + di, j_of + dj, method, False, reach)).all()


def test_documented_consequences():
    src = np.ones((4, 4, 1))
    src[2, 1, 0] = np.inf
    pi, pj = _index_fields(4, 4)
    out = H.interp(src, pi, pj, H.LINEAR, False)
    assert np.isnan(out[1, 1, 0]) and np.isnan(out[2, 0, 0]) and np.isinf(out[2, 1, 0])  # 0 * inf next to the infinity
    assert out[0, 0, 0] == 1.0 and out[3, 1, 0] == 1.0
    assert np.isinf(H.interp(src, pi, pj, H.NEAREST, False)[2, 1, 0]) and not np.isnan(H.interp(src, pi, pj, H.NEAREST, False)).any()
    pi[1, 2] = np.nan
    for method in H.METHODS:
        out = H.interp(np.ones((4, 4, 2), dtype=np.float32), pi, pj, method, False)
        assert np.isnan(out[1, 2]).all() and np.isnan(out).sum() == 2
    assert H.interp(np.ones((4, 4, 1), dtype=np.float32), pi, pj, H.NEAREST).view(np.uint32)[1, 2, 0] == 0x7FC00000
    payload = np.ones((4, 4, 1))
    payload.view(np.uint64)[3, 3, 0] = 0x7FF4_0000_DEAD_BEEF
    assert H.interp(payload, pi, pj, H.NEAREST).view(np.uint64)[3, 3, 0] == 0x7FF4_0000_DEAD_BEEF  # the item is moved


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_header_signature_and_the_abi_is_still_8():
    # the header states the contract and that the reference has no counterpart; the enums of header and binding agree
    E.check_binding("gt4mi_horizontal_interp",
                    ["const gt4mi_field* dst", "const gt4mi_field* src", "int nfields", "const gt4mi_field* pos_i",
                     "const gt4mi_field* pos_j", "const int64_t extent[3]", "const int64_t reach[4]", "int elem_size",
                     "int pos_elem_size", "int method", "int flags", "void* stream", "int* launches"],
                    prefix="INTERP", constants=("NEAREST", "LINEAR", "CUBIC", "CUBIC_MONOTONE", "RELATIVE", "DRY_RUN"),
                    phrases=("no reference counterpart", "fancy indexing", "floor(x + 0.5)", "w0j*r0 + w1j*r1", "((a*t)*c) / 6.0", "edge replication",
                             "0 * inf = NaN"))
    assert horizontal.METHODS == {"nearest": 0, "linear": 1, "cubic": 2, "cubic_monotone": 3}


DST, SRC, PI, PJ = 0x10_0000, 0x4000_0000, 0x8000_0000, 0xC000_0000  # made-up device addresses, far apart
NK = 3


def _field(ptr, nk=NK, shape_ij=(8, 8), strides=None, origin=(2, 2, 0), itemsize=8):  # (nk first; this file's plane and origin)
    return E.field(ptr, (*shape_ij, nk), strides, origin, itemsize)


def _plane(ptr, shape_ij=(8, 8), origin=(2, 2, 0), itemsize=8):  # (positions; this file's plane and origin)
    return E.plane(ptr, shape_ij, origin, itemsize)


def _call(dst, src, pi, pj, nfields=1, extent=(4, 4, NK), reach=(1, 1, 1, 1), size=8, pos_size=8, method=1, flags=0):
    return E.call("gt4mi_horizontal_interp", as_arg(dst), as_arg(src), nfields, as_arg(pi), as_arg(pj), int64s(extent), int64s(reach),
                  size, pos_size, method, flags | _lib.INTERP_DRY_RUN, None, outs=(77,))


def test_every_refusal_of_the_c_entry_without_a_gpu():
    """Every check runs before the first launch: these calls carry made-up device addresses and the dry-run flag."""
    d, s, pi, pj = _field(DST), _field(SRC), _field(PI), _field(PJ)
    rc, msg, launches = _call(d, s, pi, pj)
    assert rc == 0 and launches == 1, msg
    for method in range(4):
        for flags in (0, _lib.INTERP_RELATIVE):
            for size, pos_size in ((4, 4), (4, 8), (8, 4)):
                args = [_field(DST, itemsize=size), _field(SRC, itemsize=size), _field(PI, itemsize=pos_size), _plane(PJ, itemsize=pos_size)]
                rc, msg, launches = _call(*args, size=size, pos_size=pos_size, method=method, flags=flags)
                assert rc == 0 and launches == 1, msg
    # null pointers
    for n, what in enumerate((b"dst is null", b"src is null", b"pos_i is null", b"pos_j is null")):
        args = [d, s, pi, pj]
        args[n] = None
        rc, msg, launches = _call(*args)
        assert rc == INV and what in msg and launches == 0, msg
    rc, msg, _ = _call(d, s, pi, pj, extent=None)
    assert rc == INV and b"extent is null" in msg
    rc, msg, _ = _call(d, s, pi, pj, reach=None)
    assert rc == INV and b"reach is null" in msg
    for n, what in enumerate((b"dst 0 is null", b"src 0 is null", b"pos_i 0 is null", b"pos_j 0 is null")):
        args = [d, s, pi, pj]
        args[n] = _field(0)
        rc, msg, launches = _call(*args)
        assert rc == INV and what in msg and launches == 0, msg
    # counts, extents, flags, method, reach
    for n in (0, -2):
        rc, msg, launches = _call(d, s, pi, pj, nfields=n)
        assert rc == INV and b"nfields" in msg and launches == 0
    rc, msg, _ = _call(d, s, pi, pj, extent=(4, -1, NK))
    assert rc == INV and b"invalid extent -1 along axis 1" in msg
    for flags in (2, 512, 1 | 4):
        rc, msg, _ = _call(d, s, pi, pj, flags=flags)
        assert rc == INV and b"flags" in msg
    for method in (4, -1):
        rc, msg, launches = _call(d, s, pi, pj, method=method)
        assert rc == INV and b"unknown method" in msg and launches == 0
    for side in range(4):
        reach = [1, 1, 1, 1]
        reach[side] = -1
        rc, msg, _ = _call(d, s, pi, pj, reach=reach)
        assert rc == INV and b"negative reach -1" in msg
    # item sizes other than 4 or 8
    rc, msg, _ = _call(d, s, pi, pj, size=2)
    assert rc == UNS and b"field item size 2" in msg
    rc, msg, _ = _call(d, s, pi, pj, pos_size=16)
    assert rc == UNS and b"position item size 16" in msg
    # a box that does not fit its field: the box of a dst and of the position fields, the READABLE box of a src
    rc, msg, launches = _call(d, s, pi, pj, extent=(7, 4, NK))
    assert rc == OOB and b"dst 0" in msg and b"axis 0" in msg and launches == 0
    rc, msg, _ = _call(d, s, pi, pj, extent=(4, 4, NK + 1))
    assert rc == OOB and b"dst 0" in msg and b"axis 2" in msg
    rc, msg, _ = _call(d, s, pi, pj, extent=(6, 4, NK))  # dst holds 6 from its origin, src has no room for the reach behind them
    assert rc == OOB and b"src 0" in msg and b"reach 1 along axis 0" in msg
    rc, msg, _ = _call(d, s, pi, pj, extent=(6, 4, NK), reach=(1, 0, 1, 1))
    assert rc == 0, msg
    rc, msg, _ = _call(d, s, pi, pj, reach=(1, 1, 3, 1))
    assert rc == OOB and b"src 0" in msg and b"axis 1 leaves no room for a reach of 3" in msg
    rc, msg, _ = _call(d, s, pi, pj, reach=(2, 2, 2, 2))
    assert rc == 0, msg
    rc, msg, _ = _call(d, s, pi, pj, reach=(2, 2, 2, 3))
    assert rc == OOB and b"src 0" in msg and b"axis 1" in msg
    rc, msg, _ = _call(d, s, _field(PI, shape_ij=(5, 8)), pj)
    assert rc == OOB and b"pos_i 0" in msg and b"axis 0" in msg
    rc, msg, _ = _call(d, s, pi, _field(PJ, nk=NK - 1))
    assert rc == OOB and b"pos_j 0" in msg and b"axis 2" in msg
    rc, msg, _ = _call(d, s, pi, _plane(PJ))  # a Field[IJ] has no shape to check along K
    assert rc == 0, msg
    rc, msg, _ = _call(d, _field(SRC, origin=(2, -1, 0)), pi, pj)
    assert rc == OOB and b"negative origin -1 along axis 1" in msg
    # strides and alignment the kernels do not take
    rc, msg, _ = _call(_field(DST, strides=(8, 68, 512)), s, pi, pj)
    assert rc == UNS and b"multiple of the item size" in msg
    rc, msg, _ = _call(d, s, _field(PI + 4), pj)
    assert rc == UNS and b"not aligned to its item size" in msg
    # stride 0: refused for a dst on an extent above 1, fine on an extent of 1; a src broadcasts
    rc, msg, launches = _call(_field(DST, strides=(0, 8, 64)), s, pi, pj)
    assert rc == INV and b"dst 0 has stride 0 along axis 0" in msg and launches == 0
    rc, msg, _ = _call(_field(DST, strides=(8, 64, 0)), s, pi, pj)
    assert rc == INV and b"dst 0 has stride 0 along axis 2" in msg
    rc, msg, _ = _call(_field(DST, strides=(8, 64, 0)), s, pi, pj, extent=(4, 4, 1))
    assert rc == 0, msg
    rc, msg, _ = _call(d, _field(SRC, strides=(8, 64, 0)), pi, pj)
    assert rc == 0, msg
    # overlap in memory: a dst against its src's READABLE box, another pair's src, a position field, another dst
    rc, msg, launches = _call(d, _field(DST), pi, pj)
    assert rc == UNS and b"dst 0 and src 0 overlap in memory" in msg and launches == 0
    first, last = 8 * (2 + 8 * 2), 8 * (5 + 8 * 5 + 64 * (NK - 1))  # byte offsets of the dst box's first and last item
    ghost = 8 * (1 + 8 * 1)  # ... and of the first item of a src's readable box at reach 1
    rc, msg, _ = _call(d, _field(DST + last - ghost), pi, pj)  # the first ghost cell the gather may read IS dst's last item
    assert rc == UNS and b"dst 0 and src 0 overlap in memory" in msg
    rc, msg, _ = _call(d, _field(DST + last - ghost + 8), pi, pj)  # the byte ranges do not meet
    assert rc == 0, msg
    rc, msg, _ = _call(d, _field(DST + last - first), pi, pj, reach=(0, 0, 0, 0))  # without reach: src's first item IS dst's last
    assert rc == UNS and b"overlap in memory" in msg
    rc, msg, _ = _call(d, _field(DST + last - first + 8), pi, pj, reach=(0, 0, 0, 0))
    assert rc == 0, msg
    rc, msg, _ = _call(d, s, _field(DST + 64), pj)
    assert rc == UNS and b"dst 0 and pos_i overlap in memory" in msg
    rc, msg, _ = _call(d, s, pi, _plane(DST + 8 * 20))
    assert rc == UNS and b"dst 0 and pos_j overlap in memory" in msg
    two = lambda a, b: E.table((a, b))  # noqa: E731
    rc, msg, _ = _call(two(d, _field(DST + 0x1000)), two(s, _field(DST + 64)), pi, pj, nfields=2)
    assert rc == UNS and b"dst 0 and src 1 overlap in memory" in msg
    rc, msg, _ = _call(two(d, _field(DST + 128)), two(s, _field(SRC + 0x1000)), pi, pj, nfields=2)
    assert rc == UNS and b"dst 0 and dst 1 overlap in memory" in msg
    rc, msg, launches = _call(two(d, _field(DST + 0x1000)), two(s, s), pi, pi, nfields=2)  # one src for two dsts, one field for both axes
    assert rc == 0 and launches == 1, msg
    # an extent with a zero entry: OK, nothing to launch -- after the checks
    for extent in ((4, 0, NK), (0, 4, NK), (4, 4, 0)):
        rc, msg, launches = _call(d, s, pi, pj, extent=extent)
        assert rc == 0 and launches == 0, msg
    rc, msg, launches = _call(d, s, pi, pj, extent=(7, 0, NK))
    assert rc == OOB and launches == 0


def test_launches_are_one_per_eight_pairs():
    d = E.table(_field(DST + n * 0x1000) for n in range(9))
    s = E.table(_field(SRC + n * 0x1000) for n in range(9))
    pi, pj = _plane(PI), _plane(PJ)
    assert [_call(d, s, pi, pj, nfields=n)[2] for n in (1, 3, 8, 9)] == [1, 1, 1, 2]


def test_the_kernels_are_in_the_resource_log_without_scratch():
    kernels = E.kernel_resources(r"horizontal_interp_kernel")
    # 2 field types x 2 position types x 4 methods x the instantiations for 1, 4 and 8 entries
    assert len(kernels) == 48 and len({name for name, *_ in kernels}) == 48, kernels
    for name, scratch, waves, lds in kernels:
        assert int(scratch) == 0 and int(waves) >= 2 and int(lds) == 0, (name, scratch, waves, lds)


# ---- the Python interface: every refusal before any GPU work ---------------------------------------------------------------
def _good(**over):
    args = dict(dst=E.host_field(HOST), src=E.host_field(HOST), pos_i=E.host_field(HOST), pos_j=E.host_field((10, 9)))
    args.update(over)
    return args.pop("dst"), args.pop("src"), args


@pytest.mark.parametrize("kwargs, error, match", [
    (dict(halo=2.0), ValueError, "halo must be"),
    (dict(halo=((1, 1.5), (1, 1))), TypeError, "halo widths must be ints"),
    (dict(halo=-1), ValueError, "must not be negative"),
    (dict(halo=5), ValueError, "leave no domain"),
    (dict(halo=2, origin=(1, 2, 0)), ValueError, "axis 0 leaves no room for a reach of 2"),
    (dict(origin=(0, 0, 0, 0)), ValueError, "at most three entries"),
    (dict(origin=(0, 0, 6)), ValueError, "leave no domain"),
    (dict(method="quintic"), ValueError, "method must be one of"),
    (dict(halo=((1, 2), (0, 3)), method="cubic_monotone", relative=True), TypeError, "device fields"),  # all checks passed
    (dict(), TypeError, "device fields"),
])
def test_python_refusals_need_no_gpu(kwargs, error, match):
    dst, src, pos = _good()
    with pytest.raises(error, match=match):
        horizontal.interpolate(dst, src, **pos, **kwargs)
    with pytest.raises(error, match=match):
        horizontal.HorizontalInterp([dst], [src], **pos, **kwargs)


def test_python_refusals_about_the_fields_themselves():
    import torch

    R = horizontal.interpolate
    dst, src, pos = _good()
    with pytest.raises(ValueError, match="at least one"):
        R([], [], **pos)
    with pytest.raises(ValueError, match="2 destination.s. and 1 source"):
        R([dst, E.host_field(HOST)], [src], **pos)
    with pytest.raises(TypeError, match="host"):
        R(torch.zeros(10, 9, 5, dtype=torch.float64), src, **pos)  # as_device_array's own refusal
    with pytest.raises(TypeError):
        R(dst, np.zeros((10, 9, 5)), **pos)
    with pytest.raises(TypeError):
        R(dst, src, pos_i=np.zeros((10, 9)), pos_j=pos["pos_j"])
    with pytest.raises(ValueError, match="takes IJK fields"):
        R(E.host_field((10, 9)), src, **pos)
    with pytest.raises(ValueError, match="pos_j must be an IJK field or a Field.IJ."):
        R(dst, src, pos_i=pos["pos_i"], pos_j=E.host_field((9,)))
    # dtypes: the fields share one, the position fields share one (not necessarily the same), all float32 or float64
    with pytest.raises(TypeError, match="share a dtype"):
        R(E.host_field(HOST, dtype="float32"), src, **pos)
    with pytest.raises(TypeError, match="float32 or float64 fields"):
        R(E.host_field(HOST, dtype="int64"), E.host_field(HOST, dtype="int64"), **pos)
    with pytest.raises(TypeError, match="pos_i and pos_j share a dtype"):
        R(dst, src, pos_i=pos["pos_i"], pos_j=E.host_field((10, 9), "float32"))
    with pytest.raises(TypeError, match="position fields are float32 or float64"):
        R(dst, src, pos_i=E.host_field(HOST, dtype="int32"), pos_j=E.host_field(HOST, dtype="int32"))
    with pytest.raises(TypeError, match="device fields"):  # float32 fields against float64 positions is a combination of its own
        R(E.host_field(HOST, dtype="float32"), E.host_field(HOST, dtype="float32"), **pos)
    # a field onto itself; a dst that is also a position field
    x = E.host_field(HOST)
    with pytest.raises(TypeError, match="dst 0 and src 0 overlap in memory"):
        R(x, x, **pos)
    with pytest.raises(TypeError, match="dst 0 and pos_i overlap in memory"):
        R(x, src, pos_i=x, pos_j=pos["pos_j"])


def test_a_frozen_interpolation_knows_its_box_and_refuses_to_run_after_an_array_died(monkeypatch):
    """The weak references are taken last, behind the device check: what they guard is shown on a HorizontalInterp whose device
    check is made to pass for host memory -- the call itself is never reached, the dead reference is found first."""
    E.on_device(monkeypatch)
    dsts, srcs = [E.host_field((10, 9, 5)) for _ in range(9)], [E.host_field((12, 9, 6)) for _ in range(9)]
    pi, pj = E.host_field((10, 9), "float32"), E.host_field((10, 9, 5), "float32")
    hi = horizontal.HorizontalInterp(dsts, srcs, pos_i=pi, pos_j=pj, method="cubic", relative=True, halo=((2, 1), (1, 3)))
    assert (hi.launches, hi.domain, hi.origin, hi.method, hi.relative) == (2, (7, 5, 5), (2, 1, 0), "cubic", True)
    del pi
    E.refuses_a_dead_array(hi)
