"""``gt4py_amd.departure`` without a GPU: the two forms of the contract's restatement (tests/departure_interp_ref.py) held against
each other bit for bit, an anchor in exact rational arithmetic that shares no code with either, the reduction to
``horizontal_interp`` where every point stays on its own level, the limiter, every refusal of the C entry through the dry run
(made-up addresses that are never dereferenced), the declaration, the kernels' resources and the Python interface's argument
checks."""

import math
from fractions import Fraction

import numpy as np
import pytest

import departure_interp_ref as D
import entry_checks as E
import horizontal_interp_ref as H
from entry_checks import INV, OOB, UNS, as_arg, int64s
from gt4py_amd import _lib, departure

HOST = (10, 9, 5)  # the shape of a host field where a test states none
REACHES = [(0, 0, 0, 0), (1, 1, 1, 1), (2, 2, 2, 2), (3, 1, 0, 2)]


def _index_fields(ni, nj, nk):
    return [np.broadcast_to(np.arange(n, dtype=np.float64).reshape([-1 if ax == a else 1 for a in range(3)]), (ni, nj, nk)).copy()
            for ax, n in enumerate((ni, nj, nk))]


def _readable(rng, ni, nj, nk, reach, dtype=np.float64):
    return rng.uniform(-2, 2, (ni + reach[0] + reach[1], nj + reach[2] + reach[3], nk)).astype(dtype)


# ---- the two forms of the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nk", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("method", D.METHODS)
def test_the_plain_python_and_the_numpy_restatement_agree_bit_for_bit(method, nk):
    rng = np.random.default_rng([21, nk])
    ni, nj = 6, 5
    combos = [((0, 0, 0, 0), np.float64, np.float64, False), ((1, 1, 1, 1), np.float32, np.float32, True),
              ((2, 2, 2, 2), np.float32, np.float64, False), ((3, 1, 0, 2), np.float64, np.float32, True)]
    for reach, fdtype, pdtype, relative in combos:
        src = _readable(rng, ni, nj, nk, reach, fdtype)
        src[2, 1, 0], src[3, 3, nk - 1], src[0, 0, 0] = np.inf, np.nan, -0.0
        pi, pj, pk = rng.uniform(-4, ni + 3, (ni, nj, nk)), rng.uniform(-4, nj + 3, (ni, nj, nk)), rng.uniform(-2, nk + 1, (ni, nj, nk))
        for p in (pi, pj, pk):
            kind = rng.integers(0, 4, p.shape)
            p[...] = np.where(kind == 0, np.round(p), np.where(kind == 1, np.floor(p) + 0.5, p))  # integers and halves
        pi.flat[:8] = [0.5, -0.0, np.inf, -np.inf, 1e300, np.nan, float(-reach[0]), float(ni - 1 + reach[1])]
        pj.flat[3:9] = [2.5, np.nan, -1e300, float(nj - 1 + reach[3]), 1.0, float(-reach[2])]
        pk.flat[6:18] = [0.0, float(nk - 1), -0.0, 0.5, nk - 1.5, -3.0, nk + 2.0, np.inf, -np.inf, np.nan, 1e300, -1e300]
        if relative:
            pi, pj, pk = (p - x for p, x in zip((pi, pj, pk), _index_fields(ni, nj, nk)))
        pi, pj, pk = (p.astype(pdtype) for p in (pi, pj, pk))
        a = D.interp3(src, pi, pj, pk, method, relative, reach)
        b = D.interp3_plain(src, pi, pj, pk, method, relative, reach)
        assert a.dtype == b.dtype == src.dtype and D.same_bits(a, b).all(), (method, nk, reach, fdtype, pdtype, relative)
        # a Field[IJ] for pos_i / pos_j is the IJK field with the same items
        flat_i, flat_j = pi[:, :, 0].copy(), pj[:, :, 0].copy()
        if relative or nk == 1:
            c = D.interp3(src, flat_i, flat_j, pk, method, relative, reach)
            d = D.interp3(src, np.repeat(flat_i[:, :, None], nk, 2), np.repeat(flat_j[:, :, None], nk, 2), pk, method, relative, reach)
            assert D.same_bits(c, d).all()


# ---- an anchor that shares no code with the restatement: exact rational arithmetic -----------------------------------------------
def _lagrange(nodes, x):
    out = []
    for n in nodes:
        w = Fraction(1)
        for m in nodes:
            if m != n:
                w *= Fraction(x - m) / (n - m)
        out.append(w)
    return out


def _exact(src, x, y, z, method, reach):
    """The tensor-product Lagrange value of the integer field ``src`` (the readable box) at the exact position (x, y, z)
    (Fractions inside the domain), edge replication in I and J, the end-interval rule in K."""
    lo_i, hi_i, lo_j, hi_j = reach
    ni, nj, nk = src.shape[0] - lo_i - hi_i, src.shape[1] - lo_j - hi_j, src.shape[2]
    order = 2 if method == "linear" else 4

    def taps(p, first, last, taps_k=order):
        b = math.floor(p)
        nodes = (0, 1) if taps_k == 2 else (-1, 0, 1, 2)
        return [(min(max(b + m, first), last), w) for m, w in zip(nodes, _lagrange(nodes, p - b))]

    bk = math.floor(z)
    in_k = taps(z, 0, nk - 1, 4 if order == 4 and 1 <= bk <= nk - 3 else 2)
    total = Fraction(0)
    for c, wc in taps(x, -lo_i, ni - 1 + hi_i):
        for r, wr in taps(y, -lo_j, nj - 1 + hi_j):
            for level, wl in in_k:
                total += wc * wr * wl * int(src[c + lo_i, r + lo_j, level])
    return total


@pytest.mark.parametrize("nk", [1, 2, 3, 4, 6])
@pytest.mark.parametrize("method", ["linear", "cubic"])
def test_integer_fields_at_half_positions_equal_the_exact_tensor_product(method, nk):
    """At t in {0, 0.5} the weights are 0, 1, 1/2, -1/16 and 9/16; with small integers in the field every product and every sum of
    the contract's order of operations is exact in float64, so the result EQUALS the rational value."""
    rng = np.random.default_rng([22, nk])
    reach = (1, 2, 2, 1)
    ni, nj = 5, 4
    src = rng.integers(-9, 10, (ni + 3, nj + 3, nk)).astype(np.float64)
    pi = rng.integers(0, 2 * (ni - 1) + 1, (ni, nj, nk)) / 2.0
    pj = rng.integers(0, 2 * (nj - 1) + 1, (ni, nj, nk)) / 2.0
    pk = rng.integers(0, 2 * (nk - 1) + 1, (ni, nj, nk)) / 2.0
    pk.flat[:2] = [0.0, nk - 1.0]
    if nk > 1:
        pk.flat[2:4] = [0.5, nk - 1.5]  # the two end intervals
    out = D.interp3(src, pi, pj, pk, method, False, reach)
    want = np.empty_like(out)
    for at in np.ndindex(*out.shape):
        exact = _exact(src, Fraction(pi[at]), Fraction(pj[at]), Fraction(pk[at]), method, reach)
        want[at] = float(exact)
        assert Fraction(want[at]) == exact  # (representable)
    assert np.array_equal(out, want)
    assert len(np.unique(out)) > 5


# ---- the contract's properties ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["nearest", "linear", "cubic"])
def test_with_every_point_on_its_own_level_the_result_is_horizontal_interp_level_by_level(method):
    """pos_k = the point's own level: t_k = 0, the K weights are (1, 0) and (-0, 1, 0, -0), and on finite non-zero plane values
    w*P + 0*P' = P bit for bit."""
    rng = np.random.default_rng(23)
    assert [w.hex() for w in D.cubic_weights(0.0)] == [x.hex() for x in (-0.0, 1.0, 0.0, -0.0)]
    for nk in (1, 2, 3, 4, 7):
        for reach in REACHES:
            for dtype in (np.float32, np.float64):
                ni, nj = 8, 6
                src = (280.0 + _readable(rng, ni, nj, nk, reach) / 2.0).astype(dtype)
                pi, pj = rng.uniform(-4, ni + 3, (ni, nj, nk)), rng.uniform(-4, nj + 3, (ni, nj, nk))
                levels = _index_fields(ni, nj, nk)[2]
                want = H.interp(src, pi, pj, method, False, reach)
                assert D.same_bits(D.interp3(src, pi, pj, levels, method, False, reach), want).all(), (method, nk, reach)
                di, dj = rng.uniform(-3, 3, (ni, nj, nk)), rng.uniform(-3, 3, (ni, nj, nk))  # displacements; none along K
                want = H.interp(src, di, dj, method, True, reach)
                assert D.same_bits(D.interp3(src, di, dj, np.zeros_like(levels), method, True, reach), want).all(), (method, nk, reach)


def test_the_monotone_limiter_keeps_every_point_within_its_eight_corners():
    rng = np.random.default_rng(24)
    reach = (2, 2, 2, 2)
    for nk in (1, 2, 3, 6):
        ni, nj = 20, 15
        src = _readable(rng, ni, nj, nk, reach)
        pi, pj, pk = rng.uniform(-3, ni + 2, (ni, nj, nk)), rng.uniform(-3, nj + 2, (ni, nj, nk)), rng.uniform(-1, nk, (ni, nj, nk))
        pk.flat[:3] = [np.nan, 0.0, nk - 1.0]
        cubic = D.interp3(src, pi, pj, pk, "cubic", False, reach)
        mono = D.interp3(src, pi, pj, pk, "cubic_monotone", False, reach)
        b_i = np.floor(np.clip(pi, -2, ni + 1)).astype(int)
        b_j = np.floor(np.clip(pj, -2, nj + 1)).astype(int)
        b_k = np.floor(np.clip(np.where(np.isnan(pk), 0.0, pk), 0, nk - 1)).astype(int)
        corners = np.stack([src[np.clip(b_i + di, -2, ni + 1) + 2, np.clip(b_j + dj, -2, nj + 1) + 2, np.clip(b_k + dk, 0, nk - 1)]
                            for di in (0, 1) for dj in (0, 1) for dk in (0, 1)])
        mn, mx = corners.min(axis=0), corners.max(axis=0)
        ok = ~np.isnan(pk)
        assert np.isnan(mono[~ok]).all() and not np.isnan(mono[ok]).any()
        assert ((mono >= mn) & (mono <= mx))[ok].all()
        inside = (cubic >= mn) & (cubic <= mx) & ok
        assert inside.any() and (~inside & ok).any()  # both cases occur
        assert D.same_bits(mono[inside], cubic[inside]).all()
        assert ((mono == mn) | (mono == mx))[~inside & ok].all()


def test_the_end_interval_rule_along_k_and_a_nan_position():
    rng = np.random.default_rng(25)
    ni, nj, nk = 4, 3, 6
    src = _readable(rng, ni, nj, nk, (0, 0, 0, 0))
    pi, pj, _ = _index_fields(ni, nj, nk)
    for z, levels in ((0.25, (0, 1)), (nk - 1.75, (nk - 2, nk - 1)), (1.25, (0, 1, 2, 3)), (nk - 2.5, (nk - 4, nk - 3, nk - 2, nk - 1))):
        pk = np.full((ni, nj, nk), z)
        out = D.interp3(src, pi, pj, pk, "cubic")
        t = z - math.floor(z)
        if len(levels) == 2:
            want = (1.0 - t) * src[:, :, levels[0]] + t * src[:, :, levels[1]]
        else:
            w = D.cubic_weights(t)
            want = ((w[0] * src[:, :, levels[0]] + w[1] * src[:, :, levels[1]]) + w[2] * src[:, :, levels[2]]) + w[3] * src[:, :, levels[3]]
        assert np.array_equal(out, np.repeat(want[:, :, None], nk, 2)), z
        for level in range(nk):  # exactly the levels of the rule are read
            mask = np.zeros(src.shape, dtype=bool)
            mask[:, :, level] = True
            touched = D.stencil_touches(mask, pi, pj, pk, "cubic")
            assert touched.all() if level in levels else not touched.any(), (z, level)
    pk = _index_fields(ni, nj, nk)[2]
    pk[2, 1, 3] = np.nan
    for method in D.METHODS:
        out = D.interp3(src.astype(np.float32), pi, pj, pk, method)
        assert np.isnan(out[2, 1, 3]) and np.isnan(out).sum() == 1
    assert D.interp3(src.astype(np.float32), pi, pj, pk, "nearest").view(np.uint32)[2, 1, 3] == 0x7FC00000


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_header_signature_and_the_abi_is_still_8():
    E.check_binding("gt4mi_departure_interp",
                    ["const gt4mi_field* dst", "const gt4mi_field* src", "int nfields", "const gt4mi_field* pos_i",
                     "const gt4mi_field* pos_j", "const gt4mi_field* pos_k", "const int64_t extent[3]", "const int64_t reach[4]",
                     "int elem_size", "int pos_elem_size", "int method", "int flags", "void* stream", "int* launches"],
                    phrases=("no reference counterpart", "w0k*P(b_k) + w1k*P(b_k+1)", "1 <= b_k <= nk-3", "min(c011, c111)", "K has no ghost levels",
                             "0 * inf = NaN", "before any limiter"))


DST, SRC, PI, PJ, PK = 0x10_0000, 0x4000_0000, 0x8000_0000, 0xC000_0000, 0x1_0000_0000  # made-up device addresses, far apart
NK = 3


def _field(ptr, nk=NK, shape_ij=(8, 8), strides=None, origin=(2, 2, 0), itemsize=8):  # (nk first; this file's plane and origin)
    return E.field(ptr, (*shape_ij, nk), strides, origin, itemsize)


def _plane(ptr, shape_ij=(8, 8), origin=(2, 2, 0), itemsize=8):  # (positions; this file's plane and origin)
    return E.plane(ptr, shape_ij, origin, itemsize)


def _call(dst, src, pi, pj, pk, nfields=1, extent=(4, 4, NK), reach=(1, 1, 1, 1), size=8, pos_size=8, method=1, flags=0):
    return E.call("gt4mi_departure_interp", as_arg(dst), as_arg(src), nfields, as_arg(pi), as_arg(pj), as_arg(pk), int64s(extent), int64s(reach),
                  size, pos_size, method, flags | _lib.INTERP_DRY_RUN, None, outs=(77,))


def test_every_refusal_of_the_c_entry_without_a_gpu():
    """Every check runs before the first launch: these calls carry made-up device addresses and the dry-run flag."""
    d, s, pi, pj, pk = _field(DST), _field(SRC), _field(PI), _field(PJ), _field(PK)
    good = [d, s, pi, pj, pk]
    rc, msg, launches = _call(*good)
    assert rc == 0 and launches == 1, msg
    for method in range(4):
        for flags in (0, _lib.INTERP_RELATIVE):
            for size, pos_size in ((4, 4), (4, 8), (8, 4)):
                args = [_field(DST, itemsize=size), _field(SRC, itemsize=size), _field(PI, itemsize=pos_size), _plane(PJ, itemsize=pos_size),
                        _field(PK, itemsize=pos_size)]
                rc, msg, launches = _call(*args, size=size, pos_size=pos_size, method=method, flags=flags)
                assert rc == 0 and launches == 1, msg
    # null pointers
    for n, what in enumerate((b"dst is null", b"src is null", b"pos_i is null", b"pos_j is null", b"pos_k is null")):
        args = list(good)
        args[n] = None
        rc, msg, launches = _call(*args)
        assert rc == INV and b"departure_interp: " + what in msg and launches == 0, msg
    rc, msg, _ = _call(*good, extent=None)
    assert rc == INV and b"extent is null" in msg
    rc, msg, _ = _call(*good, reach=None)
    assert rc == INV and b"reach is null" in msg
    for n, what in enumerate((b"dst 0 is null", b"src 0 is null", b"pos_i 0 is null", b"pos_j 0 is null", b"pos_k 0 is null")):
        args = list(good)
        args[n] = _field(0)
        rc, msg, launches = _call(*args)
        assert rc == INV and what in msg and launches == 0, msg
    # counts, extents, flags, method, reach
    for n in (0, -2):
        rc, msg, launches = _call(*good, nfields=n)
        assert rc == INV and b"nfields" in msg and launches == 0
    rc, msg, _ = _call(*good, extent=(4, -1, NK))
    assert rc == INV and b"invalid extent -1 along axis 1" in msg
    rc, msg, _ = _call(*good, extent=(4, 4, 2 ** 31))
    assert rc == INV and b"invalid extent 2147483648 along axis 2" in msg
    for flags in (2, 512, 1 | 4):
        rc, msg, _ = _call(*good, flags=flags)
        assert rc == INV and b"flags" in msg
    for method in (4, -1):
        rc, msg, launches = _call(*good, method=method)
        assert rc == INV and b"unknown method" in msg and launches == 0
    for side in range(4):
        reach = [1, 1, 1, 1]
        reach[side] = -1
        rc, msg, _ = _call(*good, reach=reach)
        assert rc == INV and b"negative reach -1" in msg
    rc, msg, _ = _call(*good, reach=(2 ** 31, 0, 0, 0))
    assert rc == UNS and b"is too large" in msg
    # item sizes other than 4 or 8
    rc, msg, _ = _call(*good, size=2)
    assert rc == UNS and b"field item size 2" in msg
    rc, msg, _ = _call(*good, pos_size=16)
    assert rc == UNS and b"position item size 16" in msg
    # a box that does not fit its field: the box of a dst and of the position fields, the READABLE box of a src
    rc, msg, launches = _call(*good, extent=(7, 4, NK))
    assert rc == OOB and b"dst 0" in msg and b"axis 0" in msg and launches == 0
    rc, msg, _ = _call(*good, extent=(4, 4, NK + 1))
    assert rc == OOB and b"dst 0" in msg and b"axis 2" in msg
    rc, msg, _ = _call(*good, extent=(6, 4, NK))  # dst holds 6 from its origin, src has no room for the reach behind them
    assert rc == OOB and b"src 0" in msg and b"reach 1 along axis 0" in msg
    rc, msg, _ = _call(*good, extent=(6, 4, NK), reach=(1, 0, 1, 1))
    assert rc == 0, msg
    rc, msg, _ = _call(*good, reach=(1, 1, 3, 1))
    assert rc == OOB and b"src 0" in msg and b"axis 1 leaves no room for a reach of 3" in msg
    rc, msg, _ = _call(d, _field(SRC, nk=NK - 1), pi, pj, pk)  # every level of a src is readable
    assert rc == OOB and b"src 0" in msg and b"axis 2" in msg
    rc, msg, _ = _call(d, s, _field(PI, shape_ij=(5, 8)), pj, pk)
    assert rc == OOB and b"pos_i 0" in msg and b"axis 0" in msg
    rc, msg, _ = _call(d, s, pi, _field(PJ, nk=NK - 1), pk)
    assert rc == OOB and b"pos_j 0" in msg and b"axis 2" in msg
    rc, msg, _ = _call(d, s, _plane(PI), _plane(PJ), pk)  # a Field[IJ] has no shape to check along K
    assert rc == 0, msg
    rc, msg, _ = _call(d, s, pi, pj, _plane(PK))  # ... but pos_k is a full IJK box
    assert rc == OOB and b"pos_k 0" in msg and b"axis 2" in msg
    rc, msg, _ = _call(d, s, pi, pj, _plane(PK), extent=(4, 4, 1))
    assert rc == 0, msg
    rc, msg, _ = _call(d, s, pi, pj, _field(PK, shape_ij=(8, 5)))
    assert rc == OOB and b"pos_k 0" in msg and b"axis 1" in msg
    rc, msg, _ = _call(d, _field(SRC, origin=(2, -1, 0)), pi, pj, pk)
    assert rc == OOB and b"negative origin -1 along axis 1" in msg
    # strides and alignment the kernels do not take
    rc, msg, _ = _call(_field(DST, strides=(8, 68, 512)), s, pi, pj, pk)
    assert rc == UNS and b"multiple of the item size" in msg
    rc, msg, _ = _call(d, s, pi, pj, _field(PK + 4))
    assert rc == UNS and b"pos_k 0 is not aligned to its item size" in msg
    # stride 0: refused for a dst on an extent above 1, fine on an extent of 1; a src broadcasts
    rc, msg, launches = _call(_field(DST, strides=(0, 8, 64)), s, pi, pj, pk)
    assert rc == INV and b"dst 0 has stride 0 along axis 0" in msg and launches == 0
    rc, msg, _ = _call(_field(DST, strides=(8, 64, 0)), s, pi, pj, pk)
    assert rc == INV and b"dst 0 has stride 0 along axis 2" in msg
    rc, msg, _ = _call(d, _field(SRC, strides=(8, 64, 0)), pi, pj, pk)
    assert rc == 0, msg
    # overlap in memory: a dst against its src's READABLE box, another pair's src, each position field, another dst
    rc, msg, launches = _call(d, _field(DST), pi, pj, pk)
    assert rc == UNS and b"dst 0 and src 0 overlap in memory" in msg and launches == 0
    last = 8 * (5 + 8 * 5 + 64 * (NK - 1))  # byte offset of the dst box's last item
    ghost = 8 * (1 + 8 * 1)  # ... and of the first item of a src's readable box at reach 1
    rc, msg, _ = _call(d, _field(DST + last - ghost), pi, pj, pk)  # the first ghost cell the gather may read IS dst's last item
    assert rc == UNS and b"dst 0 and src 0 overlap in memory" in msg
    rc, msg, _ = _call(d, _field(DST + last - ghost + 8), pi, pj, pk)  # the byte ranges do not meet
    assert rc == 0, msg
    rc, msg, _ = _call(d, s, _field(DST + 64), pj, pk)
    assert rc == UNS and b"dst 0 and pos_i overlap in memory" in msg
    rc, msg, _ = _call(d, s, pi, _plane(DST + 8 * 20), pk)
    assert rc == UNS and b"dst 0 and pos_j overlap in memory" in msg
    rc, msg, _ = _call(d, s, pi, pj, _field(DST + 64))
    assert rc == UNS and b"dst 0 and pos_k overlap in memory" in msg
    two = lambda a, b: E.table((a, b))  # noqa: E731
    rc, msg, _ = _call(two(d, _field(DST + 0x1000)), two(s, _field(DST + 64)), pi, pj, pk, nfields=2)
    assert rc == UNS and b"dst 0 and src 1 overlap in memory" in msg
    rc, msg, _ = _call(two(d, _field(DST + 128)), two(s, _field(SRC + 0x1000)), pi, pj, pk, nfields=2)
    assert rc == UNS and b"dst 0 and dst 1 overlap in memory" in msg
    rc, msg, launches = _call(two(d, _field(DST + 0x1000)), two(s, s), pk, pk, pk, nfields=2)  # one src for two dsts, one field for all axes
    assert rc == 0 and launches == 1, msg
    # an extent with a zero entry: OK, nothing to launch -- after the checks
    for extent in ((4, 0, NK), (0, 4, NK), (4, 4, 0)):
        rc, msg, launches = _call(*good, extent=extent)
        assert rc == 0 and launches == 0, msg
    rc, msg, launches = _call(*good, extent=(7, 0, NK))
    assert rc == OOB and launches == 0


def test_launches_are_one_per_eight_pairs():
    d = E.table(_field(DST + n * 0x1000) for n in range(9))
    s = E.table(_field(SRC + n * 0x1000) for n in range(9))
    pi, pj, pk = _plane(PI), _plane(PJ), _field(PK)
    assert [_call(d, s, pi, pj, pk, nfields=n)[2] for n in (1, 8, 9)] == [1, 1, 2]


def test_the_kernels_are_in_the_resource_log_without_scratch():
    kernels = E.kernel_resources(r"departure_interp_kernel")
    # 2 field types x 2 position types x 4 methods x the instantiations for 1, 4 and 8 entries
    assert len(kernels) == 48 and len({name for name, *_ in kernels}) == 48, kernels
    for name, scratch, waves, lds in kernels:
        assert int(scratch) == 0 and int(lds) == 0, (name, scratch, waves, lds)


# ---- the Python interface: every refusal before any GPU work ---------------------------------------------------------------
def _good(**over):
    args = dict(dst=E.host_field(HOST), src=E.host_field(HOST), pos_i=E.host_field(HOST), pos_j=E.host_field((10, 9)), pos_k=E.host_field(HOST))
    args.update(over)
    return args.pop("dst"), args.pop("src"), args


@pytest.mark.parametrize("kwargs, error, match", [
    (dict(halo=2.0), ValueError, "halo must be"),
    (dict(halo=-1), ValueError, "must not be negative"),
    (dict(halo=5), ValueError, "leave no domain"),
    (dict(halo=2, origin=(1, 2, 0)), ValueError, "departure_interp: src 0: origin 1 along axis 0 leaves no room for a reach of 2"),
    (dict(origin=(0, 0, 6)), ValueError, "leave no domain"),
    (dict(method="quintic"), ValueError, "method must be one of"),
    (dict(halo=((1, 2), (0, 3)), method="cubic_monotone", relative=True), TypeError, "interpolate_3d works on device fields"),
    (dict(), TypeError, "interpolate_3d works on device fields"),  # all checks passed: host arrays are refused last
])
def test_python_refusals_need_no_gpu(kwargs, error, match):
    dst, src, pos = _good()
    with pytest.raises(error, match=match):
        departure.interpolate_3d(dst, src, **pos, **kwargs)
    with pytest.raises(error, match=match):
        departure.DepartureInterp([dst], [src], **pos, **kwargs)


def test_python_refusals_about_the_fields_themselves(monkeypatch):
    import torch

    R = departure.DepartureInterp
    dst, src, pos = _good()
    # what Python itself refuses is refused before any library call
    calls = []
    real = _lib.load().gt4mi_departure_interp
    monkeypatch.setattr(_lib.load(), "gt4mi_departure_interp", lambda *a: calls.append(a) or real(*a))
    with pytest.raises(ValueError, match="at least one"):
        R([], [], **pos)
    with pytest.raises(ValueError, match="2 destination.s. and 1 source"):
        R([dst, E.host_field(HOST)], [src], **pos)
    with pytest.raises(TypeError, match="host"):
        R(torch.zeros(10, 9, 5, dtype=torch.float64), src, **pos)  # as_device_array's own refusal
    with pytest.raises(TypeError):
        R(dst, src, **dict(pos, pos_k=np.zeros((10, 9, 5))))
    with pytest.raises(ValueError, match="takes IJK fields"):
        R(E.host_field((10, 9)), src, **pos)
    with pytest.raises(ValueError, match="pos_j must be an IJK field or a Field.IJ., not a field of 1"):
        R(dst, src, **dict(pos, pos_j=E.host_field((9,))))
    with pytest.raises(ValueError, match="pos_k must be an IJK field, not a field of 2 dimension"):
        R(dst, src, **dict(pos, pos_k=E.host_field((10, 9))))
    with pytest.raises(TypeError, match="the fields of one call share a dtype"):
        R(E.host_field(HOST, dtype="float32"), src, **pos)
    with pytest.raises(TypeError, match="float32 or float64 fields"):
        R(E.host_field(HOST, dtype="int64"), E.host_field(HOST, dtype="int64"), **pos)
    with pytest.raises(TypeError, match="pos_i and pos_j share a dtype"):
        R(dst, src, **dict(pos, pos_j=E.host_field((10, 9), "float32")))
    with pytest.raises(TypeError, match="pos_i and pos_k share a dtype: float64 and float32 differ"):
        R(dst, src, **dict(pos, pos_k=E.host_field(HOST, dtype="float32")))
    with pytest.raises(TypeError, match="position fields are float32 or float64"):
        R(dst, src, pos_i=E.host_field(HOST, dtype="int32"), pos_j=E.host_field(HOST, dtype="int32"), pos_k=E.host_field(HOST, dtype="int32"))
    with pytest.raises(ValueError, match="method must be one of"):
        R(dst, src, method="trilinear", **pos)
    assert not calls
    with pytest.raises(TypeError, match="device fields"):  # float32 fields against float64 positions is a combination of its own
        R(E.host_field(HOST, dtype="float32"), E.host_field(HOST, dtype="float32"), **pos)
    assert len(calls) == 1  # (the dry run)
    # a field onto itself; a dst that is also a position field
    x = E.host_field(HOST)
    with pytest.raises(TypeError, match="dst 0 and src 0 overlap in memory"):
        R(x, x, **pos)
    with pytest.raises(TypeError, match="dst 0 and pos_k overlap in memory"):
        R(x, src, **dict(pos, pos_k=x))


def test_a_frozen_call_knows_its_box_and_refuses_to_run_after_an_array_died(monkeypatch):
    """The weak references are taken last, behind the device check: what they guard is shown on a DepartureInterp whose device
    check is made to pass for host memory -- the call itself is never reached, the dead reference is found first."""
    E.on_device(monkeypatch)
    dsts, srcs = [E.host_field((10, 9, 5)) for _ in range(9)], [E.host_field((12, 9, 5)) for _ in range(9)]
    pi, pj, pk = E.host_field((10, 9), "float32"), E.host_field((10, 9, 5), "float32"), E.host_field((11, 9, 6), "float32")
    di = departure.DepartureInterp(dsts, srcs, pos_i=pi, pos_j=pj, pos_k=pk, method="cubic", relative=True, halo=((2, 1), (1, 3)))
    assert (di.launches, di.domain, di.origin, di.method, di.relative) == (2, (7, 5, 5), (2, 1, 0), "cubic", True)
    del pk
    E.refuses_a_dead_array(di)
