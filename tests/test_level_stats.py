"""Per-level statistics (``gt4mi_level_stats``, ``diagnostics.LevelStats``) without a GPU: the C entry's declaration and constants,
every refusal (before any GPU work), the dry run's workspace and launch counts, the numpy restatement of the documented order
(tests/level_stats_ref.py) against exact arithmetic, ``Profile`` / ``merge_profiles``, and the kernels' resources."""

import ctypes
import math
import re

import numpy as np
import pytest

import entry_checks as E
import level_stats_ref as R
from entry_checks import INV, OOB, UNS, int64s
from gt4py_amd import _lib, diagnostics

HOST = (8, 9, 3)  # the shape of a host field where a test states none
U = 2.0 ** -53
PARAMS = ["const gt4mi_field* fields", "const gt4mi_field* others", "int nfields", "const int64_t domain[3]", "int elem_size",
          "void* workspace", "int64_t workspace_bytes", "double* result", "int flags", "void* stream", "int64_t* workspace_needed",
          "int* launches"]


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_header_signature_and_abi_8():
    FP, c_int, vp = ctypes.POINTER(_lib.Field), ctypes.c_int, ctypes.c_void_p
    types = [FP, FP, c_int, ctypes.POINTER(ctypes.c_int64), c_int, vp, ctypes.c_int64, vp, c_int, vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(c_int)]
    E.check_binding("gt4mi_level_stats", PARAMS, argtypes=types,
                    phrases=("no reference counterpart", "function of (ni, nj) alone", "partial[((entry * nk + k) * TL + t) * 8 + slot]",
                             "result[(entry * 9 + row) * nk + k]", "ceil(nfields / 8) + 1"))
    E.check_binding("gt4mi_field_stats", PARAMS, argtypes=types)  # the signature of gt4mi_field_stats


def test_constants_of_the_header_the_binding_and_the_restatement_agree():
    text = (E.ROOT / "include" / "gt4py_amd.h").read_text()
    header = {name: int(re.search(rf"GT4MI_LEVEL_STATS_{name}\s*=?\s*(\d+)", text).group(1)) for name in ("MEAN", "ROWS", "MAX_TILES")}
    assert header == {"MEAN": 8, "ROWS": 9, "MAX_TILES": _lib.LEVEL_STATS_MAX_TILES}
    assert (_lib.LEVEL_STATS_MEAN, _lib.LEVEL_STATS_ROWS) == (8, 9) == (R.MEAN, R.ROWS)
    assert R.MAX_TILES == _lib.LEVEL_STATS_MAX_TILES  # the restatement keeps its own copy
    assert (R.COUNT, R.NONFINITE, R.SUM, R.SUM_ABS, R.SUM_SQ, R.MIN, R.MAX, R.DOT) == tuple(
        getattr(_lib, f"STATS_{n}") for n in ("COUNT", "NONFINITE", "SUM", "SUM_ABS", "SUM_SQ", "MIN", "MAX", "DOT"))
    assert diagnostics.PROFILE_ROWS == diagnostics.Stats._fields + ("mean",) and len(diagnostics.PROFILE_ROWS) == R.ROWS
    # the library was built with the same constant: 4 * LT rows give LT tiles, one row more gives 2 rows per wave
    for nj, tiles in ((4 * R.MAX_TILES, R.MAX_TILES), (4 * R.MAX_TILES + 1, (4 * R.MAX_TILES + 1 + 7) // 8)):
        shape = (4, nj, 2)
        f = ctypes.byref(_lib.Field.make(0x10000, shape, (8, 32, 32 * nj), (0, 0, 0)))
        rc, msg, launches, needed = _call(f, domain=shape, workspace=None, result=None)
        assert rc == 0 and needed == 2 * tiles * 64 and R.geometry(4, nj)[1] == tiles, (nj, msg, needed)


FIELD = (0x10000, (6, 6, 2), (8, 48, 288), (1, 1, 0))  # a fake device address: no call below reaches the GPU
WORK, RESULT = 0x900000, 0xA00000
NEEDED = 2 * 1 * 64  # domain (4, 4, 2): 2 levels of 4 rows, one per wave: one tile of 8 doubles each


def _field(ptr=FIELD[0], shape=FIELD[1], strides=FIELD[2], origin=FIELD[3]):  # (everything defaults to FIELD)
    return E.field(ptr, shape, strides, origin)


def _call(fields, others=None, nfields=1, domain=(4, 4, 2), elem_size=8, workspace=WORK, workspace_bytes=1 << 20, result=RESULT,
          flags=_lib.STATS_DRY_RUN):
    """Refusals are provoked WITHOUT the dry-run flag (a refused call enqueues nothing); a call that would pass every check
    carries the flag."""
    rc, msg, needed, launches = E.call("gt4mi_level_stats", fields, others, nfields, int64s(domain), elem_size, workspace, workspace_bytes, result,
                                       flags, None, outs=(ctypes.c_int64(-5), 77))
    return rc, msg, launches, needed


def test_argument_errors_of_the_c_entry_without_a_gpu():
    f = ctypes.byref(_field())

    def refused(status, needle, *args, **kwargs):
        kwargs.setdefault("flags", 0)  # a real call: the refusal is what keeps it from the GPU
        rc, msg, launches, _ = _call(*args, **kwargs)
        assert rc == status and needle in msg and launches == 0, (rc, msg, launches)

    refused(INV, b"level_stats: fields is null", None)
    refused(INV, b"level_stats: field 0 is null", ctypes.byref(_field(ptr=0)))
    refused(INV, b"level_stats: nfields = 0", f, nfields=0)
    refused(INV, b"level_stats: nfields = -2", f, nfields=-2)
    refused(INV, b"domain is null", f, domain=None)
    refused(UNS, b"level_stats: item size 2", f, elem_size=2)
    refused(UNS, b"level_stats: item size 16", f, elem_size=16)
    refused(INV, b"level_stats: empty domain", f, domain=(4, 0, 2))
    refused(INV, b"level_stats: empty domain", f, domain=(4, 4, 0))
    refused(INV, b"invalid domain size -1", f, domain=(4, 4, -1))
    refused(INV, b"level_stats: unknown bits in flags", f, flags=6)
    refused(OOB, b"level_stats: field 0: origin 1 + domain 6 along axis 0 is outside the array", f, domain=(6, 4, 2))
    refused(OOB, b"along axis 2 is outside the array", f, domain=(4, 4, 3))
    refused(OOB, b"level_stats: field 0: negative origin", ctypes.byref(_field(origin=(1, -1, 0))))
    refused(UNS, b"level_stats: field 0 is not aligned to its item size", ctypes.byref(_field(ptr=0x10004)))
    refused(UNS, b"byte stride 52 along axis 1 is not a multiple of the item size", ctypes.byref(_field(strides=(8, 52, 312))))
    refused(INV, b"level_stats: field 0 has stride 0 along axis 0", ctypes.byref(_field(strides=(0, 8, 48))))
    refused(INV, b"level_stats: field 0 has stride 0 along axis 2", ctypes.byref(_field(strides=(8, 48, 0))))
    # the second field: the same checks, except that a stride of 0 is a broadcast axis without a shape
    other = ctypes.byref(_field(ptr=0x20000))
    refused(UNS, b"level_stats: other 0 is not aligned", f, ctypes.byref(_field(ptr=0x20002)))
    refused(OOB, b"level_stats: other 0: origin 1 + domain 4 along axis 1", f, ctypes.byref(_field(ptr=0x20000, shape=(6, 4, 2))))
    weight = ctypes.byref(_field(ptr=0x20000, shape=(6, 6, 1), strides=(8, 48, 0)))  # IJ against IJK
    rc, msg, launches, needed = _call(f, weight)
    assert rc == 0 and launches == 2 and needed == NEEDED, msg
    rc, msg, launches, _ = _call(f, other)
    assert rc == 0 and launches == 2, msg
    # workspace and result
    refused(INV, b"level_stats: workspace is null", f, workspace=None)
    refused(INV, b"level_stats: result is null", f, result=None)
    refused(INV, b"level_stats: workspace of 127 bytes is too small, 128 are needed", f, workspace_bytes=NEEDED - 1)
    refused(INV, b"level_stats: workspace is not aligned to 8 bytes", f, workspace=WORK + 4)
    refused(INV, b"level_stats: result is not aligned to 8 bytes", f, result=RESULT + 4)
    # the domain of FIELD starts 8 + 48 = 56 bytes in; its last point is 4 * 8 + 4 * 48 + 288 = 512 bytes in and ends at 520;
    # the result of one entry and two levels is 9 * 2 * 8 = 144 bytes
    refused(INV, b"level_stats: result overlaps field 0", f, result=FIELD[0] + 56)
    refused(INV, b"level_stats: result overlaps field 0", f, result=FIELD[0] + 512)
    refused(INV, b"level_stats: result overlaps field 0", f, result=FIELD[0] + 56 - 136)  # its last double only
    refused(INV, b"level_stats: workspace overlaps field 0", f, workspace=FIELD[0] - NEEDED + 64)
    refused(INV, b"level_stats: workspace overlaps other 0", f, other, workspace=0x20000 + 512)
    refused(INV, b"level_stats: workspace overlaps result", f, result=WORK + 8)
    refused(INV, b"level_stats: workspace overlaps result", f, workspace=RESULT + 136)
    assert _call(f, result=FIELD[0] + 520)[0] == 0 and _call(f, result=FIELD[0] + 56 - 144)[0] == 0  # next to the domain: fine
    assert _call(f, workspace=RESULT + 144)[0] == 0
    # too small buffers are refused by the dry run as well when they are passed
    rc, msg, launches, _ = _call(f, workspace_bytes=8)
    assert rc == INV and b"too small" in msg and launches == 0
    # a level of more than 2^40 points
    big = (2 ** 21, 2 ** 20, 1)
    refused(UNS, b"level_stats: more than 2^40 points in a level", ctypes.byref(_field(shape=big, strides=(8, 2 ** 24, 2 ** 44), origin=(0, 0, 0))),
            domain=big, workspace=None, result=None)
    rc, msg, launches, _ = _call(ctypes.byref(_field(shape=(2 ** 20, 2 ** 20, 2), strides=(8, 2 ** 23, 2 ** 43), origin=(0, 0, 0))),
                                 domain=(2 ** 20, 2 ** 20, 2), workspace=None, result=None)
    assert rc == 0 and launches == 2, msg  # 2^41 points, 2^40 per level: what field_stats refuses passes here


def test_dry_run_reports_workspace_and_launches():
    many = E.table(_field(ptr=0x10000 * (n + 1)) for n in range(17))
    for n, want in ((1, 2), (8, 2), (9, 3), (16, 3), (17, 4)):
        rc, msg, launches, needed = _call(many, nfields=n, workspace=None, result=None)  # asking for the size
        assert rc == 0 and launches == want and needed == n * NEEDED, (n, msg)
    # the workspace follows the tile partition of the restatement: a function of nj alone per level, at most LT tiles
    for domain in ((512, 512, 128), (1024, 1024, 80), (17, 33, 5), (3, 70000, 3), (5, 1030, 3), (3, 771, 2), (9, 1, 40), (700, 5, 3)):
        big = ctypes.byref(_field(shape=domain, strides=(8, 8 * domain[0], 8 * domain[0] * domain[1]), origin=(0, 0, 0)))
        rc, msg, launches, needed = _call(big, domain=domain, workspace=None, result=None)
        tiles = R.geometry(*domain[:2])[1]
        assert rc == 0 and launches == 2 and needed == domain[2] * tiles * 64 and 0 < tiles <= R.MAX_TILES, (domain, msg)


def test_the_kernels_are_in_the_resource_log_and_use_no_scratch():
    """No scratch, LDS only for the per-workgroup combine, and no fewer waves per SIMD than the field_stats kernel of the same
    item type in the same log."""
    found = E.kernel_resources(r"(?:field|level)_stats")
    kernels = {}
    for name, scratch, waves, lds in found:
        family = "level" if "level_stats" in name else "field"
        kind = "finish" if "finish" in name else ("float" if re.search(r"IfE|<float>", name) else "double" if re.search(r"IdE|<double>", name) else name)
        kernels[family, kind] = (int(scratch), int(waves), int(lds))
    assert sorted(kernels) == sorted((f, k) for f in ("field", "level") for k in ("float", "double", "finish")), found
    for kind in ("float", "double"):
        scratch, waves, lds = kernels["level", kind]
        assert scratch == 0 and lds == 4 * 8 * 8, (kind, kernels)
        assert waves >= kernels["field", kind][1], (kind, kernels)
    assert kernels["level", "finish"][0] == 0 and kernels["level", "finish"][2] == 0, kernels


# ---- the restatement against exact arithmetic -------------------------------------------------------------------------------
DOMAINS = [(1, 1, 1), (3, 5, 2), (17, 33, 5), (64, 64, 8), (65, 63, 7), (130, 40, 3), (300, 37, 2), (700, 5, 3), (5, 1030, 3),
           (3, 771, 2)]


def test_geometry():
    assert R.geometry(1, 1) == (1, 1, 1) and R.geometry(700, 5) == (1, 2, 3) and R.geometry(256, 128) == (1, 32, 1)
    assert R.geometry(257, 129) == (2, 17, 2) and R.geometry(1024, 1024) == (8, 32, 4) and R.geometry(512, 512) == (4, 32, 2)
    assert R.halvings(29) == [29, 15, 8, 4, 2, 1] and R.halvings(1) == [1]
    for ni, nj, _ in DOMAINS:
        rw, tiles, chunks = R.geometry(ni, nj)
        assert 1 <= tiles <= R.MAX_TILES and 4 * rw * (tiles - 1) < nj <= 4 * rw * tiles and 256 * (chunks - 1) < ni <= 256 * chunks


def test_depth_counts_the_longest_chain():
    assert R.depth(1, 1) == 4 + 6 + 3  # one chunk of one row: 4 items of a lane, the butterfly, the waves
    assert R.depth(512, 512) == 4 * 2 * 4 + 6 + 3 + 5  # 4 rows per wave, 2 chunks, 32 tiles: 5 halvings
    assert R.depth(1024, 1024) == 8 * 4 * 4 + 6 + 3 + 5
    assert R.depth(5, 1030) == 9 * 1 * 4 + 6 + 3 + 5  # 29 -> 15 -> 8 -> 4 -> 2 -> 1


def _exact_int(a, b=None):
    a = a.astype(np.int64)
    x = a if b is None else a - np.broadcast_to(b.astype(np.int64), a.shape)
    dot = np.zeros(a.shape[2], np.int64) if b is None else (a * np.broadcast_to(b.astype(np.int64), a.shape)).sum(axis=(0, 1))
    plane = a.shape[0] * a.shape[1]
    return np.array([np.full(a.shape[2], plane), np.zeros(a.shape[2], np.int64), x.sum(axis=(0, 1)), np.abs(x).sum(axis=(0, 1)),
                     (x * x).sum(axis=(0, 1)), x.min(axis=(0, 1)), x.max(axis=(0, 1)), dot])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_is_exact_on_integer_data(dtype):
    """|x| <= 1000 (2000 for a difference): every partial sum in ANY order is an integer below 2^53, so any correct order gives
    numpy's int64 result exactly; the mean is one division of the two."""
    rng = np.random.default_rng(5)
    for domain in DOMAINS:
        a = rng.integers(-1000, 1000, domain, endpoint=True).astype(dtype)
        b = rng.integers(-1000, 1000, domain, endpoint=True).astype(dtype)
        w = rng.integers(0, 1000, domain[:2] + (1,), endpoint=True).astype(dtype)
        for other in (None, b, w):
            got = R.profile(a, other)
            want = _exact_int(a, other).astype(np.float64)
            assert got.shape == (9, domain[2]) and np.array_equal(got[:8], want), (domain, dtype)
            assert np.array_equal(got[R.MEAN], want[R.SUM] / want[R.COUNT])
    assert R.profile(rng.integers(-9, 9, (6, 7)).astype(dtype))[:, 0].tolist()[0] == 42.0  # an IJ field: one level


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_agrees_with_fsum_within_the_derived_bound(dtype):
    """Per level, depth * 2^-53 * sum |term|: the terms (x, |x|, x * x, a * b) are float64 numbers before they are added, each
    passes through at most `depth` additions, the first of them onto +0.0 and exact: (1 + u)^(depth - 1) - 1 <= depth u while
    depth^2 u << 1."""
    rng = np.random.default_rng(6)
    for domain in DOMAINS:
        a = (rng.standard_normal(domain) * 10.0 ** rng.integers(-3, 4, domain)).astype(dtype)
        b = rng.uniform(-2, 2, domain).astype(dtype)
        depth = R.depth(*domain[:2])
        assert depth ** 2 < 2 ** 53
        for other in (None, b):
            got = R.profile(a, other)
            for slot, term in zip((R.SUM, R.SUM_ABS, R.SUM_SQ, R.DOT), R.terms(a, other)):
                if term is None:
                    assert not got[slot].any()
                    continue
                for k in range(domain[2]):
                    exact, scale = math.fsum(term[:, :, k].ravel()), math.fsum(np.abs(term[:, :, k]).ravel())
                    assert abs(got[slot, k] - exact) <= depth * U * scale, (domain, dtype, slot, k, got[slot, k], exact)
            x = R.terms(a, other)[0]
            assert np.array_equal(got[R.MIN], x.min(axis=(0, 1))) and np.array_equal(got[R.MAX], x.max(axis=(0, 1)))
            assert not got[R.NONFINITE].any() and (got[R.COUNT] == domain[0] * domain[1]).all()


def test_a_level_of_the_restatement_depends_on_its_plane_alone():
    rng = np.random.default_rng(8)
    plane = rng.standard_normal((65, 63)) * 10.0 ** rng.integers(-3, 4, (65, 63))
    alone = R.profile(plane)[:, 0]
    box = rng.standard_normal((65, 63, 7))
    box[:, :, 3] = plane
    assert R.same_bits(R.profile(box)[:, 3], alone) and R.same_bits(R.profile(plane[:, :, None])[:, 0], alone)


def test_restatement_special_values():
    z = np.zeros((5, 3, 3))
    z[1::2, :, 0] = -0.0
    z[:, :, 2] = -0.0
    got = R.profile(z)
    assert np.signbit(got[R.MIN]).tolist() == [True, False, True] and np.signbit(got[R.MAX]).tolist() == [False, False, True]
    a = np.ones((5, 3, 3))
    a[4, 2, 1] = np.nan
    a[0, 0, 2] = -np.inf
    got = R.profile(a)
    assert got[R.NONFINITE].tolist() == [0, 1, 1]
    assert all(np.isnan(got[s, 1]) for s in (R.SUM, R.SUM_ABS, R.SUM_SQ, R.MIN, R.MAX, R.MEAN)) and not np.isnan(got[:, [0, 2]]).any()
    assert got[R.MIN, 2] == -np.inf and got[R.SUM_ABS, 2] == np.inf and got[R.MEAN, 2] == -np.inf and got[R.SUM, 0] == 15.0


# ---- Profile and merge_profiles ----------------------------------------------------------------------------------------------
def _profile(rows):
    return diagnostics.Profile.from_rows(np.asarray(rows, dtype=np.float64))


def test_profile_record():
    rows = np.array([[4, 4, 4], [0, 1, 2], [2.0, math.nan, math.inf], [6.0, math.nan, math.inf], [16.0, math.nan, math.inf],
                     [-3.0, math.nan, -1.0], [2.5, math.nan, math.inf], [0.5, 0.0, 0.0], [0.5, math.nan, math.inf]])
    p = _profile(rows)
    assert p.nk == len(p) == 3 and p.count.dtype == np.int64 and p.nonfinite.dtype == np.int64 and p.sum.dtype == np.float64
    assert p.count.tolist() == [4, 4, 4] and p.nonfinite.tolist() == [0, 1, 2] and p.mean[0] == 0.5
    assert p.all_finite.tolist() == [True, False, False] and p.first_nonfinite == 1
    assert p.max_abs[0] == 3.0 and math.isnan(p.max_abs[1]) and p.max_abs[2] == math.inf and p.norm2[0] == 4.0
    assert p[0] == diagnostics.Stats(4, 0, 2.0, 6.0, 16.0, -3.0, 2.5, 0.5) and isinstance(p[0].count, int)
    assert p[0].mean == p.mean[0] and p[-1].nonfinite == 2
    with pytest.raises(IndexError):
        p[3]
    assert _profile(rows[:, :1]).first_nonfinite is None
    total = p.total()
    assert R.same_bits(tuple(total), tuple(diagnostics.merge([p[0], p[1], p[2]])))
    assert total.count == 12 and total.nonfinite == 3 and math.isnan(total.min) and total.dot == 0.5
    # left to right over the levels
    q = diagnostics.Profile([1, 1, 1], [0, 0, 0], [1.0, 1e16, -1e16], [1.0, 1e16, 1e16], [1.0, 1e32, 1e32], [1.0, 1e16, -1e16],
                            [1.0, 1e16, -1e16], [0.0, 0.0, 0.0])
    assert q.total().sum == (1.0 + 1e16) + -1e16 == 0.0 and q.mean.tolist() == [1.0, 1e16, -1e16]
    assert p == _profile(rows) and p != q
    with pytest.raises(ValueError, match=r"\(9, nk\)"):
        diagnostics.Profile.from_rows(np.zeros((8, 3)))
    with pytest.raises(ValueError, match="one length"):
        diagnostics.Profile([1, 1], [0, 0], [1.0], [1.0], [1.0], [1.0], [1.0], [1.0])


def test_merge_profiles_joins_level_by_level_in_the_order_given():
    P = diagnostics.Profile
    #            level 0: sums whose order shows; level 1: signed zeros; level 2: a NaN in the second part
    a = P([10, 5, 3], [0, 0, 0], [1.0, 0.0, 2.0], [1.0, 0.0, 2.0], [1.0, 0.0, 4.0], [-2.0, 0.0, 2.0], [3.0, -0.0, 2.0], [0.5, 0.0, 0.0])
    b = P([5, 5, 3], [1, 0, 1], [1e16, 0.0, math.nan], [1e16, 0.0, math.nan], [2.0, 0.0, math.nan], [-1.0, -0.0, math.nan],
          [1e16, 0.0, math.nan], [0.25, 0.0, 0.0])
    c = P([7, 5, 3], [2, 0, 0], [-1e16, 0.0, 1.0], [1e16, 0.0, 1.0], [4.0, 0.0, 1.0], [-1e16, 0.0, 1.0], [0.0, -0.0, 1.0], [0.125, 0.0, 0.0])
    m = diagnostics.merge_profiles([a, b, c])
    assert m.count.tolist() == [22, 15, 9] and m.nonfinite.tolist() == [3, 0, 1] and m.first_nonfinite == 0
    assert m.sum[0] == (1.0 + 1e16) + -1e16 == 0.0 and diagnostics.merge_profiles([c, b, a]).sum[0] == (-1e16 + 1e16) + 1.0 == 1.0
    assert m.dot[0] == 0.875 and m.sum_sq[0] == 7.0 and (m.min[0], m.max[0]) == (-1e16, 1e16)
    assert m.mean[0] == 0.0 / 22 and diagnostics.merge_profiles([c, b, a]).mean[0] == 1.0 / 22  # recomputed from the joined sum
    for order in ([a, b, c], [c, b, a], [b, a, c]):
        z = diagnostics.merge_profiles(order)
        assert z.min[1] == 0 and np.signbit(z.min[1]) and z.max[1] == 0 and not np.signbit(z.max[1])
        assert all(math.isnan(v[2]) for v in (z.sum, z.min, z.max, z.mean)) and z.count[2] == 9
        for k in range(3):
            assert R.same_bits(tuple(z[k]), tuple(diagnostics.merge([p[k] for p in order])))
    assert diagnostics.merge_profiles([a]) == a
    with pytest.raises(ValueError, match="nk = 3 and 2 differ"):
        diagnostics.merge_profiles([a, P([1, 1], [0, 0], [1.0, 1.0], [1.0, 1.0], [1.0, 1.0], [1.0, 1.0], [1.0, 1.0], [0.0, 0.0])])
    with pytest.raises(ValueError, match="at least one"):
        diagnostics.merge_profiles([])
    with pytest.raises(TypeError, match="Profile records"):
        diagnostics.merge_profiles([a, a[0]])


# ---- the Python interface: every refusal before any GPU work ---------------------------------------------------------------
def test_python_refusals_need_no_gpu():
    D = diagnostics
    with pytest.raises(ValueError, match="at least one field"):
        D.level_stats()
    with pytest.raises(TypeError, match="float32 or float64 fields, not int32"):
        D.level_stats(E.host_field(HOST, dtype="int32"))
    with pytest.raises(TypeError, match="share a dtype"):
        D.level_stats(E.host_field(HOST), other=E.host_field(HOST, dtype="float32"))
    with pytest.raises(ValueError, match="one entry .* per field: 1 for 2 fields"):
        D.LevelStats([E.host_field(HOST), E.host_field(HOST)], others=[E.host_field(HOST)])
    with pytest.raises(ValueError, match="IJ or IJK fields"):
        D.level_stats(E.host_field((8,)))
    with pytest.raises(ValueError, match="leave no domain"):
        D.level_stats(E.host_field(HOST), halo=4)
    with pytest.raises(ValueError, match="level_stats: field 0: origin 0 \\+ domain 4 along axis 2 is outside the array"):
        D.level_stats(E.host_field(HOST), origin=(0, 0, 0), domain=(8, 9, 4))
    with pytest.raises(ValueError, match="level_stats: other 0: origin 1 \\+ domain 7 along axis 1"):
        D.level_stats(E.host_field(HOST), other=E.host_field((8, 7, 3)), halo=1)
    with pytest.raises(ValueError, match="level_stats: empty domain"):
        D.level_stats(E.host_field(HOST), domain=(3, 3, 0))
    # all checks passed (an IJ weight against an IJK field, levels 1-2 only, an IJ field): refused for being host memory
    for kwargs in (dict(), dict(halo=2), dict(other=E.host_field((8, 9))), dict(origin=(1, 1, 1), domain=(2, 2, 2))):
        with pytest.raises(TypeError, match="device fields"):
            D.level_stats(E.host_field(HOST), **kwargs)
    with pytest.raises(TypeError, match="device fields"):
        D.LevelStats([E.host_field((8, 9), "float32")], halo=((1, 2), (0, 3)))  # Field[IJ]: nk = 1
