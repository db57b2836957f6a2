"""``gt4py_amd.diagnostics`` without a GPU: the C entry's declaration, every refusal (before any GPU work), the numpy
restatement of the documented order (tests/stats_ref.py) against exact arithmetic, ``merge``, and the kernels' resources."""

import ctypes
import math

import numpy as np
import pytest

import entry_checks as E
import stats_ref as R
from entry_checks import INV, OOB, UNS, int64s
from gt4py_amd import _lib, diagnostics

HOST = (8, 9, 3)  # the shape of a host field where a test states none
U = 2.0 ** -53
# domain -> (rows, rows per wave, tiles, tiles per finish leaf, finish leaves)
SEVERAL_ROWS_PER_WAVE = {(5, 130, 130): (16900, 2, 2113, 17, 125), (3, 257, 129): (33153, 3, 2763, 22, 126)}


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_header_signature_and_abi_8():
    FP, c_int, vp = ctypes.POINTER(_lib.Field), ctypes.c_int, ctypes.c_void_p
    E.check_binding("gt4mi_field_stats",
                    ["const gt4mi_field* fields", "const gt4mi_field* others", "int nfields", "const int64_t domain[3]",
                     "int elem_size", "void* workspace", "int64_t workspace_bytes", "double* result", "int flags", "void* stream",
                     "int64_t* workspace_needed", "int* launches"],
                    argtypes=[FP, FP, c_int, ctypes.POINTER(ctypes.c_int64), c_int, vp, ctypes.c_int64, vp, c_int, vp,
                              ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(c_int)],
                    prefix="STATS", constants=("COUNT", "NONFINITE", "SUM", "SUM_ABS", "SUM_SQ", "MIN", "MAX", "DOT", "SLOTS", "DRY_RUN"),
                    phrases=("no reference counterpart",))
    assert diagnostics.Stats._fields == ("count", "nonfinite", "sum", "sum_abs", "sum_sq", "min", "max", "dot")
    assert (R.COUNT, R.NONFINITE, R.SUM, R.SUM_ABS, R.SUM_SQ, R.MIN, R.MAX, R.DOT) == tuple(range(8))


FIELD = (0x10000, (6, 6, 2), (8, 48, 288), (1, 1, 0))  # a fake device address: no call below reaches the GPU
WORK, RESULT = 0x900000, 0xA00000
NEEDED = 2 * 8 * 8  # domain (4, 4, 2): 8 rows, one per wave, 4 waves per tile: 2 tiles of 8 doubles


def _field(ptr=FIELD[0], shape=FIELD[1], strides=FIELD[2], origin=FIELD[3]):  # (everything defaults to FIELD)
    return E.field(ptr, shape, strides, origin)


def _call(fields, others=None, nfields=1, domain=(4, 4, 2), elem_size=8, workspace=WORK, workspace_bytes=1 << 20, result=RESULT,
          flags=_lib.STATS_DRY_RUN):
    """Refusals are provoked WITHOUT the dry-run flag where they can be (a refused call enqueues nothing); a call that would
    pass every check carries the flag."""
    rc, msg, needed, launches = E.call("gt4mi_field_stats", fields, others, nfields, int64s(domain), elem_size, workspace, workspace_bytes, result,
                                       flags, None, outs=(ctypes.c_int64(-5), 77))
    return rc, msg, launches, needed


def test_argument_errors_of_the_c_entry_without_a_gpu():
    f = ctypes.byref(_field())

    def refused(status, needle, *args, **kwargs):
        kwargs.setdefault("flags", 0)  # a real call: the refusal is what keeps it from the GPU
        rc, msg, launches, _ = _call(*args, **kwargs)
        assert rc == status and needle in msg and launches == 0, (rc, msg, launches)

    refused(INV, b"fields is null", None)
    refused(INV, b"field 0 is null", ctypes.byref(_field(ptr=0)))
    refused(INV, b"nfields = 0", f, nfields=0)
    refused(INV, b"domain is null", f, domain=None)
    refused(UNS, b"item size 2", f, elem_size=2)
    refused(UNS, b"item size 16", f, elem_size=16)
    refused(INV, b"empty domain", f, domain=(4, 0, 2))
    refused(INV, b"invalid domain size -1", f, domain=(4, 4, -1))
    refused(INV, b"unknown bits in flags", f, flags=6)
    refused(OOB, b"origin 1 + domain 6 along axis 0 is outside the array", f, domain=(6, 4, 2))
    refused(OOB, b"along axis 2 is outside the array", f, domain=(4, 4, 3))
    refused(OOB, b"negative origin", ctypes.byref(_field(origin=(1, -1, 0))))
    refused(UNS, b"field 0 is not aligned to its item size", ctypes.byref(_field(ptr=0x10004)))
    refused(UNS, b"byte stride 52 along axis 1 is not a multiple of the item size", ctypes.byref(_field(strides=(8, 52, 312))))
    refused(INV, b"field 0 has stride 0 along axis 0", ctypes.byref(_field(strides=(0, 8, 48))))
    # the second field: the same checks, except that a stride of 0 is a broadcast axis without a shape
    other = ctypes.byref(_field(ptr=0x20000))
    refused(UNS, b"other 0 is not aligned", f, ctypes.byref(_field(ptr=0x20002)))
    refused(OOB, b"other 0: origin 1 + domain 4 along axis 1", f, ctypes.byref(_field(ptr=0x20000, shape=(6, 4, 2))))
    weight = ctypes.byref(_field(ptr=0x20000, shape=(6, 6, 1), strides=(8, 48, 0)))  # IJ against IJK
    rc, msg, launches, needed = _call(f, weight)
    assert rc == 0 and launches == 2 and needed == NEEDED, msg
    rc, msg, launches, _ = _call(f, other)
    assert rc == 0 and launches == 2, msg
    # workspace and result
    refused(INV, b"workspace is null", f, workspace=None)
    refused(INV, b"result is null", f, result=None)
    refused(INV, b"workspace of 127 bytes is too small, 128 are needed", f, workspace_bytes=NEEDED - 1)
    refused(INV, b"workspace is not aligned to 8 bytes", f, workspace=WORK + 4)
    refused(INV, b"result is not aligned to 8 bytes", f, result=RESULT + 4)
    # the domain of FIELD starts 8 + 48 = 56 bytes in; its last point is 4 * 8 + 4 * 48 + 288 = 512 bytes in and ends at 520
    refused(INV, b"result overlaps field 0", f, result=FIELD[0] + 56)
    refused(INV, b"result overlaps field 0", f, result=FIELD[0] + 512)
    refused(INV, b"workspace overlaps field 0", f, workspace=FIELD[0] - NEEDED + 64)
    refused(INV, b"workspace overlaps other 0", f, other, workspace=0x20000 + 512)
    refused(INV, b"workspace overlaps result", f, result=WORK + 8)
    assert _call(f, result=FIELD[0] + 520)[0] == 0 and _call(f, result=FIELD[0] - 64)[0] == 0  # next to the domain: fine
    # too small buffers are refused by the dry run as well when they are passed
    rc, msg, launches, _ = _call(f, workspace_bytes=8)
    assert rc == INV and b"too small" in msg and launches == 0


def test_dry_run_reports_workspace_and_launches():
    many = E.table(_field(ptr=0x10000 * (n + 1)) for n in range(17))
    for n, want in ((1, 2), (8, 2), (9, 3), (16, 3), (17, 4)):
        rc, msg, launches, needed = _call(many, nfields=n, workspace=None, result=None)  # asking for the size
        assert rc == 0 and launches == want and needed == n * NEEDED, (n, msg)
    # the workspace follows the tile partition of the restatement, a function of the domain alone, at most 4096 tiles
    for domain in ((512, 512, 128), (1024, 1024, 80), (17, 33, 5), (3, 70000, 3)) + tuple(SEVERAL_ROWS_PER_WAVE):
        big = ctypes.byref(_field(shape=domain, strides=(8, 8 * domain[0], 8 * domain[0] * domain[1]), origin=(0, 0, 0)))
        rc, msg, launches, needed = _call(big, domain=domain, workspace=None, result=None)
        tiles = R.geometry(domain)[2]
        assert rc == 0 and launches == 2 and needed == tiles * 64 and 0 < tiles <= 4096, (domain, msg)
    rc, msg, launches, _ = _call(ctypes.byref(_field(shape=(2**20, 2**20, 2), strides=(8, 2**23, 2**43), origin=(0, 0, 0))),
                                 domain=(2**20, 2**20, 2), workspace=None, result=None)
    assert rc == _lib.ERR_UNSUPPORTED and b"2^40" in msg and launches == 0


def test_the_kernels_are_in_the_resource_log_and_use_no_scratch():
    kernels = E.kernel_resources(r"field_stats")
    assert len(kernels) == 3, kernels  # float, double, finish
    assert all(int(scratch) == 0 for _, scratch, _, _ in kernels), kernels
    lds = {("finish" if "finish" in name else "main"): int(size) for name, _, _, size in kernels}
    assert lds == {"main": 4 * 8 * 8, "finish": 128 * 8 * 8}  # the per-workgroup combines only


# ---- the restatement against exact arithmetic -------------------------------------------------------------------------------
DOMAINS = [(1, 1, 1), (3, 5, 2), (17, 33, 5), (64, 64, 8), (65, 63, 7), (130, 40, 3), (300, 37, 2), (700, 5, 3), (8, 300, 70)]
DOMAINS += list(SEVERAL_ROWS_PER_WAVE)


def test_geometry_of_the_domains_with_several_rows_per_wave():
    """What tests/test_gpu_diagnostics.py compares bit for bit beyond one row per wave; the C entry's workspace (64 bytes per tile)
    pins the same partition on the library's side (test_dry_run_reports_workspace_and_launches)."""
    for domain, want in SEVERAL_ROWS_PER_WAVE.items():
        rows, rw, tiles, chunks, per_leaf, leaves = R.geometry(domain)
        assert (rows, rw, tiles, per_leaf, leaves) == want and chunks == 1, (domain, R.geometry(domain))
        assert rw > 1 and per_leaf > 16 and rows % (R.WAVES * rw) != 0  # a last tile whose last waves have fewer rows, or none
        level, odd = leaves, []
        while level > 1:
            odd.append(level % 2 == 1)
            level = (level + 1) // 2
        assert any(odd), (domain, leaves)  # an odd number of leaves somewhere on the way up: one is carried unchanged


def _exact_int(a, b=None):
    a = a.astype(np.int64)
    x = a if b is None else a - np.broadcast_to(b.astype(np.int64), a.shape)
    dot = 0 if b is None else int((a * np.broadcast_to(b.astype(np.int64), a.shape)).sum())
    return [x.size, 0, int(x.sum()), int(np.abs(x).sum()), int((x * x).sum()), int(x.min()), int(x.max()), dot]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_is_exact_on_integer_data(dtype):
    """|x| <= 1000 (2000 for a difference): every partial sum in ANY order is an integer below 2^53, so any correct order gives
    numpy's int64 result exactly."""
    rng = np.random.default_rng(5)
    for domain in DOMAINS:
        a = rng.integers(-1000, 1000, domain, endpoint=True).astype(dtype)
        b = rng.integers(-1000, 1000, domain, endpoint=True).astype(dtype)
        w = rng.integers(0, 1000, domain[:2] + (1,), endpoint=True).astype(dtype)
        for other in (None, b, w):
            got = R.stats(a, other)
            assert got.tolist() == [float(v) for v in _exact_int(a, other)], (domain, dtype)
    assert R.geometry((8, 300, 70))[1:3] == (2, 2625)  # (more than one row per wave, more than one tile per finish leaf)
    assert R.stats(rng.integers(-9, 9, (6, 7)).astype(dtype)).tolist()[0] == 42.0  # an IJ field


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_restatement_agrees_with_fsum_within_the_derived_bound(dtype):
    """`depth` additions plus at most two more roundings (the difference, the float64 product) per term: the error of any
    summation order of that depth is at most gamma <= (depth + 3) u times the sum of the |terms| while depth^2 u << 1."""
    rng = np.random.default_rng(6)
    for domain in DOMAINS:
        a = (rng.standard_normal(domain) * 10.0 ** rng.integers(-3, 4, domain)).astype(dtype)
        b = rng.uniform(-2, 2, domain).astype(dtype)
        depth = R.depth(domain)
        assert depth ** 2 < 2 ** 53
        for other in (None, b):
            got = R.stats(a, other)
            for slot, term in zip((R.SUM, R.SUM_ABS, R.SUM_SQ, R.DOT), R.terms(a, other)):
                if term is None:
                    assert got[slot] == 0.0
                    continue
                exact, scale = math.fsum(term.ravel()), math.fsum(np.abs(term).ravel())
                assert abs(got[slot] - exact) <= (depth + 3) * U * scale, (domain, dtype, slot, got[slot], exact)
            x = R.terms(a, other)[0]
            assert (got[R.COUNT], got[R.NONFINITE], got[R.MIN], got[R.MAX]) == (x.size, 0, x.min(), x.max())


def test_depth_counts_the_longest_chain():
    assert R.depth((1, 1, 1)) == 4 + 6 + 3  # one chunk of one row: 4 items of a lane, the butterfly, the waves
    assert R.depth((512, 512, 128)) == 4 * 2 * 4 + 6 + 3 + 31 + 7  # 4 rows per wave, 2 chunks, 4096 tiles = 128 leaves of 32
    assert R.depth((1024, 1024, 80)) == 5 * 4 * 4 + 6 + 3 + 31 + 7


def test_restatement_special_values():
    z = np.zeros((5, 3, 2))
    z[1::2] = -0.0
    got = R.stats(z)
    assert np.signbit(got[R.MIN]) and not np.signbit(got[R.MAX]) and got[R.MIN] == 0 == got[R.MAX]
    assert not np.signbit(R.stats(np.zeros((2, 2, 2)))[R.MIN]) and np.signbit(R.stats(-np.zeros((2, 2, 2)))[R.MAX])
    a = np.ones((5, 3, 2))
    a[4, 2, 1] = np.nan
    got = R.stats(a)
    assert got[R.NONFINITE] == 1 and all(np.isnan(got[s]) for s in (R.SUM, R.SUM_ABS, R.SUM_SQ, R.MIN, R.MAX)) and got[R.DOT] == 0
    a[4, 2, 1], a[0, 0, 0] = np.inf, -np.inf
    got = R.stats(a)
    assert got[R.NONFINITE] == 2 and np.isnan(got[R.SUM]) and got[R.SUM_ABS] == np.inf and (got[R.MIN], got[R.MAX]) == (-np.inf, np.inf)
    assert R.same_bits([np.nan, 1.0, -0.0], [-np.nan, 1.0, -0.0]) and not R.same_bits([0.0], [-0.0]) and not R.same_bits([1.0], [np.nan])


# ---- merge -----------------------------------------------------------------------------------------------------------------
def test_merge_joins_in_the_order_given():
    S = diagnostics.Stats
    parts = [S(10, 0, 1.0, 1.0, 1.0, -2.0, 3.0, 0.5), S(5, 1, 1e16, 1e16, 2.0, -0.0, 0.0, 0.25), S(7, 2, -1e16, 1e16, 4.0, 0.0, -0.0, 0.125)]
    m = diagnostics.merge(parts)
    assert (m.count, m.nonfinite, m.min, m.max) == (22, 3, -2.0, 3.0)
    assert m.sum == (1.0 + 1e16) + -1e16 == 0.0 and diagnostics.merge(parts[::-1]).sum == (-1e16 + 1e16) + 1.0 == 1.0  # left to right
    assert m.sum_abs == 2e16 and m.sum_sq == 7.0 and m.dot == 0.875
    # signed zeros and NaN: the same rules as the kernels', whatever the order
    for order in (parts[1:], parts[:0:-1]):
        z = diagnostics.merge(order)
        assert z.min == 0 and math.copysign(1, z.min) == -1 and z.max == 0 and math.copysign(1, z.max) == 1
    nan = S(1, 1, math.nan, math.nan, math.nan, math.nan, math.nan, 0.0)
    for order in ([nan] + parts, parts + [nan]):
        n = diagnostics.merge(order)
        assert math.isnan(n.min) and math.isnan(n.max) and math.isnan(n.sum) and n.count == 23 and n.nonfinite == 4
    assert diagnostics.merge(parts[:1]) == parts[0]
    with pytest.raises(ValueError, match="at least one"):
        diagnostics.merge([])
    with pytest.raises(TypeError, match="Stats records"):
        diagnostics.merge([parts[0], (1, 2)])


def test_derived_values_of_a_record():
    s = diagnostics.Stats(4, 0, 2.0, 6.0, 16.0, -3.0, 2.5, 0.0)
    assert (s.mean, s.norm2, s.max_abs, s.all_finite) == (0.5, 4.0, 3.0, True)
    bad = diagnostics.Stats(4, 1, math.nan, math.nan, math.nan, math.nan, math.nan, 0.0)
    assert math.isnan(bad.max_abs) and not bad.all_finite
    row = np.array([4, 1, 2.0, 6.0, 16.0, -3.0, 2.5, 9.0])
    assert diagnostics.Stats.from_row(row) == diagnostics.Stats(4, 1, 2.0, 6.0, 16.0, -3.0, 2.5, 9.0)


# ---- the Python interface: every refusal before any GPU work ---------------------------------------------------------------
def test_python_refusals_need_no_gpu():
    import torch

    D = diagnostics
    with pytest.raises(ValueError, match="at least one field"):
        D.field_stats()
    with pytest.raises(TypeError, match="host"):
        D.field_stats(torch.zeros(4, 4, 2))  # as_device_array's own refusal
    with pytest.raises(TypeError):
        D.field_stats(np.zeros((4, 4, 2)))
    with pytest.raises(TypeError, match="float32 or float64 fields, not int32"):
        D.field_stats(E.host_field(HOST, dtype="int32"))
    with pytest.raises(TypeError, match="float32 or float64 fields, not bool"):
        D.FieldStats([E.host_field(HOST, dtype="bool")])
    with pytest.raises(TypeError, match="share a dtype"):
        D.field_stats(E.host_field(HOST), E.host_field(HOST, dtype="float32"))
    with pytest.raises(TypeError, match="share a dtype"):
        D.field_stats(E.host_field(HOST), other=E.host_field(HOST, dtype="float32"))
    with pytest.raises(ValueError, match="one entry .* per field: 1 for 2 fields"):
        D.FieldStats([E.host_field(HOST), E.host_field(HOST)], others=[E.host_field(HOST)])
    with pytest.raises(ValueError, match="IJ or IJK fields"):
        D.field_stats(E.host_field((8,)))
    with pytest.raises(ValueError, match="leave no domain"):
        D.field_stats(E.host_field(HOST), halo=4)
    with pytest.raises(TypeError, match="halo widths must be ints"):
        D.field_stats(E.host_field(HOST), halo=((1, 1.5), (1, 1)))
    with pytest.raises(ValueError, match="field 0: origin 2 \\+ domain 7 along axis 0 is outside the array"):
        D.field_stats(E.host_field(HOST), origin=(2, 0, 0), domain=(7, 9, 3))
    with pytest.raises(ValueError, match="field 1: origin 1 \\+ domain 6 along axis 0"):  # the second field is smaller
        D.field_stats(E.host_field(HOST), E.host_field((6, 9, 3)), halo=1)
    with pytest.raises(ValueError, match="other 0: origin 1 \\+ domain 7 along axis 1"):
        D.field_stats(E.host_field(HOST), other=E.host_field((8, 7, 3)), halo=1)
    with pytest.raises(ValueError, match="empty domain"):
        D.field_stats(E.host_field(HOST), domain=(0, 3, 3))
    # all checks passed (an IJ weight against an IJK field among them): refused for being host memory
    for kwargs in (dict(), dict(halo=2), dict(other=E.host_field(HOST)), dict(other=E.host_field((8, 9))), dict(origin=(1, 1), domain=(2, 2, 3))):
        with pytest.raises(TypeError, match="device fields"):
            D.field_stats(E.host_field(HOST), **kwargs)
    with pytest.raises(TypeError, match="device fields"):
        D.FieldStats([E.host_field((8, 9), "float32")], halo=((1, 2), (0, 3)))  # Field[IJ]
