"""``gt4py_amd.horizontal.remap_cells`` without a GPU: ``gt4mi_overlap_table`` (host code) bit for bit against the restatement
tests/horizontal_remap_ref.py, the table's invariants, every refusal of the two C entries (``gt4mi_horizontal_remap`` through its
dry run, with made-up addresses that are never dereferenced), the declarations, the kernels' resources, the Python interface's
argument checks and the properties of the restated arithmetic (conservation, linear fields)."""

import ctypes
import math
import re

import numpy as np
import pytest

import entry_checks as E
import horizontal_remap_ref as R
from entry_checks import INV, OOB, UNS, as_arg
from gt4py_amd import _lib, horizontal

EPS = 2.0 ** -52
METHODS = [R.PCM, R.PLM]
SIZES = [(1, 1), (1, 5), (5, 1), (2, 3), (17, 9), (9, 17), (130, 1)]


# ---- edge sets --------------------------------------------------------------------------------------------------------------------
def _increasing(rng, n, lo=None, hi=None):
    """n + 1 strictly increasing edges; with lo / hi the outer ones are exactly those."""
    x = rng.uniform(-3, 3) + np.concatenate([[0.0], np.cumsum(rng.uniform(0.05, 1.0, n))])
    if lo is not None:
        x = lo + (x - x[0]) * ((hi - lo) / (x[-1] - x[0]))
        x[0], x[-1] = lo, hi
    assert (np.diff(x) > 0).all()
    return x


def _edge_sets(ns, nd, seed=0):
    """(name, xs, xd) for every kind of pair the issue lists that exists at (ns, nd)."""
    rng = np.random.default_rng([seed, ns, nd])
    xs = _increasing(rng, ns)
    yield "random", xs, _increasing(rng, nd, xs[0] - rng.uniform(0, 0.5), xs[-1] + rng.uniform(0, 0.5))
    yield "shared outer edges", xs, _increasing(rng, nd, xs[0], xs[-1])
    xs32 = _increasing(rng, ns).astype(np.float32).astype(np.float64)
    xd32 = _increasing(rng, nd, xs32[0] - 0.25, xs32[-1] + 0.25).astype(np.float32).astype(np.float64)
    if (np.diff(xs32) > 0).all() and (np.diff(xd32) > 0).all():
        yield "float32 values", xs32, xd32
    if nd <= ns:  # every destination edge IS a source edge: the > / >= ties
        yield "coinciding", xs, xs[np.sort(rng.choice(ns + 1, nd + 1, replace=False))]
    else:  # ... and past the last one
        yield "coinciding", xs, np.concatenate([xs, xs[-1] + np.cumsum(rng.uniform(0.1, 1, nd - ns))])
    if nd == ns:
        yield "identical", xs, xs.copy()
    if nd >= 5:  # two cells below and two above the source range
        yield "outside", xs, np.concatenate([[xs[0] - 3, xs[0] - 2], _increasing(rng, nd - 4, xs[0] - 0.5, xs[-1] + 0.5), [xs[-1] + 2, xs[-1] + 3]])
    if nd == 1:
        yield "one cell spans everything", xs, np.array([xs[0] - 1.0, xs[-1] + 1.0])
        yield "one cell spans exactly", xs, np.array([xs[0], xs[-1]])


def _c_table(xs, xd, capacity=None, plm=True):
    """gt4mi_overlap_table through ctypes into buffers with a guard item behind each: (rc, message, nnz, arrays)."""
    lib = _lib.load()
    xs, xd = np.ascontiguousarray(xs, dtype=np.float64), np.ascontiguousarray(xd, dtype=np.float64)
    ns, nd = xs.size - 1, xd.size - 1
    capacity = ns + nd - 1 if capacity is None else capacity
    ptr, cell = np.full(nd + 2, -7, dtype=np.int32), np.full(capacity + 1, -7, dtype=np.int32)
    reals = [np.full(capacity + 1, -7.0) for _ in range(4)]
    nnz = ctypes.c_int(-1)
    extra = [a.ctypes.data if plm else None for a in reals[1:]]
    rc = lib.gt4mi_overlap_table(xs.ctypes.data, ns, xd.ctypes.data, nd, ptr.ctypes.data, cell.ctypes.data, reals[0].ctypes.data, *extra,
                                 capacity, ctypes.byref(nnz))
    assert ptr[-1] == -7 and cell[-1] == -7 and all(a[-1] == -7.0 for a in reals), "wrote past the capacity"
    return rc, lib.gt4mi_last_error(), nnz.value, (ptr[:-1], cell[:-1]) + tuple(a[:-1] for a in reals)


def _hex(values):
    return [float(v).hex() for v in values]


# ---- the table against the restatement, and its invariants --------------------------------------------------------------------
@pytest.mark.parametrize("ns, nd", SIZES + [(5, 5), (17, 17)])
def test_the_overlap_table_equals_the_restatement_bit_for_bit(ns, nd):
    kinds = set()
    for seed in range(3):
        for kind, xs, xd in _edge_sets(ns, nd, seed):
            kinds.add(kind)
            want = R.axis_table([float(v) for v in xs], [float(v) for v in xd])
            rc, msg, nnz, got = _c_table(xs, xd)
            assert rc == 0, msg
            assert nnz == len(want[1]) and got[0].tolist() == want[0], (kind, ns, nd)
            assert got[1][:nnz].tolist() == want[1], (kind, ns, nd)
            for name, g, w in zip("whcd", got[2:], want[2:]):
                assert _hex(g[:nnz]) == _hex(w), (kind, ns, nd, name)
            # the invariants: nd <= nnz <= ns + nd - 1, ptr increasing from 0 to nnz, cells never decrease, weights sum to 1
            ptr, cell, w = got[0], got[1][:nnz], got[2][:nnz]
            assert nd <= nnz <= ns + nd - 1 and ptr[0] == 0 and ptr[nd] == nnz and (np.diff(ptr) >= 1).all()
            assert (np.diff(cell) >= 0).all() and cell.min() >= 0 and cell.max() <= ns - 1
            for m in range(nd):
                terms = ptr[m + 1] - ptr[m]
                assert abs(math.fsum(w[ptr[m]:ptr[m + 1]]) - 1.0) <= terms * EPS, (kind, ns, nd, m)  # one rounding per weight
            if kind == "identical":
                assert nnz == ns and cell.tolist() == list(range(ns)) and _hex(w) == _hex([1.0] * ns)
            if kind == "outside":  # whole cells below / above the source range: one term, the end cell, weight exactly 1
                assert cell[ptr[0]:ptr[2]].tolist() == [0, 0] and cell[ptr[nd - 2]:].tolist() == [ns - 1, ns - 1]
                assert _hex(w[ptr[0]:ptr[2]]) == _hex(w[ptr[nd - 2]:]) == _hex([1.0, 1.0])
            if kind.startswith("one cell spans"):
                assert nnz == ns and cell.tolist() == list(range(ns))
            # a pcm-only table (h, c, den NULL) holds the same ptr, cell, w
            rc, msg, nnz2, pcm = _c_table(xs, xd, plm=False)
            assert rc == 0 and nnz2 == nnz and all(np.array_equal(a, b) for a, b in zip(pcm[:3], got[:3])), msg
            assert all((a == -7.0).all() for a in pcm[3:])
    assert {"random", "shared outer edges", "float32 values", "coinciding"} <= kinds


def test_the_term_bound_is_reached_and_a_smaller_capacity_is_enough_where_the_table_is_smaller():
    xs, xd = np.arange(6.0), np.arange(4.0) * 5 / 3  # no inner edge coincides: ns + nd - 1 terms
    rc, msg, nnz, _ = _c_table(xs, xd)
    assert rc == 0 and nnz == 5 + 3 - 1, msg
    rc, msg, nnz, _ = _c_table(xs, xd, capacity=6)
    assert rc == OOB and b"capacity 6 is too small" in msg
    rc, msg, nnz, _ = _c_table(xs, xs, capacity=5)  # identical grids: ns terms
    assert rc == 0 and nnz == 5, msg
    rc, msg, _, _ = _c_table(xs, xs, capacity=4)
    assert rc == OOB and b"too small" in msg


def test_every_refusal_of_the_table_entry():
    lib = _lib.load()
    xs, xd = np.arange(4.0), np.array([0.0, 1.5, 3.0])
    good = dict(xs=xs, ns=3, xd=xd, nd=2, ptr=np.zeros(3, np.int32), cell=np.zeros(4, np.int32), w=np.zeros(4), h=np.zeros(4), c=np.zeros(4),
                den=np.zeros(4), capacity=4)
    nnz = ctypes.c_int(0)

    def call(nnz_arg=True, **over):
        a = dict(good, **over)
        p = lambda v: None if v is None else v.ctypes.data  # noqa: E731
        rc = lib.gt4mi_overlap_table(p(a["xs"]), a["ns"], p(a["xd"]), a["nd"], p(a["ptr"]), p(a["cell"]), p(a["w"]), p(a["h"]), p(a["c"]),
                                     p(a["den"]), a["capacity"], ctypes.byref(nnz) if nnz_arg else None)
        return rc, lib.gt4mi_last_error()

    assert call()[0] == 0 and nnz.value == 4
    for name, word in (("xs", b"src_edges is null"), ("xd", b"dst_edges is null"), ("ptr", b"ptr is null"), ("cell", b"cell is null"),
                       ("w", b"w is null"), ("h", b"h is null"), ("c", b"c is null"), ("den", b"den is null")):
        rc, msg = call(**{name: None})
        assert rc == INV and word in msg, msg
    rc, msg = call(nnz_arg=False)
    assert rc == INV and b"nnz is null" in msg
    assert call(h=None, c=None, den=None)[0] == 0  # all three: a pcm table
    for over, word in ((dict(ns=0), b"ns = 0"), (dict(nd=0), b"nd = 0"), (dict(nd=-3), b"nd = -3")):
        rc, msg = call(**over)
        assert rc == INV and word in msg, msg
    for bad, word in (([0.0, 1.0, 1.0, 3.0], b"src_edges are not strictly increasing at [2]"), ([0.0, 2.0, 1.0, 3.0], b"not strictly increasing"),
                      ([0.0, np.nan, 2.0, 3.0], b"src_edges[1] is not finite"), ([0.0, 1.0, 2.0, np.inf], b"src_edges[3] is not finite"),
                      ([-np.inf, 1.0, 2.0, 3.0], b"src_edges[0] is not finite")):
        rc, msg = call(xs=np.array(bad))
        assert rc == INV and word in msg, msg
    rc, msg = call(xd=np.array([0.0, 0.0, 3.0]))
    assert rc == INV and b"dst_edges are not strictly increasing at [1]" in msg
    rc, msg = call(xd=np.array([0.0, 1.0, np.nan]))
    assert rc == INV and b"dst_edges[2] is not finite" in msg
    rc, msg = call(capacity=3)
    assert rc == OOB and b"capacity 3 is too small" in msg and nnz.value == 0
    rc, msg = call(capacity=0)
    assert rc == OOB and b"too small" in msg


# ---- the declarations ------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_header_signatures_and_the_abi_is_still_8():
    P, I = ctypes.c_void_p, ctypes.c_int
    E.check_binding("gt4mi_overlap_table",
                    ["const double* src_edges", "int ns", "const double* dst_edges", "int nd", "int32_t* ptr", "int32_t* cell",
                     "double* w", "double* h", "double* c", "double* den", "int capacity", "int* nnz"],
                    argtypes=[P, I, P, I, P, P, P, P, P, P, I, ctypes.POINTER(I)])
    E.check_binding("gt4mi_horizontal_remap",
                    ["const gt4mi_field* dst", "const gt4mi_field* src", "int nfields", "const gt4mi_overlap_axis* axis_i",
                     "const gt4mi_overlap_axis* axis_j", "int64_t nk", "int elem_size", "int method", "int flags",
                     "void* stream", "int* launches"],
                    prefix="HREMAP", constants=("PCM", "PLM", "DRY_RUN"),
                    phrases=("conservative horizontal remapping", "no reference", "(r - l) / d", "xs[k+1] >= hi", "0.5 * (xl + xr) - 0.5",
                             "edge replication", "row_b = sum_a wi_a * q[a, b]", "(q[a, b] + si * ci_a) + sj * cj_b",
                             "not strictly monotone in 2-d", "clamps each ptr value to [0, nnz]"))
    text = (E.ROOT / "include" / "gt4py_amd.h").read_text()
    struct = re.search(r"typedef struct gt4mi_overlap_axis \{(.*?)\} gt4mi_overlap_axis;", text, re.S).group(1)
    members = [" ".join(m.split()) for m in re.sub(r"/\*.*?\*/", "", struct, flags=re.S).split(";") if m.strip()]
    assert members == ["int32_t ns, nd, nnz", "const int32_t* ptr", "const int32_t* cell", "const double* w", "const double* h", "const double* c",
                       "const double* den"]
    assert [n for n, _ in _lib.OverlapAxis._fields_] == ["ns", "nd", "nnz", "ptr", "cell", "w", "h", "c", "den"]
    assert ctypes.sizeof(_lib.OverlapAxis) == 64 and _lib.OverlapAxis.ptr.offset == 16
    assert horizontal.REMAP_METHODS == {"pcm": _lib.HREMAP_PCM, "plm": _lib.HREMAP_PLM}


# ---- the refusals of gt4mi_horizontal_remap, through the dry run ------------------------------------------------------------------
DST, SRC, TAB = 0x10_0000, 0x4000_0000, 0x8000_0000  # made-up device addresses, far apart
NS_I, NS_J, ND_I, ND_J, NK = 6, 5, 4, 3, 3


def _field(ptr, shape_ij, nk=NK, strides=None, origin=(1, 1, 0), itemsize=8):  # (the plane, then this file's nk)
    return E.field(ptr, (*shape_ij, nk), strides, origin, itemsize)


def _axis(base, ns, nd, nnz=None, **over):
    """A table of made-up addresses 0x1000 apart from ``base``."""
    nnz = ns + nd - 1 if nnz is None else nnz
    a = dict(ptr=base, cell=base + 0x1000, w=base + 0x2000, h=base + 0x3000, c=base + 0x4000, den=base + 0x5000)
    a.update(over)
    return _lib.OverlapAxis(ns, nd, nnz, a["ptr"], a["cell"], a["w"], a["h"], a["c"], a["den"])


def _call(dst, src, axis_i, axis_j, nfields=1, nk=NK, size=8, method=0, flags=0):
    return E.call("gt4mi_horizontal_remap", as_arg(dst), as_arg(src), nfields, as_arg(axis_i), as_arg(axis_j), nk, size, method,
                  flags | _lib.HREMAP_DRY_RUN, None, outs=(77,))


def test_every_refusal_of_the_c_entry_without_a_gpu():
    """Every check runs before the first launch: these calls carry made-up device addresses and the dry-run flag."""
    d, s = _field(DST, (ND_I + 2, ND_J + 2)), _field(SRC, (NS_I + 2, NS_J + 2))
    ai, aj = _axis(TAB, NS_I, ND_I), _axis(TAB + 0x10000, NS_J, ND_J)
    for method in (_lib.HREMAP_PCM, _lib.HREMAP_PLM):
        rc, msg, launches = _call(d, s, ai, aj, method=method)
        assert rc == 0 and launches == 1, msg
        rc, msg, launches = _call(_field(DST, (ND_I + 2, ND_J + 2), itemsize=4), _field(SRC, (NS_I + 2, NS_J + 2), itemsize=4), ai, aj, size=4, method=method)
        assert rc == 0 and launches == 1, msg
    # null pointers: the arguments, a field's data, a table array (h, c, den only where the method reads them)
    for n, what in enumerate((b"dst is null", b"src is null", b"axis_i is null", b"axis_j is null")):
        args = [d, s, ai, aj]
        args[n] = None
        rc, msg, launches = _call(*args)
        assert rc == INV and what in msg and launches == 0, msg
    rc, msg, _ = _call(_field(0, (ND_I + 2, ND_J + 2)), s, ai, aj)
    assert rc == INV and b"dst 0 is null" in msg
    rc, msg, _ = _call(d, _field(0, (NS_I + 2, NS_J + 2)), ai, aj)
    assert rc == INV and b"src 0 is null" in msg
    for name in ("ptr", "cell", "w"):
        rc, msg, _ = _call(d, s, _axis(TAB, NS_I, ND_I, **{name: None}), aj)
        assert rc == INV and f"axis_i {name} is null".encode() in msg, msg
    for name in ("h", "c", "den"):
        rc, msg, _ = _call(d, s, ai, _axis(TAB + 0x10000, NS_J, ND_J, **{name: None}), method=_lib.HREMAP_PLM)
        assert rc == INV and f"axis_j {name} is null".encode() in msg, msg
    rc, msg, _ = _call(d, s, _axis(TAB, NS_I, ND_I, h=None, c=None, den=None), aj, method=_lib.HREMAP_PCM)
    assert rc == 0, msg
    # counts, flags, method
    for n in (0, -2):
        rc, msg, launches = _call(d, s, ai, aj, nfields=n)
        assert rc == INV and b"nfields" in msg and launches == 0
    for nk in (0, -1):
        rc, msg, _ = _call(d, s, ai, aj, nk=nk)
        assert rc == INV and b"nk = " in msg
    rc, msg, _ = _call(d, s, _axis(TAB, 0, ND_I, nnz=ND_I), aj)
    assert rc == INV and b"axis_i has ns = 0" in msg
    rc, msg, _ = _call(d, s, ai, _axis(TAB + 0x10000, NS_J, -1, nnz=3))
    assert rc == INV and b"axis_j has ns = 5 source and nd = -1" in msg
    for flags in (1, 2, 512):
        rc, msg, _ = _call(d, s, ai, aj, flags=flags)
        assert rc == INV and b"flags" in msg
    for method in (2, -1):
        rc, msg, launches = _call(d, s, ai, aj, method=method)
        assert rc == INV and b"unknown method" in msg and launches == 0
    # nnz outside [nd, ns + nd - 1]
    for nnz in (ND_I - 1, NS_I + ND_I, -1):
        rc, msg, _ = _call(d, s, _axis(TAB, NS_I, ND_I, nnz=nnz), aj)
        assert rc == INV and b"axis_i has nnz = " in msg, msg
    for nnz in (ND_I, NS_I + ND_I - 1):
        rc, msg, _ = _call(d, s, _axis(TAB, NS_I, ND_I, nnz=nnz), aj)
        assert rc == 0, msg
    # item sizes other than 4 or 8; misaligned fields and table arrays; strides
    rc, msg, _ = _call(d, s, ai, aj, size=2)
    assert rc == UNS and b"field item size 2" in msg
    rc, msg, _ = _call(_field(DST + 4, (ND_I + 2, ND_J + 2)), s, ai, aj)
    assert rc == UNS and b"dst 0 is not aligned to its item size" in msg
    rc, msg, _ = _call(d, s, _axis(TAB, NS_I, ND_I, cell=TAB + 0x1002), aj)
    assert rc == UNS and b"axis_i cell is not aligned" in msg
    rc, msg, _ = _call(d, s, ai, _axis(TAB + 0x10000, NS_J, ND_J, w=TAB + 0x12004))
    assert rc == UNS and b"axis_j w is not aligned" in msg
    rc, msg, _ = _call(d, s, ai, _axis(TAB + 0x10000, NS_J, ND_J, den=TAB + 0x15004))  # (not read by pcm)
    assert rc == 0, msg
    rc, msg, _ = _call(d, s, ai, _axis(TAB + 0x10000, NS_J, ND_J, den=TAB + 0x15004), method=_lib.HREMAP_PLM)
    assert rc == UNS and b"axis_j den is not aligned" in msg
    rc, msg, _ = _call(_field(DST, (ND_I + 2, ND_J + 2), strides=(8, 52, 312)), s, ai, aj)
    assert rc == UNS and b"multiple of the item size" in msg
    # a box that does not fit its field: the dst box is (nd_i, nd_j, nk), the src box (ns_i, ns_j, nk), each from its origin
    rc, msg, launches = _call(_field(DST, (ND_I, ND_J + 2)), s, ai, aj)
    assert rc == OOB and b"dst 0" in msg and b"extent 4 along axis 0" in msg and launches == 0
    rc, msg, _ = _call(d, _field(SRC, (NS_I + 2, NS_J)), ai, aj)
    assert rc == OOB and b"src 0" in msg and b"extent 5 along axis 1" in msg
    rc, msg, _ = _call(d, s, ai, aj, nk=NK + 1)
    assert rc == OOB and b"dst 0" in msg and b"axis 2" in msg
    rc, msg, _ = _call(_field(DST, (ND_I + 2, ND_J + 2), nk=NK + 1), s, ai, aj, nk=NK + 1)
    assert rc == OOB and b"src 0" in msg and b"axis 2" in msg
    rc, msg, _ = _call(d, _field(SRC, (NS_I + 2, NS_J + 2), origin=(1, -1, 0)), ai, aj)
    assert rc == OOB and b"negative origin -1 along axis 1" in msg
    # stride 0: refused for a dst on an extent above 1, fine on an extent of 1; a src broadcasts
    rc, msg, launches = _call(_field(DST, (ND_I + 2, ND_J + 2), strides=(0, 8, 48)), s, ai, aj)
    assert rc == INV and b"dst 0 has stride 0 along axis 0" in msg and b"only a src may be broadcast" in msg and launches == 0
    rc, msg, _ = _call(_field(DST, (ND_I + 2, ND_J + 2), strides=(8, 48, 0)), s, ai, aj)
    assert rc == INV and b"dst 0 has stride 0 along axis 2" in msg
    rc, msg, _ = _call(_field(DST, (ND_I + 2, ND_J + 2), nk=1, strides=(8, 48, 0)), _field(SRC, (NS_I + 2, NS_J + 2), nk=1), ai, aj, nk=1)
    assert rc == 0, msg
    rc, msg, _ = _call(d, _field(SRC, (NS_I + 2, NS_J + 2), strides=(0, 8, 0)), ai, aj)
    assert rc == 0, msg
    # overlap in memory: a dst box against its src box, another pair's src, another dst, any table array; a byte apart is fine
    rc, msg, launches = _call(d, _field(DST, (NS_I + 2, NS_J + 2)), ai, aj)
    assert rc == UNS and b"dst 0 and src 0 overlap in memory" in msg and launches == 0
    pitch_j, pitch_k = 8 * (ND_I + 2), 8 * (ND_I + 2) * (ND_J + 2)
    first, last = 8 + pitch_j, 8 * ND_I + pitch_j * ND_J + pitch_k * (NK - 1)  # byte offsets of the dst box's first and last item
    s_first = 8 + 8 * (NS_I + 2)  # ... and of the src box's first item in its array
    rc, msg, _ = _call(d, _field(DST + last - s_first, (NS_I + 2, NS_J + 2)), ai, aj)  # src's first item IS dst's last
    assert rc == UNS and b"overlap in memory" in msg
    rc, msg, _ = _call(d, _field(DST + last - s_first + 8, (NS_I + 2, NS_J + 2)), ai, aj)  # the byte ranges of the BOXES do not meet
    assert rc == 0, msg
    two = lambda a, b: E.table((a, b))  # noqa: E731
    rc, msg, _ = _call(two(d, _field(DST + 0x1000, (ND_I + 2, ND_J + 2))), two(s, _field(DST + 64, (NS_I + 2, NS_J + 2))), ai, aj, nfields=2)
    assert rc == UNS and b"dst 0 and src 1 overlap in memory" in msg
    rc, msg, _ = _call(two(d, _field(DST + 128, (ND_I + 2, ND_J + 2))), two(s, _field(SRC + 0x1000, (NS_I + 2, NS_J + 2))), ai, aj, nfields=2)
    assert rc == UNS and b"dst 0 and dst 1 overlap in memory" in msg
    rc, msg, launches = _call(two(d, _field(DST + 0x1000, (ND_I + 2, ND_J + 2))), two(s, s), ai, aj, nfields=2)  # one src for two dsts is fine
    assert rc == 0 and launches == 1, msg
    for name in ("ptr", "cell", "w", "h", "c", "den"):
        for which in (0, 1):
            axes = [ai, aj]
            axes[which] = _axis(TAB + 0x10000 * which, (NS_I, NS_J)[which], (ND_I, ND_J)[which], **{name: DST + first + 16})
            rc, msg, _ = _call(d, s, *axes, method=_lib.HREMAP_PLM)
            assert rc == UNS and f"dst 0 and axis_{'ij'[which]} {name} overlap in memory".encode() in msg, msg
    rc, msg, _ = _call(d, s, _axis(TAB, NS_I, ND_I, w=DST + first - 8 * (NS_I + ND_I - 1)), aj)  # the array ends where the box begins
    assert rc == 0, msg
    rc, msg, _ = _call(d, s, _axis(TAB, NS_I, ND_I, w=DST + first - 8 * (NS_I + ND_I - 1) + 8), aj)
    assert rc == UNS and b"dst 0 and axis_i w overlap" in msg
    rc, msg, _ = _call(d, s, _axis(TAB, NS_I, ND_I, h=DST + first), aj)  # (pcm does not read h)
    assert rc == 0, msg


def test_launches_are_one_per_eight_pairs():
    d = E.table(_field(DST + n * 0x1000, (ND_I + 2, ND_J + 2)) for n in range(9))
    s = E.table(_field(SRC + n * 0x1000, (NS_I + 2, NS_J + 2)) for n in range(9))
    ai, aj = _axis(TAB, NS_I, ND_I), _axis(TAB + 0x10000, NS_J, ND_J)
    assert [_call(d, s, ai, aj, nfields=n)[2] for n in (1, 4, 8, 9)] == [1, 1, 1, 2]


def test_the_kernels_are_in_the_resource_log_without_scratch():
    kernels = E.kernel_resources(r"horizontal_remap_kernel")
    # 2 field types x 2 methods x the instantiations for 1, 4 and 8 entries
    assert len(kernels) == 12 and len({name for name, *_ in kernels}) == 12, kernels
    for name, scratch, waves, lds in kernels:
        assert int(scratch) == 0 and int(waves) >= 4 and int(lds) == 0, (name, scratch, waves, lds)


# ---- the Python interface: every refusal before any GPU work -------------------------------------------------------------------
XI, XJ, YI, YJ = np.linspace(0, 1, 9), np.linspace(0, 2, 7), np.linspace(0, 1, 5), np.linspace(-0.5, 2.5, 4)


def _good(**over):
    args = dict(dst=E.host_field((4, 3, 5)), src=E.host_field((8, 6, 5)), src_edges=(XI, XJ), dst_edges=(YI, YJ))
    args.update(over)
    return args.pop("dst"), args.pop("src"), args


@pytest.mark.parametrize("kwargs, error, match", [
    (dict(method="ppm"), ValueError, "method must be one of"),
    (dict(src_edges=(XI,)), ValueError, "src_edges must be a pair"),
    (dict(dst_edges=YI), ValueError, "dst_edges must be a pair"),
    (dict(src_edges=(XI, "abc")), TypeError, "src_edges along J must be a 1-d host array-like"),
    (dict(src_edges=(XI.reshape(3, 3), XJ)), ValueError, "src_edges along I must be a 1-d array"),
    (dict(dst_edges=(YI, [1.0])), ValueError, "dst_edges along J must be a 1-d array of at least 2 edges"),
    (dict(src_edges=(np.linspace(0, 1, 10), XJ)), ValueError, "src_edges along I has 10 edges: 9 cells from origin 0 do not match src 0"),
    (dict(dst_edges=(YI, np.linspace(0, 2, 5))), ValueError, "dst_edges along J has 5 edges: 4 cells from origin 0 do not match dst 0"),
    (dict(src_origin=(1, 0, 0)), ValueError, "src_edges along I has 9 edges: 8 cells from origin 1 do not match src 0"),
    (dict(dst_origin=(0, 0, 0, 0)), ValueError, "at most three entries"),
    (dict(dst_origin=(0, 0, 1)), ValueError, r"share their number of levels behind the origin: \[4, 5\] differ"),
    (dict(dst_origin=(0, 0, 5), src_origin=(0, 0, 5)), ValueError, "leave no level"),
    (dict(src_edges=(XI[::-1], XJ)), ValueError, "src_edges are not strictly increasing at .1."),
    (dict(src_edges=(XI, np.where(np.arange(7) == 3, np.nan, XJ))), ValueError, r"src_edges\[3\] is not finite"),
    (dict(dst_edges=([0.0, 0.25, 0.25, 0.75, 1.0], YJ)), ValueError, "dst_edges are not strictly increasing at .2."),
    (dict(dst_edges=(YI, [0.0, 1.0, 2.0, np.inf])), ValueError, r"dst_edges\[3\] is not finite"),
    (dict(method="plm"), TypeError, "device fields"),  # all checks passed: refused for being host memory
    (dict(), TypeError, "device fields"),
])
def test_python_refusals_need_no_gpu(kwargs, error, match):
    dst, src, rest = _good(**kwargs)
    with pytest.raises(error, match=match):
        horizontal.remap_cells(dst, src, **rest)
    with pytest.raises(error, match=match):
        horizontal.HorizontalRemap([dst], [src], **rest)


def test_python_refusals_about_the_fields_themselves():
    import torch

    F = horizontal.remap_cells
    dst, src, edges = _good()
    with pytest.raises(ValueError, match="at least one"):
        F([], [], **edges)
    with pytest.raises(ValueError, match="2 destination.s. and 1 source"):
        F([dst, E.host_field((4, 3, 5))], [src], **edges)
    with pytest.raises(TypeError, match="host"):
        F(torch.zeros(4, 3, 5, dtype=torch.float64), src, **edges)  # as_device_array's own refusal
    with pytest.raises(TypeError):
        F(dst, np.zeros((8, 6, 5)), **edges)
    with pytest.raises(ValueError, match="takes IJK fields"):
        F(E.host_field((4, 3)), src, **edges)
    with pytest.raises(TypeError, match="share a dtype: float64 and float32 differ"):
        F(dst, E.host_field((8, 6, 5), "float32"), **edges)
    with pytest.raises(TypeError, match="share a dtype"):
        F([dst, E.host_field((4, 3, 5), "float32")], [src, src], **edges)
    with pytest.raises(TypeError, match="float32 or float64 fields"):
        F(E.host_field((4, 3, 5), "int64"), E.host_field((8, 6, 5), "int64"), **edges)
    with pytest.raises(ValueError, match=r"levels behind the origin: \[4, 5\] differ"):
        F([dst, E.host_field((4, 3, 4))], [src, src], **edges)
    with pytest.raises(ValueError, match="do not match dst 1 of shape"):
        F([dst, E.host_field((3, 3, 5))], [src, src], **edges)
    with pytest.raises(TypeError, match="device fields"):
        F(E.host_field((4, 3, 5), "float32"), E.host_field((8, 6, 5), "float32"), **edges)
    with pytest.raises(TypeError, match="device fields"):  # fields larger than the boxes, with origins
        F(E.host_field((6, 5, 5)), E.host_field((9, 9, 6)), **edges, dst_origin=(2, 1, 0), src_origin=(1, 3, 1))
    # a field onto itself (identical grids): the library's refusal, as a TypeError
    x = E.host_field((8, 6, 5))
    with pytest.raises(TypeError, match="dst 0 and src 0 overlap in memory"):
        F(x, x, src_edges=(XI, XJ), dst_edges=(XI, XJ))


def test_a_frozen_remap_knows_its_boxes_and_refuses_to_run_after_an_array_died(monkeypatch):
    """The weak references are taken last, behind the device check: what they guard is shown on a HorizontalRemap whose device
    check is made to pass for host memory -- the call itself is never reached, the dead reference is found first."""
    E.on_device(monkeypatch)
    dsts, srcs = [E.host_field((5, 3, 5)) for _ in range(9)], [E.host_field((8, 7, 6)) for _ in range(9)]
    hr = horizontal.HorizontalRemap(dsts, srcs, src_edges=(XI, XJ), dst_edges=(YI, YJ), method="plm", src_origin=(0, 1, 1))
    assert (hr.src_extent, hr.dst_extent, hr.nk, hr.launches, hr.method) == ((8, 6), (4, 3), 5, 2, "plm")
    assert hr.terms == (8, 6 + 3 - 1) and (hr.src_origin, hr.dst_origin) == ((0, 1, 1), (0, 0, 0))
    # the object owns its tables: they are the host entry's, in one int32 and one float64 array per axis
    for axis, (xs, xd) in enumerate(((XI, YI), (XJ, YJ))):
        ptr, cell, w, h, c, den = horizontal.overlap_table(xs, xd)
        assert np.array_equal(hr._tables[2 * axis].numpy(), np.concatenate([ptr, cell]))
        assert np.array_equal(hr._tables[2 * axis + 1].numpy(), np.concatenate([w, h, c, den]))
    del srcs[4]
    E.refuses_a_dead_array(hr)


# ---- properties of the restated arithmetic ----------------------------------------------------------------------------------------
def _grids(count, seed):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        ns_i, ns_j, nd_i, nd_j = (int(x) for x in rng.integers(1, 9, 4))
        xs = (_increasing(rng, ns_i), _increasing(rng, ns_j))
        yield rng, xs, (nd_i, nd_j)


def _terms_per_cell(xs, xd):
    tables = [R.axis_table([float(v) for v in s], [float(v) for v in d]) for s, d in zip(xs, xd)]
    return tables, max(np.diff(tables[0][0])) * max(np.diff(tables[1][0]))


def test_conservation_when_the_outer_edges_coincide():
    """|sum out * area - sum q * area| <= 8 eps (terms per cell + 3) sum |q| area, both sums by math.fsum: three roundings per term
    (the product of the two weights' errors, the value, the product) and the three of the areas."""
    worst = 0.0
    for rng, xs, (nd_i, nd_j) in _grids(150, 21):
        xd = (_increasing(rng, nd_i, xs[0][0], xs[0][-1]), _increasing(rng, nd_j, xs[1][0], xs[1][-1]))
        _, terms = _terms_per_cell(xs, xd)
        ns_i, ns_j = xs[0].size - 1, xs[1].size - 1
        kind = int(rng.integers(0, 3))
        if kind == 0:
            q = rng.uniform(-1, 1, (ns_i, ns_j, 1))
        elif kind == 1:  # smooth and monotone along both axes: the limited slopes are not zero
            q = (np.cumsum(rng.uniform(0.1, 1, ns_i))[:, None, None] + np.cumsum(rng.uniform(0.1, 1, ns_j))[None, :, None]) * 10.0 ** int(rng.integers(-3, 4))
        else:
            q = 1.0e6 + rng.uniform(-1, 1, (ns_i, ns_j, 1))
        area_s = np.diff(xs[0])[:, None] * np.diff(xs[1])[None, :]
        area_d = np.diff(xd[0])[:, None] * np.diff(xd[1])[None, :]
        want = math.fsum((q[:, :, 0] * area_s).ravel())
        scale = math.fsum((np.abs(q[:, :, 0]) * area_s).ravel())
        bound = 8 * EPS * (terms + 3) * scale
        for method in METHODS:
            out = R.remap(q, xs, xd, method)
            have = math.fsum((out[:, :, 0] * area_d).ravel())
            worst = max(worst, abs(have - want) / bound)
            assert abs(have - want) <= bound, (method, q.shape, (nd_i, nd_j), have, want, bound)
    print(f"conservation: worst {worst:.3f} of the bound")


def test_plm_reproduces_fields_linear_in_x_and_y_where_every_source_is_interior():
    """out = a + b x + c y at the destination cell's centre, to the order of the conservation bound, in destination cells all of
    whose source cells are interior along both axes (the end cells have slope 0); pcm does not."""
    worst, checked, pcm_off = 0.0, 0, 0
    for rng, xs, (nd_i, nd_j) in _grids(150, 22):
        ns_i, ns_j = xs[0].size - 1, xs[1].size - 1
        if ns_i < 4 or ns_j < 4:
            continue
        xd = (_increasing(rng, nd_i, xs[0][1], xs[0][-2]), _increasing(rng, nd_j, xs[1][1], xs[1][-2]))  # inside the interior cells
        tables, terms = _terms_per_cell(xs, xd)
        a, b, c = (float(v) for v in rng.uniform(-2, 2, 3))
        centre = lambda x: 0.5 * (x[:-1] + x[1:])  # noqa: E731
        q = (a + b * centre(xs[0])[:, None] + c * centre(xs[1])[None, :])[:, :, None]
        want = a + b * centre(xd[0])[:, None] + c * centre(xd[1])[None, :]
        scale = abs(a) + abs(b) * np.abs(xs[0]).max() + abs(c) * np.abs(xs[1]).max()
        bound = 8 * EPS * (terms + 3) * scale
        out = R.remap(q, xs, xd, R.PLM)[:, :, 0]
        flat = R.remap(q, xs, xd, R.PCM)[:, :, 0]
        for axis, (ptr, cell, *_rest) in enumerate(tables):
            assert min(cell) >= 1 and max(cell) <= (ns_i, ns_j)[axis] - 2  # every source is interior
        worst = max(worst, np.abs(out - want).max() / bound)
        assert np.abs(out - want).max() <= bound, (q.shape, (nd_i, nd_j), np.abs(out - want).max(), bound)
        checked += out.size
        pcm_off += int((np.abs(flat - want) > bound).sum())
    assert checked > 500 and pcm_off > checked // 2
    print(f"linear fields: worst {worst:.3f} of the bound over {checked} cells")


def test_identity_returns_the_source_bit_for_bit_and_outside_cells_see_the_end_cells():
    rng = np.random.default_rng(23)
    xs = (_increasing(rng, 7), _increasing(rng, 5))
    q = rng.uniform(-1, 1, (7, 5, 2))
    q[2, 3, 0], q[0, 0, 1] = -0.0, -0.0
    out = R.remap(q, xs, xs, R.PCM)
    assert R.same_bits(out, q).all() and np.signbit(out[2, 3, 0])
    out = R.remap(q, xs, xs, R.PLM)  # (q + s * 0.0: -0.0 comes back as +0.0 where the slope is not negative)
    assert np.array_equal(out, q)
    # destination cells wholly outside: the corner / edge cell's mean, both methods
    xd = (np.array([xs[0][0] - 2, xs[0][0] - 1, xs[0][-1] + 1, xs[0][-1] + 2]), np.array([xs[1][-1] + 1, xs[1][-1] + 3]))
    for method in METHODS:
        out = R.remap(q, xs, xd, method)
        assert np.array_equal(out[0, 0], q[0, -1]) and np.array_equal(out[2, 0], q[-1, -1])
