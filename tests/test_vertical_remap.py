"""``gt4py_amd.vertical`` without a GPU: properties of the arithmetic contract (on its restatement tests/vertical_remap_ref.py;
they do not depend on the order of operations, so they pin the contract itself), every refusal of the C entry through the dry run
(made-up addresses that are never dereferenced), the declaration, the kernels' resources and the Python interface's argument
checks."""

import math

import numpy as np
import pytest

import entry_checks as E
import vertical_remap_ref as V
from entry_checks import INV, OOB, UNS, as_arg, int64s
from gt4py_amd import _lib, vertical

HOST = (8, 9, 5)  # the shape of a host field where a test states none
EPS = float(np.finfo(np.float64).eps)
METHODS = [V.PCM, V.PLM]


# ---- the contract's properties ---------------------------------------------------------------------------------------------------
def _edges(rng, n, lo=None, hi=None):
    """n + 1 strictly increasing edges; with lo / hi the outer ones are exactly those."""
    z = np.cumsum(rng.uniform(0.05, 1.0, n + 1))
    if lo is not None:
        z = lo + (z - z[0]) * ((hi - lo) / (z[-1] - z[0]))
        z[0], z[-1] = lo, hi
        assert (np.diff(z) > 0).all()
    return [float(x) for x in z]


def _columns(count=2000, seed=5):
    rng = np.random.default_rng(seed)
    for _ in range(count):
        ns, nd = (int(x) for x in rng.integers(1, 12, 2))
        zs = _edges(rng, ns)
        kind = int(rng.integers(0, 3))
        if kind == 0:  # values of both signs
            q = rng.uniform(-1, 1, ns)
        elif kind == 1:  # a smooth monotone profile: the limited slopes are not zero
            q = np.cumsum(rng.uniform(0.1, 1.0, ns)) * 10.0 ** int(rng.integers(-3, 4))
        else:  # large offset, small variation
            q = 1.0e6 + rng.uniform(-1, 1, ns)
        yield rng, ns, nd, zs, [float(x) for x in q]


def test_identity_returns_the_source_bit_for_bit():
    for _, ns, _, zs, q in _columns():
        for method in METHODS:
            out, terms = V.remap_column(zs, list(zs), q, method)
            assert terms == ns
            assert [x.hex() for x in out] == [x.hex() for x in q], (method, zs, q)


def test_identity_keeps_a_negative_zero_for_pcm_and_plm_returns_a_positive_one():
    zs = [0.0, 1.0, 2.5, 3.0]
    for q in ([1.0, -0.0, 2.0], [-0.0, -0.0, 1.0], [3.0, 2.0, -0.0]):  # an extremum (slope 0), and the two end cells (slope 0)
        out, _ = V.remap_column(zs, zs, q, V.PCM)
        assert [x.hex() for x in out] == [x.hex() for x in q]
        out, _ = V.remap_column(zs, zs, q, V.PLM)
        assert out == q and all(math.copysign(1.0, x) == 1.0 for x in out if x == 0.0)  # -0.0 + 0.0 * 0.0 = +0.0


def test_a_column_makes_at_most_ns_plus_nd_minus_one_terms():
    worst = 0.0
    for rng, ns, nd, zs, q in _columns():
        for zd in (_edges(rng, nd), _edges(rng, nd, zs[0], zs[-1]), _edges(rng, nd, zs[0] - 3.0, zs[-1] + 3.0)):
            _, terms = V.remap_column(zs, zd, q, V.PCM)
            assert nd <= terms <= ns + nd - 1, (ns, nd, terms)
            worst = max(worst, terms / (ns + nd - 1))
    assert worst == 1.0  # the bound is reached


def test_conservation():
    """With coinciding outer edges |sum out dzd - sum q dzs| <= 4 (ns + nd) eps sum |q| dzs: the factor 4 covers the roundings of one
    term -- r - l, the division, v, the product."""
    worst = 0.0
    for rng, ns, nd, zs, q in _columns():
        zd = _edges(rng, nd, zs[0], zs[-1])
        for method in METHODS:
            out, _ = V.remap_column(zs, zd, q, method)
            have = math.fsum(o * (b - a) for o, a, b in zip(out, zd, zd[1:]))
            want = math.fsum(x * (b - a) for x, a, b in zip(q, zs, zs[1:]))
            scale = math.fsum(abs(x) * (b - a) for x, a, b in zip(q, zs, zs[1:]))
            bound = 4 * (ns + nd) * EPS * scale
            worst = max(worst, abs(have - want) / ((ns + nd) * EPS * scale))
            assert abs(have - want) <= bound, (method, ns, nd, have, want, bound)
    print(f"conservation: worst {worst:.2f} (ns + nd) eps sum|q|dz")


def test_monotonicity():
    """Both methods keep out within [min q, max q] of the column, up to 4 eps max |q|."""
    worst = 0.0
    for rng, ns, nd, zs, q in _columns():
        slack = 4 * EPS * max(abs(x) for x in q)
        for zd in (_edges(rng, nd, zs[0], zs[-1]), _edges(rng, nd, zs[0] - 2.0, zs[-1] + 2.0), _edges(rng, nd)):
            for method in METHODS:
                out, _ = V.remap_column(zs, zd, q, method)
                excess = max(max(out) - max(q), min(q) - min(out))
                worst = max(worst, excess / slack)
                assert excess <= slack, (method, ns, nd, excess, slack)
    print(f"monotonicity: worst excess {worst:.3f} of the allowance")


def test_a_constant_field_comes_back():
    for rng, ns, nd, zs, _ in _columns(500):
        c = float(rng.uniform(-5, 5)) * 10.0 ** int(rng.integers(-3, 4))
        for zd in (_edges(rng, nd), _edges(rng, nd, zs[0] - 1.0, zs[-1] + 1.0)):
            for method in METHODS:
                out, _ = V.remap_column(zs, zd, [c] * ns, method)
                assert max(abs(o - c) for o in out) <= 4 * (ns + 1) * EPS * abs(c), (method, ns, nd)


def test_a_target_outside_the_source_range_sees_the_end_cells():
    out, terms = V.remap_column([0.0, 1.0, 2.0], [-1.0, 0.5, 3.0], [1.0, 2.0], V.PCM)
    assert out == [1.0, 1.8] and terms == 3
    # the weights of a cell that lies wholly outside still sum to 1
    out, _ = V.remap_column([0.0, 1.0, 2.0], [-5.0, -4.0, 7.0, 9.0], [1.0, 2.0], V.PLM)
    assert out[0] == 1.0 and out[2] == 2.0


def test_degenerate_columns_end_and_give_what_ieee_gives():
    nan = float("nan")
    out, terms = V.remap_column([0.0, 1.0, 2.0, 3.0], [0.0, 1.5, 1.5, 3.0], [1.0, 2.0, 3.0], V.PCM)  # a repeated target edge
    assert terms <= 5 and math.isnan(out[1]) and out[0] == (1.0 / 1.5) * 1.0 + (0.5 / 1.5) * 2.0
    for method in METHODS:
        for zs in ([0.0, nan, 2.0, 3.0], [nan] * 4, [3.0, 2.0, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0]):
            out, terms = V.remap_column(zs, [0.5, 1.5, 2.5], [1.0, 2.0, 3.0], method)
            assert len(out) == 2 and terms <= 4
    assert V.div(1.0, 0.0) == math.inf and V.div(-1.0, 0.0) == -math.inf and V.div(1.0, -0.0) == -math.inf and math.isnan(V.div(0.0, 0.0))


def test_the_array_form_rounds_once_and_broadcasts_a_shared_column_of_edges():
    rng = np.random.default_rng(3)
    q = rng.uniform(-1, 1, (2, 3, 4)).astype(np.float32)
    zs = np.array(_edges(rng, 4), dtype=np.float32)
    zd = np.cumsum(rng.uniform(0.1, 1, (2, 3, 6)), axis=2)
    out = V.remap_as(q, zs, zd, V.PLM)
    assert out.dtype == np.float32 and out.shape == (2, 3, 5)
    col, _ = V.remap_column([float(x) for x in zs], [float(x) for x in zd[1, 2]], [float(x) for x in q[1, 2]], V.PLM)
    assert np.array_equal(out[1, 2], np.asarray(col).astype(np.float32))
    assert V.same_bits(np.array([np.nan, -0.0]), np.array([-np.nan, 0.0])).tolist() == [True, False]


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_header_signature_and_the_abi_is_still_8():
    # the header states the contract and that the reference has no counterpart; the enums of header and binding agree
    E.check_binding("gt4mi_vertical_remap",
                    ["const gt4mi_field* dst", "const gt4mi_field* src", "int nfields", "const gt4mi_field* src_edges",
                     "const gt4mi_field* dst_edges", "const int64_t extent_ij[2]", "int64_t ns", "int64_t nd", "int elem_size",
                     "int edge_elem_size", "int method", "int flags", "void* stream", "int* launches"],
                    prefix="REMAP", constants=("PCM", "PLM", "DRY_RUN"),
                    phrases=("no reference counterpart", "user stencils", "(r - l) / d", "zs[k+1] >= hi", "copysign", "ns + nd - 1"))
    assert vertical.METHODS == {"pcm": _lib.REMAP_PCM, "plm": _lib.REMAP_PLM}


DST, SRC, ZS, ZD = 0x10_0000, 0x4000_0000, 0x8000_0000, 0xC000_0000  # made-up device addresses, far apart
NS, ND = 5, 3


def _field(ptr, nk, shape_ij=(6, 6), strides=None, origin=(1, 1, 0), itemsize=8):  # (nk first; this file's plane)
    return E.field(ptr, (*shape_ij, nk), strides, origin, itemsize)


def _call(dst, src, zs, zd, nfields=1, extent=(4, 4), ns=NS, nd=ND, size=8, edge_size=8, method=0, flags=0):
    return E.call("gt4mi_vertical_remap", as_arg(dst), as_arg(src), nfields, as_arg(zs), as_arg(zd), int64s(extent), ns, nd, size, edge_size,
                  method, flags | _lib.REMAP_DRY_RUN, None, outs=(77,))


def test_every_refusal_of_the_c_entry_without_a_gpu():
    """Every check runs before the first launch: these calls carry made-up device addresses and the dry-run flag."""
    d, s, zs, zd = _field(DST, ND), _field(SRC, NS), _field(ZS, NS + 1), _field(ZD, ND + 1)
    rc, msg, launches = _call(d, s, zs, zd)
    assert rc == 0 and launches == 1, msg
    for method in (_lib.REMAP_PCM, _lib.REMAP_PLM):
        for size, edge_size in ((4, 4), (4, 8), (8, 4)):
            args = [_field(p, n, itemsize=i) for p, n, i in ((DST, ND, size), (SRC, NS, size), (ZS, NS + 1, edge_size), (ZD, ND + 1, edge_size))]
            rc, msg, launches = _call(*args, size=size, edge_size=edge_size, method=method)
            assert rc == 0 and launches == 1, msg
    # null pointers
    for n, what in enumerate((b"dst is null", b"src is null", b"src_edges is null", b"dst_edges is null")):
        args = [d, s, zs, zd]
        args[n] = None
        rc, msg, launches = _call(*args)
        assert rc == INV and what in msg and launches == 0, msg
    rc, msg, _ = _call(d, s, zs, zd, extent=None)
    assert rc == INV and b"extent_ij is null" in msg
    for n, what in enumerate((b"dst 0 is null", b"src 0 is null", b"src_edges 0 is null", b"dst_edges 0 is null")):
        args = [d, s, zs, zd]
        args[n] = _field(0, 8)
        rc, msg, launches = _call(*args)
        assert rc == INV and what in msg and launches == 0, msg
    # counts, extents, flags, method
    for n in (0, -2):
        rc, msg, launches = _call(d, s, zs, zd, nfields=n)
        assert rc == INV and b"nfields" in msg and launches == 0
    rc, msg, _ = _call(d, s, zs, zd, ns=0)
    assert rc == INV and b"ns = 0" in msg
    rc, msg, _ = _call(d, s, zs, zd, nd=-1)
    assert rc == INV and b"nd = -1" in msg
    rc, msg, _ = _call(d, s, zs, zd, extent=(4, -1))
    assert rc == INV and b"invalid extent -1 along axis 1" in msg
    rc, msg, _ = _call(d, s, zs, zd, flags=2)
    assert rc == INV and b"flags" in msg
    for method in (2, -1):
        rc, msg, launches = _call(d, s, zs, zd, method=method)
        assert rc == INV and b"unknown method" in msg and launches == 0
    # item sizes other than 4 or 8
    rc, msg, _ = _call(d, s, zs, zd, size=2)
    assert rc == UNS and b"field item size 2" in msg
    rc, msg, _ = _call(d, s, zs, zd, edge_size=16)
    assert rc == UNS and b"edge item size 16" in msg
    # a box that does not fit its field: I, J, and the levels of every role (an edge field needs one more than its fields)
    rc, msg, launches = _call(d, s, zs, zd, extent=(6, 4))
    assert rc == OOB and b"dst 0" in msg and b"axis 0" in msg and launches == 0
    rc, msg, _ = _call(_field(DST, ND, (8, 8)), s, zs, zd, extent=(4, 6))
    assert rc == OOB and b"src 0" in msg and b"axis 1" in msg
    rc, msg, _ = _call(d, s, zs, zd, nd=ND + 1)
    assert rc == OOB and b"dst 0" in msg and b"axis 2" in msg
    rc, msg, _ = _call(d, s, zs, zd, ns=NS + 1)
    assert rc == OOB and b"src 0" in msg and b"axis 2" in msg
    rc, msg, _ = _call(d, s, _field(ZS, NS), zd)
    assert rc == OOB and b"src_edges 0" in msg and b"extent 6 along axis 2" in msg
    rc, msg, _ = _call(d, s, zs, _field(ZD, ND))
    assert rc == OOB and b"dst_edges 0" in msg and b"extent 4 along axis 2" in msg
    rc, msg, _ = _call(d, _field(SRC, NS, origin=(1, -1, 0)), zs, zd)
    assert rc == OOB and b"negative origin -1 along axis 1" in msg
    # strides and alignment the kernels do not take
    rc, msg, _ = _call(_field(DST, ND, strides=(8, 52, 312)), s, zs, zd)
    assert rc == UNS and b"multiple of the item size" in msg
    rc, msg, _ = _call(d, s, _field(ZS + 4, NS + 1), zd)
    assert rc == UNS and b"not aligned to its item size" in msg
    # stride 0: refused for a dst on an extent above 1, fine on an extent of 1; a src and the edge fields broadcast, and a
    # broadcast axis of an edge field has no shape to check
    rc, msg, launches = _call(_field(DST, ND, strides=(0, 8, 48)), s, zs, zd)
    assert rc == INV and b"dst 0 has stride 0 along axis 0" in msg and launches == 0
    rc, msg, _ = _call(_field(DST, ND, strides=(8, 48, 0)), s, zs, zd)
    assert rc == INV and b"dst 0 has stride 0 along axis 2" in msg
    rc, msg, _ = _call(_field(DST, 1, strides=(8, 48, 0)), s, zs, _field(ZD, 2), nd=1)
    assert rc == 0, msg
    rc, msg, _ = _call(d, _field(SRC, NS, strides=(0, 0, 8)), zs, zd)
    assert rc == 0, msg
    column = lambda ptr, n: _lib.Field.make(ptr, (1, 1, n), (0, 0, 8), (0, 0, 0))  # noqa: E731  (a Field[K])
    rc, msg, launches = _call(d, s, column(ZS, NS + 1), column(ZD, ND + 1))
    assert rc == 0 and launches == 1, msg
    rc, msg, _ = _call(d, s, column(ZS, NS), column(ZD, ND + 1))
    assert rc == OOB and b"src_edges 0" in msg and b"axis 2" in msg
    # overlap in memory: a dst against its src, another pair's src, either edge field, another dst; a byte apart is fine
    rc, msg, launches = _call(d, _field(DST, NS), zs, zd)
    assert rc == UNS and b"dst 0 and src 0 overlap in memory" in msg and launches == 0
    first, last = 8 * (1 + 6), 8 * (4 + 6 * 4 + 36 * (ND - 1))  # byte offsets of the dst box's first and last item
    rc, msg, _ = _call(d, _field(DST + last - first, NS), zs, zd)  # src's first item IS dst's last
    assert rc == UNS and b"overlap in memory" in msg
    rc, msg, _ = _call(d, _field(DST + last - first + 8, NS), zs, zd)  # the byte ranges of the BOXES do not meet
    assert rc == 0, msg
    rc, msg, _ = _call(d, s, _field(DST + 64, NS + 1), zd)
    assert rc == UNS and b"dst 0 and src_edges overlap in memory" in msg
    rc, msg, _ = _call(d, s, zs, column(DST + 8 * 40, ND + 1))
    assert rc == UNS and b"dst 0 and dst_edges overlap in memory" in msg
    two = lambda a, b: E.table((a, b))  # noqa: E731
    rc, msg, _ = _call(two(d, _field(DST + 0x1000, ND)), two(s, _field(DST + 64, NS)), zs, zd, nfields=2)
    assert rc == UNS and b"dst 0 and src 1 overlap in memory" in msg
    rc, msg, _ = _call(two(d, _field(DST + 128, ND)), two(s, _field(SRC + 0x1000, NS)), zs, zd, nfields=2)
    assert rc == UNS and b"dst 0 and dst 1 overlap in memory" in msg
    rc, msg, launches = _call(two(d, _field(DST + 0x1000, ND)), two(s, s), zs, zd, nfields=2)  # one src for two dsts is fine
    assert rc == 0 and launches == 1, msg
    rc, msg, _ = _call(d, s, zs, zs, nd=NS)  # and so is one edge field on both sides (the identity)
    assert rc == OOB  # (dst holds ND levels only)
    rc, msg, _ = _call(_field(DST, NS), s, zs, zs, nd=NS)
    assert rc == 0, msg
    # an extent with a zero entry: OK, nothing to launch -- after the checks
    rc, msg, launches = _call(d, s, zs, zd, extent=(4, 0))
    assert rc == 0 and launches == 0, msg
    rc, msg, launches = _call(d, s, zs, zd, extent=(7, 0))
    assert rc == OOB and launches == 0


def test_launches_are_one_per_eight_pairs():
    d = E.table(_field(DST + n * 0x1000, ND) for n in range(9))
    s = E.table(_field(SRC + n * 0x1000, NS) for n in range(9))
    zs, zd = _field(ZS, NS + 1), _field(ZD, ND + 1)
    assert [_call(d, s, zs, zd, nfields=n)[2] for n in (1, 3, 8, 9)] == [1, 1, 1, 2]


def test_the_kernels_are_in_the_resource_log_without_scratch():
    kernels = E.kernel_resources(r"vertical_remap_kernel")
    # 2 field types x 2 edge types x 2 methods x the register budgets for 1, 4 and 8 entries
    assert len(kernels) == 24 and len({name for name, *_ in kernels}) == 24, kernels
    for name, scratch, waves, lds in kernels:
        assert int(scratch) == 0 and int(waves) >= 2 and int(lds) == 0, (name, scratch, waves, lds)


# ---- the Python interface: every refusal before any GPU work ---------------------------------------------------------------
def _good(**over):
    args = dict(dst=E.host_field((8, 9, 3)), src=E.host_field(HOST), src_edges=E.host_field((8, 9, 6)), dst_edges=E.host_field((4,)))
    args.update(over)
    return args.pop("dst"), args.pop("src"), args


@pytest.mark.parametrize("kwargs, error, match", [
    (dict(halo=2.0), ValueError, "halo must be"),
    (dict(halo=((1, 1.5), (1, 1))), TypeError, "halo widths must be ints"),
    (dict(halo=-1), ValueError, "must not be negative"),
    (dict(halo=5), ValueError, "leave no domain"),
    (dict(halo=2, origin=(1, 2, 0)), ValueError, "negative origin -1 along axis 0"),
    (dict(origin=(0, 0, 0, 0)), ValueError, "at most three entries"),
    (dict(origin=(0, 0, 5)), ValueError, "leaves no level"),
    (dict(method="ppm"), ValueError, "method must be one of"),
    (dict(halo=((1, 2), (0, 3)), method="plm"), TypeError, "device fields"),  # all checks passed: refused for being host memory
    (dict(), TypeError, "device fields"),
])
def test_python_refusals_need_no_gpu(kwargs, error, match):
    dst, src, edges = _good()
    with pytest.raises(error, match=match):
        vertical.remap_levels(dst, src, **edges, **kwargs)
    with pytest.raises(error, match=match):
        vertical.VerticalRemap([dst], [src], **edges, **kwargs)


def test_python_refusals_about_the_fields_themselves():
    import torch

    R = vertical.remap_levels
    dst, src, edges = _good()
    with pytest.raises(ValueError, match="at least one"):
        R([], [], **edges)
    with pytest.raises(ValueError, match="2 destination.s. and 1 source"):
        R([dst, E.host_field((8, 9, 3))], [src], **edges)
    with pytest.raises(TypeError, match="host"):
        R(torch.zeros(8, 9, 3, dtype=torch.float64), src, **edges)  # as_device_array's own refusal
    with pytest.raises(TypeError):
        R(dst, np.zeros((8, 9, 5)), **edges)
    with pytest.raises(TypeError):
        R(dst, src, src_edges=np.zeros((8, 9, 6)), dst_edges=edges["dst_edges"])
    with pytest.raises(ValueError, match="takes IJK fields"):
        R(E.host_field((8, 9)), src, **edges)
    with pytest.raises(ValueError, match="dst_edges must be an IJK field or a Field.K."):
        R(dst, src, src_edges=edges["src_edges"], dst_edges=E.host_field((9, 4)))
    # dtypes: the fields share one, the edge fields share one (not necessarily the same), all float32 or float64
    with pytest.raises(TypeError, match="share a dtype"):
        R(E.host_field((8, 9, 3), "float32"), src, **edges)
    with pytest.raises(TypeError, match="float32 or float64 fields"):
        R(E.host_field((8, 9, 3), "int64"), E.host_field(HOST, dtype="int64"), **edges)
    with pytest.raises(TypeError, match="src_edges and dst_edges share a dtype"):
        R(dst, src, src_edges=edges["src_edges"], dst_edges=E.host_field((4,), "float32"))
    with pytest.raises(TypeError, match="edge fields are float32 or float64"):
        R(dst, src, src_edges=E.host_field((8, 9, 6), "int32"), dst_edges=E.host_field((4,), "int32"))
    with pytest.raises(TypeError, match="device fields"):  # float32 fields against float64 edges is a combination of its own
        R(E.host_field((8, 9, 3), "float32"), E.host_field(HOST, dtype="float32"), **edges)
    # levels: the sources share theirs, an edge field has exactly one more
    with pytest.raises(ValueError, match="sources of one call share their number of levels: 5 and 4"):
        R([dst, E.host_field((8, 9, 3))], [src, E.host_field((8, 9, 4))], **edges)
    with pytest.raises(ValueError, match="src_edges has 5 edges along K, 5 levels need 6"):
        R(dst, src, src_edges=E.host_field((8, 9, 5)), dst_edges=edges["dst_edges"])
    with pytest.raises(ValueError, match="dst_edges has 3 edges along K, 3 levels need 4"):
        R(dst, src, src_edges=edges["src_edges"], dst_edges=E.host_field((3,)))
    # a field onto itself; a dst that is also the edge field
    x = E.host_field((8, 9, 5))
    with pytest.raises(TypeError, match="dst 0 and src 0 overlap in memory"):
        R(x, x, src_edges=edges["src_edges"], dst_edges=E.host_field((6,)))
    z = E.host_field((8, 9, 6))
    with pytest.raises(TypeError, match="dst 0 and src_edges overlap in memory"):
        R(z, E.host_field((8, 9, 5)), src_edges=z, dst_edges=E.host_field((7,)))


def test_a_frozen_remap_knows_its_box_and_refuses_to_run_after_an_array_died(monkeypatch):
    """The weak references are taken last, behind the device check: what they guard is shown on a VerticalRemap whose device
    check is made to pass for host memory -- the call itself is never reached, the dead reference is found first."""
    E.on_device(monkeypatch)
    dsts, srcs = [E.host_field((8, 9, 3)) for _ in range(9)], [E.host_field((10, 9, 5)) for _ in range(9)]
    zs, zd = E.host_field((8, 9, 6), "float32"), E.host_field((4,), "float32")
    vr = vertical.VerticalRemap(dsts, srcs, src_edges=zs, dst_edges=zd, method="plm", halo=1)
    assert (vr.ns, vr.nd, vr.launches, vr.extent, vr.domain, vr.origin, vr.method) == (5, 3, 2, (8, 9), (6, 7), (1, 1, 0), "plm")
    del zd
    E.refuses_a_dead_array(vr)
