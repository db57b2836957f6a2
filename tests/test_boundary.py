"""``gt4py_amd.boundary`` without a GPU: the contract's numpy restatement against ``numpy.pad``, the C entry's declaration,
every refusal (raised before any GPU work), and ``physical_sides``."""

import ctypes
import itertools

import numpy as np
import pytest

import boundary_ref as R
import entry_checks as E
from entry_checks import INV, OOB, UNS, int64s
from gt4py_amd import _lib, boundary
from gt4py_amd.distributed.halo import Decomposition

HOST = (8, 9, 3)  # the shape of a host field where a test states none
SENTINEL = -12345.0


# ---- the restatement (tests/boundary_ref.py) is numpy.pad, axis by axis ------------------------------------------------------
SHAPES = [(4, 5, 2), (7, 3, 1), (3, 3, 3), (9, 6, 2)]
WIDTHS = [(1, 1, 1, 1), (2, 2, 2, 2), (2, 3, 0, 2)]
# how many of the 4 shapes x 3 width sets x 25 pairs of modes the width rule admits (all pairs / pairs without "constant"): 300 and
# 192 less the 5 and 4 pairs with REFLECT in I on shape (3, 3, 3) with the high I width 3 > n - 1; no width here exceeds n
CHECKED, COPYING = 295, 188


def _pad(interior, widths, modes, value):
    out = interior
    for axis, mode in enumerate(modes):
        pad = [(0, 0)] * 3
        pad[axis] = tuple(widths[2 * axis: 2 * axis + 2])
        kwargs = {"constant_values": value} if mode == "constant" else {}
        out = np.pad(out, pad, mode=R.NUMPY_PAD[mode], **kwargs)
    return out


def test_restatement_equals_numpy_pad_for_every_pair_of_modes():
    rng = np.random.default_rng(11)
    checked = copying = 0
    for shape, widths, modes in itertools.product(SHAPES, WIDTHS, R.mode_pairs(with_none=False)):
        if not R.admissible(modes, widths, shape):
            continue
        interior = rng.uniform(-1, 1, shape)
        lo_i, hi_i, lo_j, hi_j = widths
        # one more ghost cell than the widths on every side, and a level below and above: they must stay as they are
        a = np.full((shape[0] + lo_i + hi_i + 2, shape[1] + lo_j + hi_j + 2, shape[2] + 2), SENTINEL)
        origin = (lo_i + 1, lo_j + 1, 1)
        a[origin[0]: origin[0] + shape[0], origin[1]: origin[1] + shape[1], 1:-1] = interior
        want = np.full_like(a, SENTINEL)
        want[1:-1, 1:-1, 1:-1] = _pad(interior, widths, modes, 2.5)
        R.fill(a, origin, shape, widths, modes, value=2.5)
        assert np.array_equal(a, want), (shape, widths, modes)
        checked += 1
        copying += "constant" not in modes
    print(f"{checked} admissible combinations, {copying} of them of the four copying modes alone")
    assert (checked, copying) == (CHECKED, COPYING)  # pinned: the grid cannot shrink unnoticed


def test_index_maps_are_the_table():
    n = 6
    table = {"periodic": ([5, 4, 3], [0, 1, 2]), "zero_gradient": ([0, 0, 0], [5, 5, 5]), "symmetric": ([0, 1, 2], [5, 4, 3]),
             "reflect": ([1, 2, 3], [4, 3, 2])}
    for mode, (low, high) in table.items():
        assert [R.source_index(mode, True, d, n) for d in (1, 2, 3)] == low
        assert [R.source_index(mode, False, d, n) for d in (1, 2, 3)] == high


def test_sides_and_corner_rule_of_the_restatement():
    """J sides only over pre-filled I ghosts: the corners take the CURRENT content of the ghost columns."""
    a = np.arange(6 * 6, dtype=np.float64).reshape(6, 6, 1)
    before = a.copy()
    R.fill(a, (1, 1, 0), (4, 4, 1), (1, 1, 1, 1), ("periodic", "zero_gradient"), sides=R.J_LO | R.J_HI)
    assert np.array_equal(a[:, 1:5], before[:, 1:5])  # I ghosts and the domain untouched
    assert np.array_equal(a[:, 0], before[:, 1]) and np.array_equal(a[:, 5], before[:, 4])  # corners from the ghost columns
    b = before.copy()
    R.fill(b, (1, 1, 0), (4, 4, 1), (1, 1, 1, 1), ("periodic", "zero_gradient"), sides=R.I_LO)
    assert np.array_equal(b[0, 1:5], before[4, 1:5]) and np.array_equal(b[1:], before[1:]) and b[0, 0] == before[0, 0]


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_header_signature_and_abi_8():
    # the header says the entry has no reference counterpart, and the enums of header and binding agree
    E.check_binding("gt4mi_halo_fill",
                    ["const gt4mi_field* fields", "int nfields", "const int64_t domain[3]", "const int64_t halo[4]", "int mode_i",
                     "int mode_j", "int sides", "const void* value", "int elem_size", "void* stream", "int* launches"],
                    prefix="HALO", constants=("NONE", "PERIODIC", "ZERO_GRADIENT", "SYMMETRIC", "REFLECT", "CONSTANT", "I_LO", "I_HI", "J_LO",
                                              "J_HI", "ALL_SIDES", "DRY_RUN"),
                    phrases=("no reference counterpart",))
    assert boundary.ALL == boundary.I_LO | boundary.I_HI | boundary.J_LO | boundary.J_HI == 15


def _call(fields, nfields=1, domain=(4, 4, 2), halo=(1, 1, 1, 1), mode_i=_lib.HALO_PERIODIC, mode_j=_lib.HALO_PERIODIC,
          sides=_lib.HALO_ALL_SIDES, value=b"\0" * 8, elem_size=8):
    return E.call("gt4mi_halo_fill", fields, nfields, int64s(domain), int64s(halo), mode_i, mode_j, sides, value, elem_size, None, outs=(77,))


def test_argument_errors_of_the_c_entry_without_a_gpu():
    """Every check runs before the first launch: these calls carry fake device addresses and never reach the GPU."""
    f = ctypes.byref(_lib.Field.make(0x10000, (6, 6, 2), (8, 48, 288), (1, 1, 0)))
    rc, msg, launches = _call(None)
    assert rc == INV and b"null" in msg and launches == 0
    null_data = ctypes.byref(_lib.Field.make(0, (6, 6, 2), (8, 48, 288), (1, 1, 0)))
    rc, msg, _ = _call(null_data)
    assert rc == INV and b"null" in msg
    rc, msg, _ = _call(f, nfields=0)
    assert rc == INV and b"nfields" in msg
    rc, msg, _ = _call(f, domain=None)
    assert rc == INV and b"null" in msg
    rc, msg, _ = _call(f, halo=None)
    assert rc == INV and b"null" in msg
    rc, msg, _ = _call(f, mode_i=_lib.HALO_CONSTANT, value=None)
    assert rc == INV and b"value is null" in msg
    rc, msg, _ = _call(f, mode_j=9)
    assert rc == INV and b"unknown mode 9 for axis J" in msg
    rc, msg, _ = _call(f, sides=32)
    assert rc == INV and b"sides" in msg
    rc, msg, _ = _call(f, elem_size=3)
    assert rc == UNS and b"item size 3" in msg
    rc, msg, _ = _call(f, halo=(1, -1, 1, 1))
    assert rc == INV and b"high width -1 along axis I" in msg
    # widths outside the array: low side (origin 1), high side (1 + 4 + 2 > 6)
    rc, msg, _ = _call(f, halo=(2, 1, 1, 1))
    assert rc == OOB and b"low width 2 along axis 0" in msg
    rc, msg, _ = _call(f, halo=(1, 1, 1, 2))
    assert rc == OOB and b"high width 2 along axis 1" in msg
    rc, msg, _ = _call(f, domain=(4, 4, 3))
    assert rc == OOB and b"axis 2" in msg
    # width against mode: PERIODIC / SYMMETRIC take at most n, REFLECT n - 1; ZERO_GRADIENT and CONSTANT whatever fits
    big = ctypes.byref(_lib.Field.make(0x10000, (12, 12, 2), (8, 96, 1152), (5, 5, 0)))
    for mode, width, refused in ((_lib.HALO_PERIODIC, 2, False), (_lib.HALO_PERIODIC, 3, True), (_lib.HALO_SYMMETRIC, 3, True),
                                 (_lib.HALO_REFLECT, 1, False), (_lib.HALO_REFLECT, 2, True), (_lib.HALO_ZERO_GRADIENT, 5, False),
                                 (_lib.HALO_CONSTANT, 5, False)):
        rc, msg, launches = _call(big, domain=(2, 2, 2), halo=(1, width, 1, 1), mode_i=mode, sides=_lib.HALO_ALL_SIDES | _lib.HALO_DRY_RUN)
        if refused:
            assert rc == INV and b"high width %d along axis I is larger than" % width in msg and launches == 0, (mode, width, msg)
        else:
            assert rc == 0 and launches == 1, (mode, width, msg)
        rc, msg, _ = _call(big, domain=(2, 2, 2), halo=(1, 1, width, 1), mode_j=mode, sides=_lib.HALO_ALL_SIDES | _lib.HALO_DRY_RUN)
        assert (rc == INV and b"low width %d along axis J" % width in msg) if refused else rc == 0, (mode, width, msg)
    # a field without an I axis (stride 0), a stride that is no multiple of the item size
    rc, msg, _ = _call(ctypes.byref(_lib.Field.make(0x10000, (6, 6, 2), (0, 8, 48), (1, 1, 0))))
    assert rc == INV and b"no I axis" in msg
    rc, msg, _ = _call(ctypes.byref(_lib.Field.make(0x10000, (6, 6, 2), (8, 0, 48), (1, 1, 0))))
    assert rc == INV and b"no J axis" in msg
    rc, msg, _ = _call(ctypes.byref(_lib.Field.make(0x10000, (6, 6, 2), (8, 52, 312), (1, 1, 0))))
    assert rc == UNS and b"multiple of the item size" in msg
    # the dry run counts launches: one per eight fields; nothing to do = none
    many = E.table(_lib.Field.make(0x10000 * (n + 1), (6, 6, 2), (8, 48, 288), (1, 1, 0)) for n in range(17))
    dry = _lib.HALO_ALL_SIDES | _lib.HALO_DRY_RUN
    assert [_call(many, nfields=n, sides=dry)[2] for n in (1, 8, 9, 16, 17)] == [1, 1, 2, 2, 3]
    assert _call(many, nfields=8, sides=dry, mode_i=_lib.HALO_NONE, mode_j=_lib.HALO_NONE)[::2] == (0, 0)
    assert _call(many, nfields=8, sides=_lib.HALO_DRY_RUN)[::2] == (0, 0)


def test_a_row_longer_than_an_int_is_refused_even_without_j_rows():
    """I faces only: the products of rows and row length do not see a padded I range that an int cannot index."""
    n = 2**31 - 100
    f = ctypes.byref(_lib.Field.make(0x10000, (n + 2, 3, 1), (1, n + 2, 3 * (n + 2)), (1, 1, 0)))
    rc, msg, launches = _call(f, domain=(n, 1, 1), halo=(1, 1, 0, 0), mode_i=_lib.HALO_PERIODIC, mode_j=_lib.HALO_NONE, elem_size=1)
    assert rc == _lib.ERR_UNSUPPORTED and b"too many ghost cells" in msg and launches == 0


def test_the_kernels_are_in_the_resource_log_and_use_no_scratch():
    kernels = E.kernel_resources(r"halo_fill_kernel")
    assert len(kernels) == 4, kernels  # item sizes 1, 2, 4, 8
    assert all(int(scratch) == 0 and int(lds) == 0 for _, scratch, _, lds in kernels), kernels


# ---- the Python interface: every refusal before any GPU work ---------------------------------------------------------------
@pytest.mark.parametrize("kwargs, error, match", [
    (dict(halo=2, mode="bogus"), ValueError, "unknown boundary mode 'bogus'"),
    (dict(halo=2, mode=("periodic", "reflect", None)), ValueError, "mode_i, mode_j"),
    (dict(halo=2, mode=3), TypeError, "mode must be a name"),
    (dict(halo=2.0, mode="periodic"), ValueError, "halo must be"),
    (dict(halo=(1, 2, 3), mode="periodic"), ValueError, "halo must be"),
    (dict(halo=((1, 1.5), (1, 1)), mode="periodic"), TypeError, "halo widths must be ints"),
    (dict(halo=1, mode="periodic", sides=16), ValueError, "sides"),
    (dict(halo=1, mode="periodic", sides="all"), TypeError, "sides"),
    (dict(halo=5, mode="periodic"), ValueError, "leave no domain"),
    (dict(halo=-1, mode="periodic"), ValueError, "invalid low width -1 along axis I"),
    (dict(halo=2, mode="periodic", origin=(1, 2, 0)), ValueError, "low width 2 along axis 0 is outside the array"),
    (dict(halo=2, mode="periodic", origin=(2, 2, 0), domain=(4, 6, 3)), ValueError, "high width 2 along axis 1 is outside the array"),
    (dict(halo=2, mode="periodic", domain=(4, 5, 4)), ValueError, "axis 2"),
    (dict(halo=3, mode=("reflect", None), origin=(3, 3, 0), domain=(2, 3, 3)), ValueError, "low width 3 along axis I is larger than 1, the most mode REFLECT"),
    (dict(halo=3, mode=(None, "symmetric"), origin=(3, 3, 0), domain=(2, 2, 3)), ValueError, "low width 3 along axis J is larger than 2, the most mode SYMMETRIC"),
    (dict(halo=3, mode="periodic", origin=(3, 3, 0), domain=(2, 3, 3)), ValueError, "along axis I is larger than 2, the most mode PERIODIC"),
    (dict(halo=1, mode="constant", value="x"), TypeError, "cannot be held"),
    (dict(halo=1, mode="constant", value=[1.0, 2.0]), TypeError, "scalar"),
    (dict(halo=1, mode="periodic"), TypeError, "device fields"),  # all checks passed: refused for being host memory
])
def test_python_refusals_need_no_gpu(kwargs, error, match):
    with pytest.raises(error, match=match):
        boundary.fill_halo(E.host_field(HOST), **kwargs)
    with pytest.raises(error, match=match):
        boundary.HaloFill([E.host_field(HOST)], **kwargs)


def test_python_refusals_about_the_fields_themselves():
    import torch

    with pytest.raises(ValueError, match="at least one field"):
        boundary.fill_halo(halo=1, mode="periodic")
    with pytest.raises(TypeError, match="host"):
        boundary.fill_halo(torch.zeros(4, 4, 2), halo=1, mode="periodic")  # as_device_array's own refusal
    with pytest.raises(TypeError):
        boundary.fill_halo(np.zeros((4, 4, 2)), halo=1, mode="periodic")
    with pytest.raises(ValueError, match="no I or no J axis"):
        boundary.fill_halo(E.host_field((8,)), halo=1, mode="periodic")
    with pytest.raises(TypeError, match="share an item size"):
        boundary.fill_halo(E.host_field(HOST), E.host_field(HOST, dtype="float32"), halo=1, mode="periodic")
    with pytest.raises(TypeError, match="share an item size"):
        boundary.fill_halo(E.host_field(HOST, dtype="int32"), E.host_field(HOST, dtype="float32"), halo=1, mode="constant")
    with pytest.raises(ValueError, match="field 1: high width 1 along axis 0"):  # the second field is smaller
        boundary.fill_halo(E.host_field(HOST), E.host_field((7, 9, 3)), halo=1, mode="periodic")


def test_defaults_of_origin_and_domain():
    with pytest.raises(TypeError, match="device fields"):
        boundary.HaloFill([E.host_field((8, 9))], halo=((1, 2), (0, 3)), mode=("reflect", "periodic"))  # Field[IJ]
    # (the object is not built for host memory; what it would have bound is checked through the library's messages)
    with pytest.raises(ValueError, match=r"high width 3 along axis J is larger than 2"):
        boundary.HaloFill([E.host_field((8, 5))], halo=((1, 2), (0, 3)), mode=("reflect", "periodic"))  # domain (5, 2, 1)


# ---- physical_sides ----------------------------------------------------------------------------------------------------------
def test_physical_sides():
    B = boundary
    assert B.physical_sides(Decomposition((64, 64, 8), (1, 1), 0, 2)) == B.ALL
    got = [B.physical_sides(Decomposition((64, 64, 8), (4, 2), r, 2)) for r in range(8)]
    row0 = [B.I_LO | B.J_LO, B.J_LO, B.J_LO, B.I_HI | B.J_LO]
    row1 = [B.I_LO | B.J_HI, B.J_HI, B.J_HI, B.I_HI | B.J_HI]
    assert got == row0 + row1
    assert all(B.physical_sides(Decomposition((64, 64, 8), (4, 2), r, 2, periodic=(True, True))) == 0 for r in range(8))
    assert B.physical_sides(Decomposition((64, 64, 8), (1, 1), 0, 1, periodic=(True, False))) == B.J_LO | B.J_HI  # a channel
    assert [B.physical_sides(Decomposition((64, 64, 8), (4, 2), r, 2, periodic=(True, False))) for r in (0, 5)] == [B.J_LO, B.J_HI]
