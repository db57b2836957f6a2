"""``gt4py_amd.transfer`` without a GPU: the C entry's declaration, every refusal (through the dry run, with made-up addresses
that are never dereferenced), the path and the launch count the library reports, the kernels' resources, the Python interface's
argument checks, and numpy's own two conversions on the edge values the GPU test plants."""

import ctypes

import numpy as np
import pytest

import device_layouts as L
import entry_checks as E
import transfer_ref as R
from entry_checks import INV, OOB, UNS, as_arg, int64s
from gt4py_amd import _lib, transfer

HOST = (8, 9, 3)  # the shape of a host field where a test states none
DST, SRC = 0x10_0000, 0x4000_0000  # made-up device addresses, far apart


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
def test_binding_declares_the_header_signature_and_the_abi_is_still_8():
    # the header says what the entry replaces, and the enums of header and binding agree
    E.check_binding("gt4mi_field_copy",
                    ["const gt4mi_field* dst", "const gt4mi_field* src", "int nfields", "const int64_t extent[3]", "int dst_elem_size",
                     "int src_elem_size", "int flags", "void* stream", "int* paths", "int* launches"],
                    prefix="COPY", constants=("PATH_ROWS", "PATH_TILES", "PATH_ITEMS", "CONVERT", "DRY_RUN"), phrases=("slicing", "cp.asarray"))
    assert (transfer.PATH_ROWS, transfer.PATH_TILES, transfer.PATH_ITEMS) == (R.ROWS, R.TILES, R.ITEMS) == (0, 1, 2)


def _field(ptr, shape=(6, 6, 2), *rest, **kwargs):  # (this file's shape)
    return E.field(ptr, shape, *rest, **kwargs)


def _call(dst, src, nfields=1, extent=(4, 4, 2), dsize=8, ssize=8, flags=0, want_paths=True):
    paths = (ctypes.c_int * max(nfields, 1))(*([-1] * max(nfields, 1)))
    rc, msg, launches = E.call("gt4mi_field_copy", as_arg(dst), as_arg(src), nfields, int64s(extent), dsize, ssize, flags | _lib.COPY_DRY_RUN, None,
                               paths if want_paths else None, outs=(77,))
    return rc, msg, launches, list(paths)


def test_every_refusal_of_the_c_entry_without_a_gpu():
    """Every check runs before the first launch: these calls carry made-up device addresses and the dry-run flag."""
    d, s = _field(DST), _field(SRC)
    rc, msg, launches, _ = _call(d, s)
    assert rc == 0 and launches == 1, msg
    # null pointers
    rc, msg, launches, _ = _call(None, s)
    assert rc == INV and b"dst is null" in msg and launches == 0
    rc, msg, _, _ = _call(d, None)
    assert rc == INV and b"src is null" in msg
    rc, msg, _, _ = _call(d, s, extent=None)
    assert rc == INV and b"extent is null" in msg
    rc, msg, _, _ = _call(_field(0), s)
    assert rc == INV and b"dst 0 is null" in msg
    rc, msg, _, _ = _call(d, _field(0))
    assert rc == INV and b"src 0 is null" in msg
    # nfields <= 0, negative extents, unknown flags
    for n in (0, -3):
        rc, msg, launches, _ = _call(d, s, nfields=n)
        assert rc == INV and b"nfields" in msg and launches == 0
    rc, msg, _, _ = _call(d, s, extent=(4, -1, 2))
    assert rc == INV and b"invalid extent -1 along axis 1" in msg
    rc, msg, _, _ = _call(d, s, flags=2)
    assert rc == INV and b"flags" in msg
    # a box outside either shape
    rc, msg, launches, _ = _call(d, s, extent=(6, 4, 2))
    assert rc == OOB and b"dst 0" in msg and b"axis 0" in msg and launches == 0
    rc, msg, _, _ = _call(_field(DST, shape=(8, 8, 2)), s, extent=(6, 4, 2))
    assert rc == OOB and b"src 0" in msg and b"axis 0" in msg
    rc, msg, _, _ = _call(d, s, extent=(4, 4, 3))
    assert rc == OOB and b"axis 2" in msg
    rc, msg, _, _ = _call(d, _field(SRC, origin=(1, -1, 0)))
    assert rc == OOB and b"negative origin -1 along axis 1" in msg
    # item sizes: other than 1, 2, 4, 8; unequal without CONVERT; CONVERT other than 4 <-> 8
    rc, msg, _, _ = _call(d, s, dsize=3, ssize=3)
    assert rc == UNS and b"item size 3" in msg
    rc, msg, _, _ = _call(d, s, dsize=8, ssize=16)
    assert rc == UNS and b"item size 16" in msg
    d4 = _field(DST, itemsize=4)
    rc, msg, _, _ = _call(d4, s, dsize=4, ssize=8)
    assert rc == UNS and b"differ and GT4MI_COPY_CONVERT is not set" in msg
    rc, msg, launches, _ = _call(d4, s, dsize=4, ssize=8, flags=_lib.COPY_CONVERT)
    assert rc == 0 and launches == 1, msg
    rc, msg, _, _ = _call(d, _field(SRC, itemsize=4), dsize=8, ssize=4, flags=_lib.COPY_CONVERT)
    assert rc == 0, msg
    rc, msg, _, _ = _call(d4, _field(SRC, itemsize=2), dsize=4, ssize=2, flags=_lib.COPY_CONVERT)
    assert rc == UNS and b"float32 <-> float64 only" in msg
    rc, msg, _, _ = _call(d, _field(SRC, itemsize=1), dsize=8, ssize=1, flags=_lib.COPY_CONVERT)
    assert rc == UNS and b"float32 <-> float64 only" in msg
    # strides and alignment the kernels do not take
    rc, msg, _, _ = _call(_field(DST, strides=(8, 52, 312)), s)
    assert rc == UNS and b"multiple of the item size" in msg
    rc, msg, _, _ = _call(_field(DST + 4), s)
    assert rc == UNS and b"not aligned to its item size" in msg
    # a dst stride of 0 on an axis of extent > 1 (fine on an axis of extent 1); a src stride of 0 broadcasts
    rc, msg, launches, _ = _call(_field(DST, strides=(0, 8, 48)), s)
    assert rc == INV and b"dst 0 has stride 0 along axis 0" in msg and launches == 0
    rc, msg, _, _ = _call(_field(DST, shape=(6, 6, 1), strides=(8, 48, 0)), _field(SRC, shape=(6, 6, 1)), extent=(4, 4, 1))
    assert rc == 0, msg
    rc, msg, _, paths = _call(d, _field(SRC, strides=(0, 8, 48)))
    assert rc == 0 and paths == [R.ITEMS], msg
    # overlap in memory: dst against its own src, against another pair's src, against another dst; a byte apart is fine
    rc, msg, launches, _ = _call(d, d)
    assert rc == UNS and b"dst 0 and src 0 overlap in memory" in msg and launches == 0
    first, last = 8 * (1 + 6), 8 * (4 + 6 * 4 + 36)  # byte offsets of the box's first and last item
    rc, msg, _, _ = _call(d, _field(DST + last - first))  # src's first item IS dst's last
    assert rc == UNS and b"overlap in memory" in msg
    rc, msg, _, _ = _call(d, _field(DST + last - first + 8))  # the byte ranges of the BOXES (not of the arrays) do not meet
    assert rc == 0, msg
    two = lambda a, b: E.table((a, b))  # noqa: E731
    rc, msg, _, _ = _call(two(d, _field(DST + 0x1000)), two(s, _field(DST + 64)), nfields=2)
    assert rc == UNS and b"dst 0 and src 1 overlap in memory" in msg
    rc, msg, _, _ = _call(two(d, _field(DST + 128)), two(s, _field(SRC + 0x1000)), nfields=2)
    assert rc == UNS and b"dst 0 and dst 1 overlap in memory" in msg
    rc, msg, launches, _ = _call(two(d, _field(DST + 0x1000)), two(s, s), nfields=2)  # one src for two dsts is fine
    assert rc == 0 and launches == 1, msg
    # an extent with a zero entry: OK, nothing to launch -- after the checks
    rc, msg, launches, _ = _call(d, s, extent=(4, 0, 2))
    assert rc == 0 and launches == 0, msg
    rc, msg, launches, _ = _call(d, s, extent=(7, 0, 2))
    assert rc == OOB and launches == 0
    # paths may be NULL
    rc, msg, launches, _ = _call(d, s, want_paths=False)
    assert rc == 0 and launches == 1


def test_more_items_than_a_launch_can_index_are_refused():
    n = 2**31 - 100
    d = _lib.Field.make(DST, (n, 2, 1), (1, n, 2 * n), (0, 0, 0))
    s = _lib.Field.make(DST + 2**40, (n, 2, 1), (1, n, 2 * n), (0, 0, 0))
    rc, msg, launches, _ = _call(d, s, extent=(n, 2, 1), dsize=1, ssize=1)
    assert rc == UNS and b"too many items" in msg and launches == 0


@pytest.mark.parametrize("itemsize", R.ITEMSIZES)
def test_paths_of_the_dry_run(itemsize):
    shape, extent = (40, 36, 9), (38, 34, 9)
    mk = lambda ptr, layout: _field(ptr, shape, origin=(1, 1, 0), itemsize=itemsize, layout=layout)  # noqa: E731
    for a, b in (("ifirst", "kfirst"), ("ifirst", "jfirst"), ("jfirst", "kfirst")):
        for dl, sl in ((a, b), (b, a)):
            rc, msg, _, paths = _call(mk(DST, dl), mk(SRC, sl), extent=extent, dsize=itemsize, ssize=itemsize)
            assert rc == 0 and paths == [R.TILES], (dl, sl, msg)
    for layout in ("ifirst", "kfirst", "jfirst"):
        rc, msg, _, paths = _call(mk(DST, layout), mk(SRC, layout), extent=extent, dsize=itemsize, ssize=itemsize)
        assert rc == 0 and paths == [R.ROWS], (layout, msg)
    # rows that sit differently relative to a 16-byte boundary are rows still (item by item)
    rc, msg, _, paths = _call(mk(DST, "ifirst"), mk(SRC + itemsize, "ifirst"), extent=extent, dsize=itemsize, ssize=itemsize)
    assert rc == 0 and paths == [R.ROWS], msg
    # a src broadcast along I; a side without a unit stride; an axis of extent 1 does not count as a fast axis
    bro = _lib.Field.make(SRC, shape, (0, 9 * itemsize, itemsize), (1, 1, 0))
    rc, msg, _, paths = _call(mk(DST, "ifirst"), bro, extent=extent, dsize=itemsize, ssize=itemsize)
    assert rc == 0 and paths == [R.ITEMS], msg
    every_other = _lib.Field.make(SRC, shape, (2 * itemsize, 80 * itemsize, 2880 * itemsize), (1, 1, 0))
    rc, msg, _, paths = _call(mk(DST, "ifirst"), every_other, extent=extent, dsize=itemsize, ssize=itemsize)
    assert rc == 0 and paths == [R.ITEMS], msg
    rc, msg, _, paths = _call(mk(DST, "ifirst"), mk(SRC, "kfirst"), extent=(38, 34, 1), dsize=itemsize, ssize=itemsize)
    assert rc == 0 and paths == [R.ITEMS], msg
    # the rule restated in tests/transfer_ref.py names the same paths
    items = lambda f: tuple(s // itemsize for s in f.stride)  # noqa: E731
    for dl, sl in ((a, b) for a in ("ifirst", "kfirst", "jfirst") for b in ("ifirst", "kfirst", "jfirst")):
        d, s = mk(DST, dl), mk(SRC, sl)
        for ext in (extent, (1, 1, 1), (5, 5, 1), (1, 7, 3), (7, 1, 3)):
            rc, msg, _, paths = _call(d, s, extent=ext, dsize=itemsize, ssize=itemsize)
            assert rc == 0 and paths == [R.expected_path(items(d), items(s), ext)], (dl, sl, ext, msg)


def test_a_mixed_call_reports_one_path_per_pair_and_conversion_keeps_them():
    shape, extent = (40, 36, 9), (38, 34, 9)
    layouts = [("ifirst", "kfirst"), ("kfirst", "kfirst"), ("jfirst", "ifirst")]
    for dsize, ssize, flags in ((8, 8, 0), (4, 8, _lib.COPY_CONVERT), (8, 4, _lib.COPY_CONVERT)):
        d = E.table(_field(DST + n * 0x10_0000, shape, itemsize=dsize, layout=dl) for n, (dl, _) in enumerate(layouts))
        s = E.table(_field(SRC + n * 0x10_0000, shape, itemsize=ssize, layout=sl) for n, (_, sl) in enumerate(layouts))
        rc, msg, launches, paths = _call(d, s, nfields=3, extent=extent, dsize=dsize, ssize=ssize, flags=flags)
        assert rc == 0 and launches == 1 and paths == [R.TILES, R.ROWS, R.TILES], msg


def test_launches_are_one_per_eight_pairs():
    d = E.table(_field(DST + n * 0x1000) for n in range(9))
    s = E.table(_field(SRC + n * 0x1000) for n in range(9))
    assert [_call(d, s, nfields=n)[2] for n in (1, 8, 9)] == [1, 1, 2]


def test_the_kernels_are_in_the_resource_log():
    kernels = E.kernel_resources(r"field_copy_kernel")
    assert len(kernels) == 6, kernels  # item sizes 1, 2, 4, 8 and the two conversions
    for name, scratch, waves, lds in kernels:
        # every instantiation holds the tile path: no scratch, at least 4 waves per SIMD, a tile of at most 32 KiB
        assert int(scratch) == 0 and int(waves) >= 4 and 0 < int(lds) <= 32 * 1024, (name, scratch, waves, lds)


# ---- the Python interface: every refusal before any GPU work ---------------------------------------------------------------
@pytest.mark.parametrize("kwargs, error, match", [
    (dict(halo=2.0), ValueError, "halo must be"),
    (dict(halo=(1, 2, 3)), ValueError, "halo must be"),
    (dict(halo=((1, 1.5), (1, 1))), TypeError, "halo widths must be ints"),
    (dict(halo=-1), ValueError, "must not be negative"),
    (dict(halo=5), ValueError, "leave no domain"),
    (dict(halo=2, origin=(1, 2, 0), domain=(3, 3, 3)), ValueError, "negative origin -1 along axis 0"),
    (dict(halo=2, origin=(2, 2, 0), domain=(4, 6, 3)), ValueError, "axis 1 is outside the array"),
    (dict(halo=1, domain=(4, 5, 4)), ValueError, "axis 2"),
    (dict(halo=1, origin=(1, 1, 0, 0)), ValueError, "at most three entries"),
    (dict(halo=((1, 2), (0, 3))), TypeError, "device fields"),  # all checks passed: refused for being host memory
    (dict(), TypeError, "device fields"),
])
def test_python_refusals_need_no_gpu(kwargs, error, match):
    with pytest.raises(error, match=match):
        transfer.copy_fields(E.host_field(HOST), E.host_field(HOST), **kwargs)
    with pytest.raises(error, match=match):
        transfer.FieldCopy([E.host_field(HOST)], [E.host_field(HOST)], **kwargs)
    with pytest.raises(error, match=match):
        transfer.Download([E.host_field(HOST)], **kwargs)
    with pytest.raises(error, match=match):
        transfer.Upload(E.host_field(HOST), **kwargs)


def test_python_refusals_about_the_fields_themselves():
    import torch

    T = transfer
    with pytest.raises(ValueError, match="at least one"):
        T.copy_fields([], [])
    with pytest.raises(ValueError, match="at least one"):
        T.Download([])
    with pytest.raises(ValueError, match="2 destination.s. and 1 source"):
        T.copy_fields([E.host_field(HOST), E.host_field(HOST)], [E.host_field(HOST)])
    with pytest.raises(TypeError, match="host"):
        T.copy_fields(torch.zeros(4, 4, 2), E.host_field(HOST))  # as_device_array's own refusal
    with pytest.raises(TypeError):
        T.copy_fields(E.host_field(HOST), np.zeros((4, 4, 2)))
    with pytest.raises(ValueError, match="IJ or IJK"):
        T.copy_fields(E.host_field((8,)), E.host_field((8,)))
    # dtypes: the sides of a call share one each; different ones need convert, and convert is float32 <-> float64 only
    with pytest.raises(TypeError, match="share a dtype"):
        T.copy_fields([E.host_field(HOST), E.host_field(HOST, dtype="float32")], [E.host_field(HOST), E.host_field(HOST)])
    with pytest.raises(TypeError, match="pass convert=True"):
        T.copy_fields(E.host_field(HOST, dtype="float32"), E.host_field(HOST))
    with pytest.raises(TypeError, match="pass convert=True"):
        T.copy_fields(E.host_field(HOST, dtype="int32"), E.host_field(HOST, dtype="float32"))  # the same item size is not the same dtype
    with pytest.raises(TypeError, match="only float32 <-> float64"):
        T.copy_fields(E.host_field(HOST, dtype="int32"), E.host_field(HOST), convert=True)
    with pytest.raises(TypeError, match="device fields"):
        T.copy_fields(E.host_field(HOST, dtype="float32"), E.host_field(HOST), convert=True)
    with pytest.raises(TypeError, match="only float32 <-> float64"):
        T.Download([E.host_field(HOST, dtype="int32")], dtype=np.float32)
    with pytest.raises(TypeError, match="only float32 <-> float64"):
        T.Upload([E.host_field(HOST)], dtype=np.int64)
    with pytest.raises(ValueError, match="slots"):
        T.Download([E.host_field(HOST)], slots=0)
    # the common domain is what fits EVERY field; a stated one that does not fit is the library's refusal
    with pytest.raises(ValueError, match="src 0: origin 0 . extent 8 along axis 0 is outside the array .shape 7."):
        T.copy_fields(E.host_field(HOST), E.host_field((7, 9, 3)), domain=(8, 9, 3))
    with pytest.raises(TypeError, match="device fields"):
        T.copy_fields(E.host_field(HOST), E.host_field((7, 9, 3)))
    # a field onto itself
    x = E.host_field(HOST)
    with pytest.raises(TypeError, match="overlap in memory"):
        T.copy_fields(x, x)


def test_a_frozen_copy_refuses_to_run_after_an_array_died(monkeypatch):
    """The weak references are taken last, behind the device check: what they guard is shown on a FieldCopy whose device check
    is made to pass for host memory -- the call itself is never reached, the dead reference is found first."""
    E.on_device(monkeypatch)
    a, b = E.host_field(HOST), E.host_field(HOST)
    cp = transfer.FieldCopy([a], [b], halo=1)
    assert cp.launches == 1 and cp.paths == [transfer.PATH_ROWS] and cp.extent == (8, 9, 3) and cp.domain == (6, 7, 3)
    del b
    E.refuses_a_dead_array(cp)


# ---- the layouts every GPU test of a utility entry puts its buffers in -------------------------------------------------------------
def test_the_geometry_of_the_four_layouts():
    """tests/device_layouts.py's ``geometry``: every item of the view inside the flat buffer and at an address of its own, the
    column ``align_i`` of an "ifirst" row on a 256-byte address, an "ifirst_unaligned" view on an odd item address with an odd
    pitch -- wherever the allocation starts."""
    base = 0x7F00_0000_0000  # (a multiple of 256 bytes, as allocations are; the sweep below moves off it)
    cases = 0
    for layout in L.LAYOUTS:
        for itemsize in (1, 2, 4, 8):
            for align_i in (0, 1, 3):
                for shape in ((1, 1, 1), (3, 5, 2), (65, 63, 7)):
                    numel, strides, offset_of = L.geometry(shape, layout, itemsize, align_i)
                    index = sum(np.arange(n).reshape([-1 if a == ax else 1 for a in range(3)]) * strides[ax] for ax, n in enumerate(shape))
                    rows = index[0]  # (the first item of every row)
                    for k in (0, 1, 2, 7, 31, 100, 255):  # ptr // itemsize of both parities, 7 residues modulo 256 bytes
                        ptr = base + k * itemsize
                        offset = offset_of(ptr)
                        what = (layout, itemsize, align_i, shape, k)
                        assert 0 <= offset and offset + int(index.max()) < numel, what
                        assert np.unique(index).size == index.size, what
                        if layout == "ifirst":
                            assert ((ptr + (offset + align_i + rows) * itemsize) % 256 == 0).all(), what
                        if layout == "ifirst_unaligned":
                            assert (ptr // itemsize + offset) % 2 == 1 and strides[1] % 2 == 1, what
                        cases += 1
    assert cases == 4 * 4 * 3 * 3 * 7


# ---- numpy's own two conversions on the values the GPU test plants ----------------------------------------------------------
def test_numpy_conversions_agree_with_the_expectations_of_the_planted_values():
    src64, src32 = R.conversion_inputs()
    for src in (src64, src32):
        assert np.isnan(src).mean() <= 0.01
    with np.errstate(over="ignore", under="ignore"):
        narrow = src64.astype(np.float32)
    wide = src32.astype(np.float64)
    f32 = np.finfo(np.float32)
    for value, want in R.NARROWING_EXPECTATIONS:
        with np.errstate(over="ignore", under="ignore"):
            got = np.float64(value).astype(np.float32)
        assert got.view(np.uint32) == np.float32(want).view(np.uint32), (float(value).hex(), float(got).hex(), float(want).hex())
        hit = src64.view(np.uint64) == np.float64(value).view(np.uint64)
        assert hit.any() and (narrow[hit].view(np.uint32) == np.float32(want).view(np.uint32)).all(), float(value).hex()
    # widening is exact: back to float32 gives the same bits, subnormals and signed zeros included (NaNs aside)
    back = wide.astype(np.float32)
    keep = ~np.isnan(src32)
    assert np.array_equal(back.view(np.uint32)[keep], src32.view(np.uint32)[keep])
    assert np.array_equal(np.signbit(wide), np.signbit(src32)) and np.array_equal(np.isnan(wide), np.isnan(src32))
    # the planted classes are all there
    assert (np.isinf(narrow) & np.isfinite(src64)).sum() >= 4  # overflow to +-inf
    assert ((narrow == 0) & (src64 != 0)).sum() >= 2  # underflow to +-0
    assert ((np.abs(narrow) < f32.tiny) & (narrow != 0)).sum() >= 4  # float32 subnormals
    assert (np.signbit(src64) & (src64 == 0)).sum() >= 1 and (np.signbit(src32) & (src32 == 0)).sum() >= 1
