"""``gt4py_amd.transfer`` on the GPU: the layout-converting copy against numpy slicing on host images of the FLAT buffers
(tests/transfer_ref.py), EVERY BYTE of the destination buffer -- row padding, ghost cells outside the box and the allocation's
slack keep a NaN-payload sentinel --, conversion at IEEE edge values, position in a launch of nine pairs, ``Download`` / ``Upload``
and stream capture.

Wall time of this file on one MI355X: not recorded yet (1 152 grid copies among them)."""

import ctypes
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import device_layouts as L  # noqa: E402  (the layouts; test infrastructure)
import transfer_ref as R  # noqa: E402
from oracle import ref_numpy as ORACLE  # noqa: E402  (oracle = checker only)

HALOS = [0, 2]


def _case(src_layout, dst_layout, itemsize, halo, domain, rng):
    """One copy of the grid: returns the path taken."""
    from gt4py_amd import transfer

    # one more ghost cell than the halo on every I / J side: outside the box, it must stay as it is
    origin = (halo + 1, halo + 1, 0)
    shape = (domain[0] + 2 * halo + 2, domain[1] + 2 * halo + 2, domain[2])
    src, dst = L.Layout(shape, src_layout, itemsize, origin[0]), L.Layout(shape, dst_layout, itemsize, origin[0])
    src_image = L.random_image(src.flat.numel(), itemsize, rng)
    want = L.sentinel_image(dst.flat.numel(), itemsize)
    src.upload(src_image)
    dst.upload(want)
    cp = transfer.FieldCopy(dst.view, src.view, halo=halo, origin=origin, domain=domain)
    extent = (domain[0] + 2 * halo, domain[1] + 2 * halo, domain[2])
    assert cp.extent == extent and cp.launches == 1
    expected = R.expected_path(dst.strides, src.strides, extent)
    assert cp.paths == [expected], (src_layout, dst_layout, itemsize, halo, domain, cp.paths, expected)
    cp()
    got = dst.download()
    R.copy_box(dst.host_view(want), src.host_view(src_image), (1, 1, 0), (1, 1, 0), extent)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{src_layout} -> {dst_layout} item size {itemsize} halo {halo} domain {domain} "
                             f"(path {transfer.PATH_NAMES[expected]}): {bad.size} items of the whole buffer differ, first at flat "
                             f"index {bad[:6].tolist()} (view offset {dst.offset}, strides {dst.strides}); got {got[bad[:6]].tolist()}, "
                             f"want {want[bad[:6]].tolist()}")
    assert np.array_equal(src.download(), src_image), "the source changed"
    return expected


@pytest.mark.parametrize("domain", L.DOMAINS + R.K_LONG)
def test_copy_grid(domain):
    rng = np.random.default_rng(sum(domain))
    taken = {R.ROWS: 0, R.TILES: 0, R.ITEMS: 0}
    for src_layout, dst_layout, itemsize, halo in itertools.product(L.LAYOUTS, L.LAYOUTS, R.ITEMSIZES, HALOS):
        taken[_case(src_layout, dst_layout, itemsize, halo, domain, rng)] += 1
    assert sum(taken.values()) == 16 * 4 * 2
    # the tile path cannot go unexercised behind the item path: of the 16 pairs of layouts 10 differ in their fast axis
    # (ifirst and ifirst_unaligned share theirs), 6 do not.  A box of extent 1 along a side's fast axis has no fast axis there.
    if min(domain) > 1:
        assert taken == {R.ROWS: 6 * 8, R.TILES: 10 * 8, R.ITEMS: 0}, taken
    else:
        assert domain == (1, 1, 1) and taken[R.ITEMS] > 0


def test_grid_size():
    assert len(L.DOMAINS + R.K_LONG) * len(L.LAYOUTS) ** 2 * len(R.ITEMSIZES) * len(HALOS) == 9 * 16 * 4 * 2 == 1152


def test_nine_pairs_of_mixed_layouts_are_two_launches_and_equal_nine_single_calls():
    """Position in the launch: every pair of a call of nine lands where a call of its own puts it."""
    from gt4py_amd import transfer

    domain, halo, itemsize = (65, 33, 5), 1, 4
    extent = (67, 35, 5)
    pairs = [("ifirst", "kfirst"), ("kfirst", "ifirst"), ("ifirst", "ifirst"), ("jfirst", "ifirst_unaligned"), ("kfirst", "jfirst"),
             ("ifirst_unaligned", "ifirst"), ("kfirst", "kfirst"), ("ifirst", "jfirst"), ("ifirst_unaligned", "kfirst")]
    rng = np.random.default_rng(23)
    origin = (2, 2, 0)
    srcs, dsts, images, singles = [], [], [], []
    for n, (sl, dl) in enumerate(pairs):
        # arrays of different shapes around the one box
        s_shape = (extent[0] + 2 + n % 3, extent[1] + 2 + n % 2, extent[2])
        d_shape = (extent[0] + 2 + (n + 1) % 3, extent[1] + 3, extent[2])
        src, dst, alone = L.Layout(s_shape, sl, itemsize, origin[0]), L.Layout(d_shape, dl, itemsize, origin[0]), L.Layout(d_shape, dl, itemsize, origin[0])
        image = L.random_image(src.flat.numel(), itemsize, rng)
        src.upload(image)
        for d in (dst, alone):
            d.upload(L.sentinel_image(d.flat.numel(), itemsize))
        transfer.copy_fields(alone.view, src.view, halo=halo, origin=origin, domain=domain)
        srcs.append(src), dsts.append(dst), images.append(image), singles.append(alone)
    cp = transfer.FieldCopy([d.view for d in dsts], [s.view for s in srcs], halo=halo, origin=origin, domain=domain)
    assert cp.launches == 2 and cp.extent == extent
    assert cp.paths == [R.expected_path(d.strides, s.strides, extent) for d, s in zip(dsts, srcs)]
    assert sorted(set(cp.paths)) == [R.ROWS, R.TILES]
    cp()
    for n, (src, dst, alone, image) in enumerate(zip(srcs, dsts, singles, images)):
        got = dst.download()
        want = L.sentinel_image(dst.flat.numel(), itemsize)
        R.copy_box(dst.host_view(want), src.host_view(image), (1, 1, 0), (1, 1, 0), extent)
        assert np.array_equal(got, want), f"pair {n} {pairs[n]}: {int((got != want).sum())} items of the whole buffer differ"
        # (the two buffers may sit differently in memory: compared through their views and their slack separately)
        assert np.array_equal(dst.host_view(got), alone.host_view(alone.download())), f"pair {n} differs from its single call"


def test_a_broadcast_source_and_a_strided_side_take_the_item_path():
    import torch

    from gt4py_amd import transfer

    rng = np.random.default_rng(4)
    plane = torch.from_numpy(rng.uniform(-1, 1, (1, 37, 9))).cuda()
    dst = L.Layout((21, 37, 9), "ifirst", 8)
    dst.upload(L.sentinel_image(dst.flat.numel(), 8))
    view = dst.view.view(torch.float64)
    everywhere = plane.expand(21, 37, 9)  # (held: the frozen copy keeps weak references to what the caller passes)
    cp = transfer.FieldCopy(view, everywhere)
    assert cp.paths == [R.ITEMS]
    cp()
    want = L.sentinel_image(dst.flat.numel(), 8)
    dst.host_view(want.view(np.float64))[...] = plane.cpu().numpy()
    assert np.array_equal(dst.download(), want)
    # every other column of a wider array, on both sides
    wide_s, wide_d = torch.from_numpy(rng.uniform(-1, 1, (40, 12, 6))).cuda(), torch.zeros(40, 12, 6, dtype=torch.float64, device="cuda")
    some_d, some_s = wide_d[::2, :, ::2], wide_s[::2, :, ::2]
    cp = transfer.FieldCopy(some_d, some_s)
    assert cp.paths == [R.ITEMS]
    cp()
    want = np.zeros((40, 12, 6))
    want[::2, :, ::2] = wide_s.cpu().numpy()[::2, :, ::2]
    assert np.array_equal(wide_d.cpu().numpy().view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("layouts", [("ifirst", "kfirst"), ("kfirst", "ifirst"), ("ifirst", "ifirst"), ("jfirst", "ifirst_unaligned")])
def test_conversion_at_ieee_edge_values(layouts):
    """float64 -> float32 is ONE rounding to nearest even, float32 -> float64 exact: bit-equal to ``numpy.astype`` wherever the
    expected value is not NaN; there a NaN of the same sign (tests/test_transfer.py confirms numpy's conversions on this input)."""
    import torch

    from gt4py_amd import transfer

    src64, src32 = R.conversion_inputs()
    for host, to in ((src64, np.float32), (src32, np.float64)):
        assert np.isnan(host).mean() <= 0.01
        shape = host.shape
        isz, osz = host.dtype.itemsize, np.dtype(to).itemsize
        src, dst = L.Layout(shape, layouts[0], isz), L.Layout(shape, layouts[1], osz)
        image = L.random_image(src.flat.numel(), isz, np.random.default_rng(1))
        src.host_view(image.view(host.dtype))[...] = host
        src.upload(image)
        dst.upload(L.sentinel_image(dst.flat.numel(), osz))
        tf = {4: torch.float32, 8: torch.float64}
        d_view, s_view = dst.view.view(tf[osz]), src.view.view(tf[isz])
        with pytest.raises(TypeError, match="convert=True"):
            transfer.copy_fields(d_view, s_view)
        cp = transfer.FieldCopy(d_view, s_view, convert=True)
        assert cp.paths == [R.expected_path(dst.strides, src.strides, shape)]
        cp()
        got_flat = dst.download()
        with np.errstate(over="ignore", under="ignore"):
            expected = host.astype(to)
        got = dst.host_view(got_flat.view(to))
        ut = L.NP_UINT[osz]
        nan = np.isnan(expected)
        assert nan.mean() <= 0.01
        differ = ~nan & (np.ascontiguousarray(got).view(ut) != expected.view(ut))
        assert not differ.any(), (f"{host.dtype} -> {np.dtype(to)} {layouts}: {int(differ.sum())} items differ from numpy.astype, first "
                                  f"{[(float(host[tuple(i)]).hex(), float(got[tuple(i)]).hex(), float(expected[tuple(i)]).hex()) for i in np.argwhere(differ)[:4]]}")
        assert np.isnan(got[nan]).all() and np.array_equal(np.signbit(got[nan]), np.signbit(expected[nan]))
        # and nothing outside the view was written
        want_flat = L.sentinel_image(dst.flat.numel(), osz)
        dst.host_view(want_flat)[...] = dst.host_view(got_flat)
        assert np.array_equal(got_flat, want_flat)


# ---- Download / Upload ---------------------------------------------------------------------------------------------------------
def _storage(host, aligned_index=(2, 2, 0)):
    import gt4py_amd.storage as gt_storage

    return gt_storage.from_array(host, host.dtype, backend="hip:mi300", aligned_index=aligned_index)


@pytest.mark.parametrize("dtype", [None, np.float32])
@pytest.mark.parametrize("halo", [0, 2])
def test_download_of_a_storage(halo, dtype):
    from gt4py_amd import transfer

    rng = np.random.default_rng(8)
    hosts = [rng.uniform(-1, 1, (37, 22, 9)), rng.uniform(-1, 1, (37, 22, 9))]
    fields = [_storage(h) for h in hosts]
    out = transfer.Download(fields, halo=halo, dtype=dtype, origin=(2, 2, 0), domain=(33, 18, 9))
    assert out.launches == 1 and out.paths == [transfer.PATH_TILES] * 2  # I-contiguous storage -> C order
    handle = out()
    arrays = handle.get()
    box = (slice(2 - halo, 35 + halo), slice(2 - halo, 20 + halo), slice(None))
    assert len(arrays) == 2
    for a, h in zip(arrays, hosts):
        want = np.ascontiguousarray(h[box]) if dtype is None else h[box].astype(dtype)
        assert a.dtype == want.dtype and a.shape == want.shape and a.flags["C_CONTIGUOUS"]
        assert np.array_equal(a.view(L.NP_UINT[a.itemsize]), want.view(L.NP_UINT[a.itemsize]))
        pinned = out._host_stage[handle._slot]
        assert pinned.is_pinned() and np.shares_memory(a, pinned.numpy())
    assert handle.done()


def test_two_downloads_in_flight_return_their_own_data():
    import torch

    from gt4py_amd import transfer

    rng = np.random.default_rng(9)
    first, second, third = (rng.uniform(-1, 1, (20, 12, 5)) for _ in range(3))
    u = _storage(first, (0, 0, 0))
    out = transfer.Download([u], slots=2)
    h1 = out()
    u[...] = second  # stream-ordered behind the first transfer
    h2 = out()
    u[...] = third
    a2, = h2.get()
    a1, = h1.get()
    assert np.array_equal(a1, first) and np.array_equal(a2, second)
    assert not np.shares_memory(a1, a2)
    # the third call takes the first slot again: the views of h1 now show the third field, and h1 refuses to be read
    h3 = out()
    a3, = h3.get()
    assert np.array_equal(a3, third) and np.shares_memory(a3, a1)
    with pytest.raises(RuntimeError, match="slot has been reused"):
        h1.get()
    assert np.array_equal(h2.get()[0], second)
    # a slot whose handle was never read: the call that takes the slot again waits for that transfer's event first, and the
    # unread handle refuses to be read afterwards -- it is never torn
    h4 = out()  # slot of h2
    h5 = out()  # slot of h3
    h6 = out()  # slot of h4, which nobody read
    with pytest.raises(RuntimeError, match="slot has been reused"):
        h4.get()
    assert np.array_equal(h5.get()[0], third) and np.array_equal(h6.get()[0], third)
    torch.cuda.synchronize()


def test_upload_writes_the_box_and_nothing_else():
    import torch

    import fullsize_util as F
    from gt4py_amd import transfer

    rng = np.random.default_rng(10)
    for dtype, host_dtype in ((np.float64, None), (np.float32, None), (np.float64, np.float32)):
        isz = np.dtype(dtype).itemsize
        tint = {4: torch.int32, 8: torch.int64}[isz]
        u = _storage(np.zeros((37, 22, 9), dtype))
        F.fill_sentinel(u.tensor)
        want = F.padded(u.tensor).view(tint).clone()  # the whole allocation behind the array, row padding included
        up = transfer.Upload([u], halo=1, dtype=host_dtype, origin=(2, 2, 0), domain=(33, 18, 9))
        assert up.paths == [transfer.PATH_TILES] and up.shapes == [(35, 20, 9)]
        host = rng.uniform(-1, 1, (35, 20, 9)).astype(host_dtype or dtype)
        with pytest.raises(ValueError, match="shape"):
            up([host[1:]])
        with pytest.raises(TypeError, match="dtype"):
            up([host.astype(np.float16)])
        with pytest.raises(ValueError, match="1 field"):
            up([host, host])
        up([host])
        kept = host.copy()
        host[...] = 0  # the pinned slot has its own copy
        whole = u.get()
        assert whole.shape == (37, 22, 9)
        inside = np.zeros(whole.shape, bool)
        inside[1:36, 1:21] = True
        ut = L.NP_UINT[isz]
        assert np.array_equal(whole[1:36, 1:21].view(ut), kept.astype(dtype).view(ut))
        assert (whole.view(ut)[~inside] == ut(F.SENTINEL_BITS[isz])).all()
        # every other byte: ghost cells outside the box and the row padding keep the sentinel
        bits = torch.from_numpy(np.ascontiguousarray(kept.astype(dtype)).view({4: np.int32, 8: np.int64}[isz])).cuda()
        want[1:36, 1:21, :] = bits
        assert torch.equal(F.padded(u.tensor).view(tint), want)
        # a second upload goes through the second slot
        again = rng.uniform(-1, 1, (35, 20, 9)).astype(host_dtype or dtype)
        up([again])
        assert np.array_equal(u.get()[1:36, 1:21], again.astype(dtype))


def test_upload_stencil_download_round_trip_equals_the_oracle():
    import gt4py_amd.storage as gt_storage
    from gt4py_amd import transfer
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates

    backend = "hip:mi300"
    rng = np.random.default_rng(77)
    shape = (68, 68, 8)
    u = rng.uniform(-10, 10, shape).astype(np.float32)
    c = rng.uniform(0, 0.5, shape).astype(np.float32)
    d_u, d_c, d_o = (gt_storage.zeros(shape, np.float32, backend=backend, aligned_index=(2, 2, 0)) for _ in range(3))
    up = transfer.Upload([d_u, d_c], halo=2)
    hd = gtscript.stencil(backend=backend, definition=hip_templates.hdiff_limiter_field, dtypes={"T": np.float32})
    up([u, c])
    hd(d_u, d_o, d_c, origin=(2, 2, 0))
    down = transfer.Download([d_o], origin=(2, 2, 0), domain=(64, 64, 8))
    got, = down().get()
    want = np.zeros_like(u)
    ORACLE.hdiff(u, want, c)
    assert got.shape == (64, 64, 8)
    assert np.array_equal(got.view(np.uint32), want[2:-2, 2:-2].view(np.uint32))


def test_one_capture_of_a_frozen_copy_replays_the_same_bits():
    """A single stream, one capture, one replay, no parallel branches: the call neither synchronises nor allocates."""
    import torch

    from gt4py_amd import transfer

    rng = np.random.default_rng(12)
    shape = (70, 35, 9)
    src, dst = L.Layout(shape, "ifirst", 8, 1), L.Layout(shape, "kfirst", 8)
    first, second = L.random_image(src.flat.numel(), 8, rng), L.random_image(src.flat.numel(), 8, rng)
    sentinel = L.sentinel_image(dst.flat.numel(), 8)
    cp = transfer.FieldCopy(dst.view, src.view, halo=1)
    assert cp.paths == [R.TILES] and cp.extent == shape
    graph = torch.cuda.CUDAGraph()
    src.upload(first)
    dst.upload(sentinel)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        cp()
    src.upload(second)
    dst.upload(sentinel)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    want = sentinel.copy()
    R.copy_box(dst.host_view(want), src.host_view(second), (0, 0, 0), (0, 0, 0), shape)
    assert np.array_equal(dst.download(), want)


def test_the_c_entry_counts_what_it_enqueued():
    import torch

    from gt4py_amd import _lib, transfer

    src, dst = L.Layout((33, 9, 4), "jfirst", 2), L.Layout((33, 9, 4), "ifirst", 2)
    cp = transfer.FieldCopy(dst.view, src.view)
    launches, paths = ctypes.c_int(-1), (ctypes.c_int * 1)(-1)
    rc = _lib.load().gt4mi_field_copy(cp._dst, cp._src, 1, cp._extent3, 2, 2, 0, torch.cuda.current_stream().cuda_stream, paths,
                                      ctypes.byref(launches))
    torch.cuda.synchronize()
    assert rc == 0 and launches.value == 1 and list(paths) == [R.TILES]
