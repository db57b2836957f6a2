"""``gt4py_amd.boundary`` on the GPU: the single-launch halo fill against the contract's numpy restatement
(tests/boundary_ref.py), BIT PATTERNS OF THE WHOLE ARRAY -- row padding, ghost cells beyond the widths and the allocation's
slack included --, on arrays pre-filled with a NaN sentinel outside the domain.

Wall time of this file on one MI355X: 6 s (41 100 grid cases among them), measured together with tests/test_boundary.py."""

import gc
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import boundary_ref as R  # noqa: E402
import device_layouts as L  # noqa: E402  (the layouts; test infrastructure)
from oracle import ref_numpy as ORACLE  # noqa: E402  (oracle = checker only)

WIDTHS = [(1, 1, 1, 1), (2, 2, 2, 2), (2, 3, 0, 2)]
ITEMSIZES = [1, 4, 8]
#: all four; one side; the high sides; J sides only (over I ghosts the caller filled: the corner rule's last branch); a channel's
SIDE_MASKS = [R.ALL, R.I_LO, R.I_HI | R.J_HI, R.J_LO | R.J_HI, R.I_LO | R.I_HI]
MODE_PAIRS = R.mode_pairs(with_none=True)  # 6 x 6
# Of the 3 x 36 (widths, modes) combinations per domain the width rule (PERIODIC / SYMMETRIC <= n, REFLECT <= n - 1) admits
# all but, counted by hand from the rule:
#   (1, 1, 1)  per axis REFLECT never fits, PERIODIC / SYMMETRIC only width 1: 5 x 5 pairs for (1, 1, 1, 1), 3 x 3 for the others;
#   (3, 5, 2)  REFLECT in I does not take the high I width 3 of (2, 3, 0, 2): 36 - 6 there.
# Each runs on 4 layouts x 3 item sizes x 5 side masks.
ADMISSIBLE = {(1, 1, 1): 25 + 9 + 9, (3, 5, 2): 36 + 36 + 30}
CONSTANT = {1: 0x3C, 4: 0x7FC1_2345, 8: 0x7FF8_0000_0BAD_F00D}  # NaNs with payload as integers


def _initial(lay, itemsize, origin, domain, rng):
    """Host image of the flat buffer: the sentinel everywhere, random bits in the domain box."""
    host = L.sentinel_image(lay.flat.numel(), itemsize)
    box = tuple(slice(o, o + d) for o, d in zip(origin, domain))
    info = np.iinfo(L.NP_INT[itemsize])
    lay.host_view(host)[box] = rng.integers(info.min, info.max, size=domain, dtype=L.NP_INT[itemsize], endpoint=True)
    return host


def _grid_case(domain, layout):
    import torch

    from gt4py_amd import boundary
    from gt4py_amd.storage.device_array import DeviceArray

    rng = np.random.default_rng(sum(domain) * 4 + L.LAYOUTS.index(layout))
    ran = refused = 0
    for widths, itemsize in itertools.product(WIDTHS, ITEMSIZES):
        origin = (widths[0] + 1, widths[2] + 1, 0)  # one ghost cell beyond the widths: it must stay as it is
        shape = (origin[0] + domain[0] + widths[1] + 1, origin[1] + domain[1] + widths[3] + 1, domain[2])
        lay = L.Layout(shape, layout, itemsize, origin[0])
        initial = _initial(lay, itemsize, origin, domain, rng)
        pristine = torch.from_numpy(initial).cuda()
        arr = DeviceArray(lay.view)
        value = np.array(CONSTANT[itemsize], dtype=L.NP_UINT[itemsize]).view(L.NP_INT[itemsize])[()]
        halo = ((widths[0], widths[1]), (widths[2], widths[3]))
        for modes, sides in itertools.product(MODE_PAIRS, SIDE_MASKS):
            kwargs = dict(halo=halo, mode=modes, origin=origin, domain=domain, value=value, sides=sides)
            if not R.admissible(modes, widths, domain):
                with pytest.raises(ValueError, match="is larger than"):
                    boundary.fill_halo(arr, **kwargs)
                refused += 1
                continue
            lay.flat.copy_(pristine)
            boundary.fill_halo(arr, **kwargs)
            got = lay.flat.cpu().numpy()
            want = initial.copy()
            R.fill(lay.host_view(want), origin, domain, widths, modes, value, sides)
            if not np.array_equal(got, want):
                bad = np.flatnonzero(got != want)
                raise AssertionError(f"{domain} {layout} item size {itemsize} widths {widths} modes {modes} sides {sides}: "
                                     f"{bad.size} items differ, first at flat index {bad[:6].tolist()} (view offset {lay.offset}, "
                                     f"strides {lay.strides}); got {got[bad[:6]].tolist()}, want {want[bad[:6]].tolist()}")
            ran += 1
    return ran, refused


def _admissible_count(domain):
    return ADMISSIBLE.get(domain, len(WIDTHS) * len(MODE_PAIRS))


@pytest.mark.parametrize("layout", L.LAYOUTS)
@pytest.mark.parametrize("domain", L.DOMAINS)
def test_fill_grid(domain, layout):
    ran, refused = _grid_case(domain, layout)
    per = len(ITEMSIZES) * len(SIDE_MASKS)
    total = len(WIDTHS) * len(MODE_PAIRS) * per
    # the grid cannot shrink unnoticed: what the width rule forbids RAISED, everything else ran and was compared
    assert ran == _admissible_count(domain) * per and ran + refused == total, (ran, refused)


def test_grid_size():
    assert sum(_admissible_count(d) for d in L.DOMAINS) * len(L.LAYOUTS) * len(ITEMSIZES) * len(SIDE_MASKS) == (43 + 102 + 5 * 108) * 4 * 3 * 5 == 41100


def test_special_values_survive_as_bit_patterns():
    """+-0.0, NaNs with payload (quiet and signalling) and infinities on the edges of the domain, compared as integers."""
    import torch

    import gt4py_amd.storage as gt_storage
    from gt4py_amd import boundary

    for dtype, bits in ((np.float64, [0x0, 0x8000_0000_0000_0000, 0x7FF8_0000_0000_0001, 0xFFF8_0000_DEAD_BEEF, 0x7FF0_0000_0000_0001,
                                      0x7FF0_0000_0000_0000, 0xFFF0_0000_0000_0000, 0x1]),
                        (np.float32, [0x0, 0x8000_0000, 0x7FC0_0001, 0xFFC0_BEEF, 0x7F80_0001, 0x7F80_0000, 0xFF80_0000, 0x1])):
        u = np.dtype(dtype).itemsize
        utype = {4: np.uint32, 8: np.uint64}[u]
        host = np.resize(np.array(bits, dtype=utype), (12, 10, 3)).copy()  # every special value on every edge, cyclically
        host[0:2] = host[-2:] = L.SENTINEL[u]
        host[:, 0:2] = host[:, -2:] = L.SENTINEL[u]
        for modes in (("periodic", "symmetric"), ("reflect", "zero_gradient"), ("constant", "periodic")):
            d = gt_storage.empty(host.shape, dtype, backend="hip:mi300", aligned_index=(2, 2, 0))
            d.tensor.view({4: torch.int32, 8: torch.int64}[u]).copy_(torch.from_numpy(host.view({4: np.int32, 8: np.int64}[u])))
            value = np.array(bits[3], dtype=utype).view(dtype)[()]  # a negative NaN with a payload
            boundary.fill_halo(d, halo=2, mode=modes, value=value)
            got = d.tensor.view({4: torch.int32, 8: torch.int64}[u]).cpu().numpy().view(utype)
            want = host.copy()
            R.fill(want, (2, 2, 0), (8, 6, 3), (2, 2, 2, 2), modes, np.array(bits[3], dtype=utype)[()])
            assert np.array_equal(got, want), (dtype, modes)


def test_plain_torch_tensors_are_fields_too():
    """Anything ``as_device_array`` accepts: the wrapper it makes for a torch tensor lives only inside the constructor, so the
    frozen call is bound to the TENSOR the caller holds -- it runs while that lives and refuses once it is gone."""
    import torch

    from gt4py_amd import boundary

    rng = np.random.default_rng(5)
    host = rng.uniform(-1, 1, (14, 11, 3))
    widths, modes = (2, 1, 1, 2), ("reflect", "periodic")
    halo = ((2, 1), (1, 2))
    want = host.copy()
    R.fill(want, (2, 1, 0), (11, 8, 3), widths, modes)
    t = torch.from_numpy(host).cuda()
    boundary.fill_halo(t, halo=halo, mode=modes)
    assert np.array_equal(t.cpu().numpy().view(np.uint64), want.view(np.uint64))
    u, v = torch.from_numpy(host).cuda(), torch.from_numpy(host).cuda().permute(2, 1, 0).contiguous().permute(2, 1, 0)  # I-contiguous
    bc = boundary.HaloFill([u, v], halo=halo, mode=modes)
    gc.collect()
    bc()
    bc()  # (idempotent: the domain is never written)
    assert bc.launches == 1
    for x in (u, v):
        assert np.array_equal(x.cpu().numpy().view(np.uint64), want.view(np.uint64))
    del v, x
    gc.collect()
    with pytest.raises(RuntimeError, match="no longer exists"):
        bc()


def test_nine_fields_of_mixed_lanes_are_two_launches():
    """More than 8 fields: a second chunk; and chunks that mix fields on 16-byte lanes with fields on item lanes (unaligned
    rows, K-contiguous), whose J sections need different numbers of blocks of the one grid."""
    import torch

    from gt4py_amd import boundary
    from gt4py_amd.storage.device_array import DeviceArray

    domain, widths, modes = (65, 33, 5), (2, 3, 1, 2), ("symmetric", "periodic")
    origin = (3, 2, 0)
    shape = (origin[0] + domain[0] + widths[1] + 1, origin[1] + domain[1] + widths[3] + 1, domain[2])
    layouts = ["ifirst", "ifirst", "ifirst_unaligned", "ifirst", "kfirst", "ifirst", "ifirst", "ifirst", "ifirst_unaligned"]
    rng = np.random.default_rng(17)
    lays = [L.Layout(shape, name, 4, origin[0]) for name in layouts]
    initial = [_initial(lay, 4, origin, domain, rng) for lay in lays]
    for lay, host in zip(lays, initial):
        lay.flat.copy_(torch.from_numpy(host).cuda())
    arrays = [DeviceArray(lay.view) for lay in lays]
    bc = boundary.HaloFill(arrays, halo=((2, 3), (1, 2)), mode=modes, origin=origin, domain=domain)
    assert bc.launches == 2
    bc()
    for n, (lay, host) in enumerate(zip(lays, initial)):
        want = host.copy()
        R.fill(lay.host_view(want), origin, domain, widths, modes)
        got = lay.flat.cpu().numpy()
        assert np.array_equal(got, want), f"field {n} ({layouts[n]}): {int((got != want).sum())} items of the whole buffer differ"


def test_bool_and_field_ij():
    import torch

    from gt4py_amd import boundary
    from gt4py_amd.storage.device_array import DeviceArray

    rng = np.random.default_rng(3)
    host = rng.integers(0, 2, (9, 11)).astype(bool)
    d = DeviceArray(torch.from_numpy(host).cuda())  # Field[IJ]: no K axis
    boundary.fill_halo(d, halo=((1, 2), (3, 0)), mode=("symmetric", "periodic"))
    want = host.copy()[:, :, None]
    R.fill(want, (1, 3, 0), (6, 8, 1), (1, 2, 3, 0), ("symmetric", "periodic"))
    assert np.array_equal(d.get(), want[:, :, 0])
    mask = DeviceArray(torch.from_numpy(host).cuda())
    boundary.fill_halo(mask, halo=1, mode="constant", value=True)
    want = host.copy()
    want[0] = want[-1] = True
    want[:, 0] = want[:, -1] = True
    assert np.array_equal(mask.get(), want)


# ---- full size: fields from gt_storage.empty, the restatement run ON THE DEVICE through the same slice assignments -----------
def _full_size(shape, dtype, aligned_index, width, modes, nfields=1):
    import torch

    import fullsize_util as F
    import gt4py_amd.storage as gt_storage
    from gt4py_amd import boundary

    origin = (width, width, 0)
    domain = (shape[0] - 2 * width, shape[1] - 2 * width, shape[2])
    gen = torch.Generator(device="cuda").manual_seed(99)
    tint = {4: torch.int32, 8: torch.int64}[np.dtype(dtype).itemsize]
    fields, wants = [], []
    for _ in range(nfields):
        d = gt_storage.empty(shape, dtype, backend="hip:mi300", aligned_index=aligned_index)
        F.fill_sentinel(d.tensor)
        F.fill_uniform(d.tensor[width:-width, width:-width], gen, -1.0, 1.0)
        whole = F.padded(d.tensor)
        want = whole.clone()  # (padded() of an I-contiguous storage is dense: the clone keeps its layout)
        assert want.stride() == whole.stride()
        # the restatement's slice assignments on the clone's view of the same elements
        R.fill(want[: shape[0], : shape[1]].view(tint), origin, domain, (width,) * 4, modes)
        fields.append(d)
        wants.append(want)
    bc = boundary.HaloFill(fields, halo=width, mode=modes)
    bc()
    torch.cuda.synchronize()
    for n, (d, want) in enumerate(zip(fields, wants)):
        got = F.padded(d.tensor)
        assert got.shape == want.shape
        differ = int((got.view(tint) != want.view(tint)).sum().item())
        assert differ == 0, f"field {n}: {differ} items of the whole array differ from the restatement"
        # and the restatement did fill something: no sentinel left in the ring, on any of its four sides
        t = d.tensor.view(tint)
        for ring in (t[:width], t[-width:], t[:, :width], t[:, -width:]):
            assert int((ring == F.SENTINEL_BITS[np.dtype(dtype).itemsize]).sum().item()) == 0
    return bc


def test_full_size_hdiff_field():
    bc = _full_size((1028, 1028, 80), np.float32, (2, 2, 0), 2, ("periodic", "zero_gradient"))
    assert bc.launches == 1


def test_full_size_headline_field():
    bc = _full_size((514, 514, 512), np.float64, (1, 1, 0), 1, ("periodic", "periodic"))
    assert bc.launches == 1


def test_full_size_batch_of_eight_is_one_launch():
    bc = _full_size((514, 514, 128), np.float64, (1, 1, 0), 1, ("zero_gradient", "periodic"), nfields=8)
    assert bc.launches == 1
    # and through the C entry's own count of what it enqueued
    import ctypes

    import torch

    from gt4py_amd import _lib

    launches = ctypes.c_int(-1)
    rc = _lib.load().gt4mi_halo_fill(bc._fields, 8, bc._domain3, bc._halo4, bc._modes[0], bc._modes[1], bc._sides, bc._value, 8,
                                     torch.cuda.current_stream().cuda_stream, ctypes.byref(launches))
    torch.cuda.synchronize()
    assert rc == 0 and launches.value == 1


# ---- end to end: fill + the library's horizontal diffusion, against numpy.pad + the oracle -----------------------------------
def _time_loop(domain, steps, modes):
    import gt4py_amd.storage as gt_storage
    from gt4py_amd import boundary
    from gt4py_amd.cartesian import gtscript
    from gt4py_amd.cartesian.backend import hip_templates

    backend = "hip:mi300"
    rng = np.random.default_rng(2024)
    shape = (domain[0] + 4, domain[1] + 4, domain[2])
    u0 = np.zeros(shape, np.float32)
    u0[2:-2, 2:-2] = rng.uniform(-10, 10, domain).astype(np.float32)
    coeff = rng.uniform(0, 0.5, shape).astype(np.float32)
    hd = gtscript.stencil(backend=backend, definition=hip_templates.hdiff_limiter_field, dtypes={"T": np.float32})
    d_a, d_b, d_c = (gt_storage.from_array(x, np.float32, backend=backend, aligned_index=(2, 2, 0)) for x in (u0, u0, coeff))
    fills = {id(d): boundary.HaloFill([d], halo=2, mode=modes) for d in (d_a, d_b)}
    src, dst = d_a, d_b
    for _ in range(steps):
        fills[id(src)]()
        hd(src, dst, d_c, origin=(2, 2, 0))
        src, dst = dst, src
    got = src.get()
    # host: numpy.pad axis by axis + the oracle's horizontal diffusion
    pad_mode = [R.NUMPY_PAD[m] for m in modes]
    h_src, h_dst = u0.copy(), u0.copy()
    for _ in range(steps):
        inner = h_src[2:-2, 2:-2]
        padded = np.pad(np.pad(inner, ((2, 2), (0, 0), (0, 0)), mode=pad_mode[0]), ((0, 0), (2, 2), (0, 0)), mode=pad_mode[1])
        h_src[...] = padded
        ORACLE.hdiff(h_src, h_dst, coeff)
        h_src, h_dst = h_dst, h_src
    return got, h_src


@pytest.mark.parametrize("modes", [("periodic", "periodic"), ("periodic", "zero_gradient")])
def test_time_loop_is_bit_identical_to_numpy_pad_and_the_oracle(modes):
    import fullsize_util as F

    for domain, steps in (((40, 28, 5), 10), ((256, 256, 8), 3)):
        got, want = _time_loop(domain, steps, modes)
        F.assert_bitwise(got[2:-2, 2:-2], want[2:-2, 2:-2], f"{modes} {domain} x {steps} steps")


def test_frozen_fill_refuses_to_run_after_an_array_died():
    import gt4py_amd.storage as gt_storage
    from gt4py_amd import boundary

    a = gt_storage.zeros((12, 12, 4), backend="hip:mi300", aligned_index=(1, 1, 0))
    b = gt_storage.zeros((12, 12, 4), backend="hip:mi300", aligned_index=(1, 1, 0))
    bc = boundary.HaloFill([a, b], halo=1, mode="periodic")
    bc()
    assert bc.launches == 1
    del b
    gc.collect()
    with pytest.raises(RuntimeError, match="no longer exists"):
        bc()
